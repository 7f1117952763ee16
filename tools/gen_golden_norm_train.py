#!/usr/bin/env python3
"""TEST INFRASTRUCTURE — generates tests/golden/norm_train_*.npz: the REFERENCE with its RMSNorm weights TRAINABLE, which is
what `--train_norm` makes of the product.

Works as tools/gen_golden_audio_train.py does (same shims, same closed-form parameters, same `run_case` of oracle/gen_golden.py,
nothing under oracle/ changes); the one difference: after `build_reference`, `requires_grad = True` on `norm.weight` and on every
`layers.N.attention_norm.weight` / `layers.N.ffn_norm.weight`. `run_case` then stores their gradients with the others, and a
layer the reference never walks (adapter_layer < n_layers, llama/model.py:338) leaves a `gradnone__` record: the product keeps
such a layer's norms frozen. The closed-form norm weights are 1 +- 0.1, so a dropped or doubled weight shows up. The records
  param_names / param_shapes / param_trainable   carry the widened freeze flags
  case_preset / case_over                        the SynthConfig the case was made from (JSON)

usage: python tools/gen_golden_norm_train.py [case ...]      (default: every case in CASES)
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "flipped-vqa_amd"))
import oracle.gen_golden as G  # noqa: E402

ALL = dict(vaq=True, qav=True)
C3 = dict(batch_size=8, peaked=True, **ALL)                 # BASELINE configs[2]: 7B width, B = 8, three streams
NORM_SUFFIXES = ("attention_norm.weight", "ffn_norm.weight")
CASES = {
    "norm_train_tiny_all": ("tiny", dict(**ALL)),
    "norm_train_tiny_vqa": ("tiny", dict(vaq=False, qav=False)),
    "norm_train_tiny_l3_a2_all": ("tiny", dict(n_layers=3, adapter_layer=2, **ALL)),      # layer 0 is never walked
    "norm_train_7b_l2_b8_all_peaked": ("7b_l2", dict(**C3)),
}
_build = G.build_reference


def build_reference(M, cfg):
    """oracle/gen_golden.py's build_reference, then the norm weights switched to trainable."""
    model, args = _build(M, cfg)
    for n, p in model.named_parameters():
        if n == "norm.weight" or (n.startswith("layers.") and n.endswith(NORM_SUFFIXES)):
            p.requires_grad = True
    build_reference.last = model
    return model, args


def main():
    names = sys.argv[1:] or list(CASES)
    M = G.install_shims()
    G.build_reference = build_reference                        # run_case looks it up in its module
    for name in names:
        pname, over = CASES[name]
        G.CASES[name] = (pname, over)
        G.run_case(M, name)
        path = os.path.join(ROOT, "tests", "golden", f"{name}.npz")
        out = dict(np.load(path))
        params = list(build_reference.last.named_parameters())
        out["param_names"] = np.array([n for n, _ in params])
        out["param_shapes"] = np.array(["x".join(str(int(d)) for d in p.shape) for _, p in params])
        out["param_trainable"] = np.array([bool(p.requires_grad) for _, p in params])
        out["case_preset"] = np.array(pname)
        out["case_over"] = np.array(json.dumps(over, sort_keys=True))
        np.savez_compressed(path, **out)
        print(f"[{name}] + {len(params)} parameter records -> {os.path.getsize(path) / 1024:.0f} KiB", flush=True)


if __name__ == "__main__":
    main()
