#!/usr/bin/env python3
"""TEST INFRASTRUCTURE — generates tests/golden/audio_train_*.npz: the REFERENCE in its audio modes with the audio half of the
front end TRAINABLE, which is what `--train_audio` makes of the product.

Works as tools/gen_golden_audio.py does (same shims, same closed-form parameters, same `run_case` of oracle/gen_golden.py,
nothing under oracle/ changes); the one difference: after `build_reference`, `requires_grad = True` on every parameter whose name
starts with `audio_proj.` or `video_audio_cross_attn.` — the parameters the reference's freeze filter (llama_vqa.py:72) misses.
`run_case` then stores their gradients with the others (whole when small, norm + sampled picks when large), and the records
  param_names / param_shapes / param_trainable   carry the widened freeze flags
  case_preset / case_over                        the SynthConfig the case was made from (JSON)

usage: python tools/gen_golden_audio_train.py [case ...]      (default: every case in CASES)
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "flipped-vqa_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import oracle.gen_golden as G  # noqa: E402
import gen_golden_audio as A  # noqa: E402

ALL = dict(vaq=True, qav=True)
C3 = dict(batch_size=8, peaked=True, **ALL)                 # BASELINE configs[2]: 7B width, B = 8, three streams
AUDIO_PREFIXES = ("audio_proj.", "video_audio_cross_attn.")
CASES = {
    "audio_train_tiny_only": ("tiny", dict(audio="only", **ALL)),
    "audio_train_tiny_sum": ("tiny", dict(audio="sum", **ALL)),
    "audio_train_tiny_attn1": ("tiny", dict(audio="attention", audio_len=1, **ALL)),   # one key: dq = dk = 0 exactly
    "audio_train_tiny_attn3": ("tiny", dict(audio="attention", audio_len=3, **ALL)),
    "audio_train_tiny_attnF": ("tiny", dict(audio="attention", **ALL)),                # T = max_feats
    "audio_train_7b_l2_b8_sum_peaked": ("7b_l2", dict(audio="sum", **C3)),
    "audio_train_7b_l2_b8_attnF_peaked": ("7b_l2", dict(audio="attention", **C3)),
}


def build_reference(M, cfg):
    """tools/gen_golden_audio.py's build_reference, then the audio front end switched to trainable."""
    model, args = A.build_reference(M, cfg)
    for n, p in model.named_parameters():
        if n.startswith(AUDIO_PREFIXES):
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
