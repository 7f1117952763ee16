#!/usr/bin/env python3
"""TEST INFRASTRUCTURE — generates tests/golden/audio_*.npz by running the REFERENCE itself in its audio modes.

Runs only where the reference checkout is (oracle/gen_golden.py's REF). It imports the reference in-process with the three
shims of oracle/gen_golden.py (`install_shims`: Tensor.cuda -> identity, stub tokenizer, fp32 for .half()), builds its
`Transformer` with the audio arguments (llama/model.py:209-227), overwrites EVERY parameter — the frozen audio_proj and
cross-attention included — with the closed form of fvqa/synth.py, runs forward + backward on `synth.make_batch` and stores what
oracle/gen_golden.py stores (its `run_case`, unchanged: losses, argmax, sampled logits and margins, layer checksums, trainable
gradients incl. `gradnone__` marks), plus
  param_names / param_shapes / param_trainable   the reference's state-dict names, shapes and requires_grad flags after the
                                                 freeze policy of llama_vqa.py:72 (tests compare the product model against them)
  case_preset / case_over                        the SynthConfig the case was made from (JSON)

usage: python tools/gen_golden_audio.py [case ...]      (default: every case in CASES)
"""
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "flipped-vqa_amd"))
from fvqa import synth  # noqa: E402
import oracle.gen_golden as G  # noqa: E402

ALL = dict(vaq=True, qav=True)
C3 = dict(batch_size=8, peaked=True, **ALL)                 # BASELINE configs[2]: 7B width, B = 8, three streams
CASES = {
    "audio_tiny_only": ("tiny", dict(audio="only", **ALL)),
    "audio_tiny_concat": ("tiny", dict(audio="concat", **ALL)),
    "audio_tiny_sum": ("tiny", dict(audio="sum", **ALL)),
    "audio_tiny_attn1": ("tiny", dict(audio="attention", audio_len=1, **ALL)),       # the dataset's shape: one audio row per sample
    "audio_tiny_attnF": ("tiny", dict(audio="attention", **ALL)),                    # T = max_feats: a real softmax
    "audio_7b_l2_b8_concat_peaked": ("7b_l2", dict(audio="concat", **C3)),
    "audio_7b_l2_b8_attn1_peaked": ("7b_l2", dict(audio="attention", audio_len=1, **C3)),
}


def reference_audio_args(cfg) -> dict:
    """SynthConfig.audio -> the reference's three arguments, as train.py leaves them after its validation."""
    if cfg.audio == "none":
        return dict(audio=False, audio_only=False, audio_merge="none")
    if cfg.audio == "only":
        return dict(audio=True, audio_only=True, audio_merge=None)
    return dict(audio=True, audio_only=False, audio_merge=cfg.audio)


def build_reference(M, cfg):
    """oracle/gen_golden.py's build_reference with the audio arguments."""
    args = types.SimpleNamespace(
        max_feats=cfg.max_feats, bias=cfg.bias, tau=cfg.tau, llama_model_path="/nonexistent/",
        vaq=cfg.vaq, qav=cfg.qav, debug=False, adapter_len=cfg.adapter_len, adapter_layer=cfg.adapter_layer,
        max_seq_len=cfg.max_seq_len, **reference_audio_args(cfg))
    ma = M.ModelArgs(max_seq_len=cfg.max_seq_len, max_batch_size=2, adapter_len=cfg.adapter_len,
                     adapter_layer=cfg.adapter_layer, **cfg.params_json())
    ma.vocab_size = cfg.vocab_size
    torch.manual_seed(0)
    saved = {}
    for fn in ("kaiming_uniform_", "normal_", "uniform_"):      # every tensor is overwritten below
        saved[fn] = getattr(torch.nn.init, fn)
        setattr(torch.nn.init, fn, lambda t, *a, **k: t)
    try:
        model = M.Transformer(ma, args)
    finally:
        for fn, f in saved.items():
            setattr(torch.nn.init, fn, f)
    spec = {n: (shape, kind) for n, shape, kind in synth.state_spec(cfg)}
    own = {n: tuple(p.shape) for n, p in model.named_parameters()}
    assert own == {n: tuple(s) for n, (s, _) in spec.items()}, set(own) ^ set(spec)
    with torch.no_grad():
        for n, p in model.named_parameters():
            shape, kind = spec[n]
            p.data = synth.make_tensor(cfg, n, shape, kind)
    for n, p in model.named_parameters():                      # llama_vqa.py:71-76
        p.requires_grad = synth.is_trainable(n)
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
