#!/usr/bin/env python3
"""Measurements behind profiles/audio_frontend.log: the step in one front-end mode, run from the repository root of the tree to
measure (the current one, or a checkout of an earlier commit — run from THAT root, mode `none`, the script itself may lie
anywhere):

    python tools/audio_frontend_profile.py --mode concat --steps 10 --warmup 3            # step time (HIP events), C2's shape
    rocprofv3 --kernel-trace --stats --output-format csv -d out -- \\
        python tools/audio_frontend_profile.py --mode concat --layers 2 --steps 5          # the front-end kernels' durations
    python tools/audio_frontend_profile.py --mode none --dump out.npz                      # losses + flat gradient of two
                                                                                           # video-only cases, for a bitwise diff
    python tools/audio_frontend_profile.py --diff a.npz b.npz
    python tools/audio_frontend_profile.py --mode attention --audio_len 10 --interleave 4  # profiles/audio_train.log: --train_audio
                                                                                           # off against on, alternating blocks
    rocprofv3 --kernel-trace --stats --output-format csv -d out -- \\
        python tools/audio_frontend_profile.py --mode attention --audio_len 10 --train_audio --layers 2 --steps 5

C2 is BASELINE configs[1]: 7B, B = 8, S = 128, bf16, VQA loss. `--layers 2` keeps width and batch and cuts the depth (the front end
does not see the depth)."""
import argparse
import json
import os
import sys
import types

import numpy as np

ROOT = os.getcwd()
for p in (os.path.join(ROOT, "flipped-vqa_amd"), ROOT):
    sys.path.insert(0, p)
os.environ.setdefault("FVQA_SYNTHETIC_TOKENIZER", "1")


def build(cfg, dtype, mode, train_audio=False):
    import torch
    import llama
    from fvqa import synth
    from llama_vqa import fill_closed_form
    audio = dict(audio=False, audio_only=False, audio_merge="none")
    if mode == "only":
        audio = dict(audio=True, audio_only=True, audio_merge=None)
    elif mode != "none":
        audio = dict(audio=True, audio_only=False, audio_merge=mode)
    args = types.SimpleNamespace(max_feats=cfg.max_feats, bias=cfg.bias, tau=cfg.tau, llama_model_path="/nonexistent/",
                                 vaq=cfg.vaq, qav=cfg.qav, synthetic=True, vocab_size=cfg.vocab_size, debug=False,
                                 adapter_len=cfg.adapter_len, adapter_layer=cfg.adapter_layer, max_seq_len=cfg.max_seq_len, train_audio=train_audio,
                                 **audio)
    ma = llama.ModelArgs(max_seq_len=cfg.max_seq_len, max_batch_size=32, adapter_len=cfg.adapter_len,
                         adapter_layer=cfg.adapter_layer, **cfg.params_json())
    ma.vocab_size = cfg.vocab_size
    prev = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        with torch.device("cuda"):
            model = llama.Transformer(ma, args)
    finally:
        torch.set_default_dtype(prev)
    for n, p in model.named_parameters():
        p.requires_grad = synth.is_trainable(n, getattr(model, "train_audio", False))
        if p.requires_grad:
            p.data = p.data.float()
    fill_closed_form(model, cfg)
    return model


def step(model, batch):
    flat = model.flat_params()
    flat.zero_grad()
    vqa, vaq, qav = model(batch)
    total = vqa + (vaq if model.args.vaq else 0) + (qav if model.args.qav else 0)
    total.sum().backward()
    return vqa, vaq, qav                                    # (device tensors: no host synchronisation inside a step)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="none", choices=["none", "only", "concat", "sum", "attention"])
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--train_audio", action="store_true", help="the audio half of the front end trains (train.py --train_audio)")
    ap.add_argument("--audio_len", type=int, default=1, help="audio rows per sample in mode attention (the dataset hands 1)")
    ap.add_argument("--interleave", type=int, default=0, metavar="ROUNDS",
                    help="flag off and flag on in ONE process: ROUNDS alternating blocks of --steps steps each")
    ap.add_argument("--dump")
    ap.add_argument("--diff", nargs=2)
    a = ap.parse_args()
    if a.diff:
        x, y = (dict(np.load(f)) for f in a.diff)
        same = sorted(x) == sorted(y) and all(x[k].tobytes() == y[k].tobytes() for k in x)
        print(json.dumps({"diff": a.diff, "arrays": len(x), "elements": int(sum(v.size for v in x.values())),
                          "bitwise_equal": bool(same)}))
        sys.exit(0 if same else 1)
    import torch
    from fvqa import build as fb
    from fvqa import synth
    from fvqa.step import stage_batch
    over = {} if a.mode == "none" else dict(audio=a.mode, audio_len=a.audio_len if a.mode == "attention" else 0)
    if a.dump:
        out = {}
        for name, pname, kw in (("tiny_all", "tiny", dict(vaq=True, qav=True)),
                                ("7b_l2_b8_vqa_peaked", "7b_l2", dict(batch_size=8, peaked=True))):
            cfg = synth.preset(pname, **kw)
            for dtype in (torch.float32, torch.bfloat16):
                model = build(cfg, dtype, "none")
                out[f"{name}__{dtype}__losses"] = np.array(
                    [float(x.detach()) for x in step(model, synth.make_batch(cfg, seed=0))], dtype=np.float64)
                torch.cuda.synchronize()
                out[f"{name}__{dtype}__flat_grad"] = model.flat_params().flat_grad.cpu().numpy()
                del model
                torch.cuda.empty_cache()
        np.savez(a.dump, **out)
        print(json.dumps({"dumped": a.dump, "sources": fb.source_hash()[:12], "arrays": len(out)}))
        return
    cfg = synth.preset("7b", n_layers=a.layers, adapter_layer=a.layers, batch_size=8, **over)
    batch = stage_batch(synth.make_batch(cfg, seed=0), torch.device("cuda"))
    if a.interleave:
        models = {flag: build(cfg, torch.bfloat16, a.mode, train_audio=flag) for flag in (False, True)}
        for m in models.values():
            for _ in range(a.warmup):
                step(m, batch)
        torch.cuda.synchronize()
        ms = {False: [], True: []}
        for _ in range(a.interleave):
            for flag, m in models.items():
                ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.steps)]
                for e0, e1 in ev:
                    e0.record()
                    step(m, batch)
                    e1.record()
                torch.cuda.synchronize()
                ms[flag] += [e0.elapsed_time(e1) for e0, e1 in ev]
        med = {flag: sorted(v)[len(v) // 2] for flag, v in ms.items()}
        print(json.dumps({"mode": a.mode, "audio_len": cfg.audio_rows if a.mode != "none" else 0, "layers": a.layers, "B": 8,
                          "S": cfg.max_seq_len, "dtype": "bf16", "steps_each": a.steps * a.interleave,
                          "off_ms_median": round(med[False], 3), "on_ms_median": round(med[True], 3),
                          "off_ms_min": round(min(ms[False]), 3), "on_ms_min": round(min(ms[True]), 3),
                          "on_minus_off_ms": round(med[True] - med[False], 3), "sources": fb.source_hash()[:12]}))
        return
    model = build(cfg, torch.bfloat16, a.mode, train_audio=a.train_audio)
    for _ in range(a.warmup):
        losses = step(model, batch)
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.steps)]
    for e0, e1 in ev:
        e0.record()
        step(model, batch)
        e1.record()
    torch.cuda.synchronize()
    ms = sorted(e0.elapsed_time(e1) for e0, e1 in ev)
    print(json.dumps({"mode": a.mode, "train_audio": bool(getattr(model, "train_audio", False)), "layers": a.layers, "B": 8, "S": cfg.max_seq_len, "dtype": "bf16", "steps": a.steps,
                      "step_ms_median": round(ms[len(ms) // 2], 3), "step_ms_min": round(ms[0], 3),
                      "loss_vqa": float(losses[0].detach()), "sources": fb.source_hash()[:12]}))


if __name__ == "__main__":
    main()
