#!/usr/bin/env python3
"""Measurements behind profiles/audio_frontend.log: the step in one front-end mode, run from the repository root of the tree to
measure (the current one, or a checkout of an earlier commit — run from THAT root, mode `none`, the script itself may lie
anywhere):

    python tools/audio_frontend_profile.py --mode concat --steps 10 --warmup 3            # step time (HIP events), C2's shape
    rocprofv3 --kernel-trace --stats --output-format csv -d out -- \\
        python tools/audio_frontend_profile.py --mode concat --layers 2 --steps 5          # the front-end kernels' durations
    python tools/audio_frontend_profile.py --mode none --dump out.npz                      # losses + flat gradient of two
                                                                                           # video-only cases, for a bitwise diff
    python tools/audio_frontend_profile.py --diff a.npz b.npz                              # (--dump honours --mode, --audio_len,
                                                                                           # --train_audio: profiles/front_refactor.log)
    python tools/audio_frontend_profile.py --hashes > tree.txt                             # one sha256 per output of the projection
                                                                                           # entries; compare two trees with diff
    python tools/audio_frontend_profile.py --direct --steps 50                             # the wave-per-feature forward at R = 160
    python tools/audio_frontend_profile.py --preset 13b --layers 2 --steps 5               # the timed step at the 13B width
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


VP_SHAPES = [(128, 8, 64, 520), (120, 10, 832, 512), (129, 3, 768, 520), (160, 10, 768, 512), (30, 10, 1792, 40),
             (30, 10, 100, 24)]                           # tests/test_rowops_edges_gpu.py


def hashes():
    """One sha256 per output tensor of the projection entries, inputs from fixed host seeds, accumulating outputs from a fixed
    non-zero start: the text of two trees is compared with diff. Shapes as tests/test_rowops_edges_gpu.py (VP_SHAPES) and the
    layouts of tests/test_audio_gpu.py at 80 (MFMA), 129 and 160 rows (wave per feature)."""
    import hashlib
    import math
    import torch
    from fvqa import ops

    def rnd(*shape, seed, scale=1.0):
        return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).cuda()

    def put(name, *ts):
        torch.cuda.synchronize()
        for i, t in enumerate(ts):
            b = t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32).cpu().numpy().tobytes()
            print(f"{name}[{i}] {hashlib.sha256(b).hexdigest()}")

    for R, F, K, D in VP_SHAPES:
        video, W, temp = rnd(R, K, seed=1), rnd(D, K, seed=2, scale=1 / math.sqrt(K)), rnd(F, D, seed=3)
        for dtype in (torch.float32, torch.bfloat16):
            raw, tok = torch.empty(R, D, device="cuda"), torch.empty(R, D, dtype=dtype, device="cuda")
            ops.visual_proj_fwd(video, W, temp, raw, tok)
            put(f"visual_proj_fwd {R},{F},{K},{D} {dtype}", raw, tok)
            ops.av_proj_fwd([(video, W)], raw, temporal=temp, out_tok=tok)       # the same operands through the other entry
            put(f"av_proj_fwd of the same {R},{F},{K},{D} {dtype}", raw, tok)
        d_tok, d_qav = rnd(R, D, seed=4), rnd(R, D, seed=5)
        for dq in (d_qav, None):
            dW, dT = rnd(D, K, seed=6), rnd(F, D, seed=7)
            ops.visual_proj_bwd(d_tok, dq, video, dW, dT)
            put(f"visual_proj_bwd {R},{F},{K},{D} d_qav={dq is not None}", dW, dT)
    KV, KA, D = 768, 1024, 520
    for R, F in ((80, 10), (129, 3), (160, 10)):
        v, a, wide = rnd(R, KV, seed=11), rnd(R, KA, seed=12), rnd(R, KV + KA, seed=13)
        Wc, Wv, Wa = (rnd(D, k, seed=14 + i, scale=1 / math.sqrt(k)) for i, k in enumerate((KV + KA, KV, KA)))
        layouts = {"one": [(v, Wv)], "concat": [(v, Wc[:, :KV]), (a, Wc[:, KV:])], "sum": [(a, Wa), (v, Wv)], "wide": [(wide, Wc)]}
        bias, temp = rnd(D, seed=17, scale=0.05), rnd(F, D, seed=18)
        g2 = rnd(R, 2 * D, seed=19)                          # the gradient of av_linear_bwd: a column range of a wider matrix
        d_tok, d_qav = rnd(R, D, seed=20), rnd(R, D, seed=21)
        for name, srcs in layouts.items():
            for dtype in (torch.float32, torch.bfloat16):
                raw, tok = torch.empty(R, D, device="cuda"), torch.empty(R, D, dtype=dtype, device="cuda")
                ops.av_proj_fwd(srcs, raw, bias=bias, temporal=temp, out_tok=tok)
                put(f"av_proj_fwd {name} R={R} {dtype}", raw, tok)
            raw = torch.empty(R, D, device="cuda")
            ops.av_proj_fwd(srcs, raw)
            put(f"av_proj_fwd {name} R={R} no bias, no tok", raw)
            for entry in ("av_proj_bwd", "av_linear_bwd"):
                G = [rnd(D, KV + KA, seed=22), rnd(D, KV + KA, seed=23)]     # gradients laid out as the weights are
                gs = {"one": [(v, G[0][:, :KV])], "concat": [(v, G[0][:, :KV]), (a, G[0][:, KV:])],
                      "sum": [(a, G[0][:, :KA]), (v, G[1][:, KA:])], "wide": [(wide, G[0])]}[name]
                if entry == "av_proj_bwd":
                    dT = rnd(F, D, seed=24)
                    ops.av_proj_bwd(d_tok, d_qav, gs, dT)
                    put(f"av_proj_bwd {name} R={R}", dT, *G)
                else:
                    db = rnd(D, seed=25)
                    ops.av_linear_bwd(g2[:, D:], gs, dbias=db)
                    put(f"av_linear_bwd {name} R={R}", db, *G)


def direct(steps):
    """The wave-per-feature forward on the one shape family of the project that reaches it (batch 16 at ten frames: R = 160,
    K = 768, D = 4096, bf16 tokens), through the video-only entry and through av_proj_fwd on the same operands."""
    import math
    import torch
    from fvqa import ops
    R, F, K, D = 160, 10, 768, 4096
    g = torch.Generator().manual_seed(1)
    video, W, temp = (torch.randn(*s, generator=g).cuda() for s in ((R, K), (D, K), (F, D)))
    W *= 1 / math.sqrt(K)
    raw, tok = torch.empty(R, D, device="cuda"), torch.empty(R, D, dtype=torch.bfloat16, device="cuda")
    calls = {"visual_proj_fwd": lambda: ops.visual_proj_fwd(video, W, temp, raw, tok),
             "av_proj_fwd": lambda: ops.av_proj_fwd([(video, W)], raw, temporal=temp, out_tok=tok)}
    us = {k: [] for k in calls}
    for _ in range(3):                                      # alternating blocks
        for k, f in calls.items():
            f()
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
            for e0, e1 in ev:
                e0.record()
                f()
                e1.record()
            torch.cuda.synchronize()
            us[k] += [1e3 * e0.elapsed_time(e1) for e0, e1 in ev]
    print(json.dumps({"direct": [R, F, K, D], "dtype": "bf16", "calls_each": 3 * steps,
                      **{f"{k}_us_{q}": round(f(v), 1) for k, v in us.items()
                         for q, f in (("min", min), ("median", lambda x: sorted(x)[len(x) // 2]), ("max", max))}}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="none", choices=["none", "only", "concat", "sum", "attention"])
    ap.add_argument("--preset", default="7b", choices=["7b", "13b"], help="the width of the timed step (batch 8 either way)")
    ap.add_argument("--hashes", action="store_true", help="one sha256 per output of the projection entries (kernel-level bits)")
    ap.add_argument("--direct", action="store_true", help="the wave-per-feature forward at R = 160, called directly, --steps times")
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
    if a.hashes:
        return hashes()
    if a.direct:
        return direct(a.steps)
    over = {} if a.mode == "none" else dict(audio=a.mode, audio_len=a.audio_len if a.mode == "attention" else 0)
    if a.dump:
        out = {}
        for name, pname, kw in (("tiny_all", "tiny", dict(vaq=True, qav=True)),
                                ("7b_l2_b8_vqa_peaked", "7b_l2", dict(batch_size=8, peaked=True)),
                                ("13b_l2_all", "13b", dict(n_layers=2, adapter_layer=2, vaq=True, qav=True))):
            cfg = synth.preset(pname, **kw, **over)
            for dtype in (torch.float32, torch.bfloat16):
                model = build(cfg, dtype, a.mode, train_audio=a.train_audio)
                out[f"{name}__{dtype}__losses"] = np.array(
                    [float(x.detach()) for x in step(model, synth.make_batch(cfg, seed=0))], dtype=np.float64)
                torch.cuda.synchronize()
                out[f"{name}__{dtype}__flat_grad"] = model.flat_params().flat_grad.cpu().numpy()
                del model
                torch.cuda.empty_cache()
        np.savez(a.dump, **out)
        print(json.dumps({"dumped": a.dump, "sources": fb.source_hash()[:12], "arrays": len(out)}))
        return
    cfg = synth.preset(a.preset, n_layers=a.layers, adapter_layer=a.layers, batch_size=8, **over)
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
