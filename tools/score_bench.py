#!/usr/bin/env python3
"""Option-scoring measurement on the MI355X box (fvqa/score.py): `score_options` in both routes on a make_option_batch —
7B full depth, bf16, B = 8, five options, S = 128 by default — interleaved (shared, dense, shared, dense ...) after a warm-up
of each, every call bracketed by device events; the shared route's prompt pass and suffix pass on their own; which GEMM kernel
took the suffix rows' projections (the library's launch record + fvqa_gemm_sk_describe). With --errors: the per-option-mean
errors of both routes against the reference-generated 7B-width fixture in bf16 and fp16 — the figures the bounds of
tests/test_score_gpu.py are set from. With --frame_attention: the cost of score_options(frame_attention=True), the keyword off and
on in interleaved pairs on both routes (profiles/score_frame_attention.log). Everything is appended to --log
(profiles/score_options.log)."""
import argparse
import ctypes as C
import os
import statistics
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "flipped-vqa_amd"))
os.environ.setdefault("FVQA_SYNTHETIC_TOKENIZER", "1")
import numpy as np  # noqa: E402
import torch  # noqa: E402

import llama  # noqa: E402
from fvqa import _lib, build, ops, score, synth  # noqa: E402
from llama_vqa import fill_closed_form  # noqa: E402

PIN = "score_7b_l2_peakedperm"


def make_model(cfg, dtype):
    args = types.SimpleNamespace(
        max_feats=cfg.max_feats, bias=cfg.bias, tau=cfg.tau, llama_model_path="/nonexistent/", vaq=False, qav=False,
        synthetic=True, vocab_size=cfg.vocab_size, audio=False, audio_only=False, audio_merge="none", debug=False)
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
        p.requires_grad = synth.is_trainable(n)
        if p.requires_grad:
            p.data = p.data.float()
    fill_closed_form(model, cfg)
    return model.eval()


def ms(ev):
    return ev[1].elapsed_time(ev[2])


def timing(a, say):
    cfg = synth.preset("7b", vaq=False, qav=False, batch_size=a.batch_size, n_layers=a.n_layers, adapter_layer=a.n_layers)
    model = make_model(cfg, torch.bfloat16)
    eng = model.ensure_engine()
    batch = synth.make_option_batch(cfg, n_options=a.n_options, seed=1)
    plan = score.plan_options(batch["text_id"]["vqa"], batch["label"]["vqa"], batch["prefix_index"]["vqa"],
                              batch["video_start"]["vqa"], cfg.max_feats)
    B, O, S, T = a.batch_size, a.n_options, cfg.max_seq_len, plan.T
    rows_sh, rows_de = B * S + B * O * T, B * O * S
    say(f"shape: 7B width, {a.n_layers} layers, bf16, B={B}, O={O}, S={S}; suffix rows per option T={T} "
        f"(lengths {plan.length.tolist()}), scored rows {plan.rows.shape[0]}")
    say(f"rows through the layers: shared {rows_sh} (prompt {B * S} + suffix {B * O * T}), dense {rows_de}: "
        f"{rows_de / rows_sh:.2f}x fewer")
    for r in ("shared", "dense"):
        for _ in range(a.warmup):
            score.score_options(eng, batch, route=r)
    torch.cuda.synchronize()
    # outputs of the two routes on this batch (faster and different is not faster)
    rs, rd = score.score_options(eng, batch, route="shared"), score.score_options(eng, batch, route="dense")
    d = float(((rs["mean"] - rd["mean"]).abs() / rd["mean"].abs()).max())
    say(f"outputs: per-option mean, shared vs dense, largest relative difference {d:.3e}; predictions equal on "
        f"{int((rs['prediction'] == rd['prediction']).sum())} of {B} samples; counts equal: "
        f"{bool(torch.equal(rs['count'], rd['count']))}")
    total = {"shared": [], "dense": []}
    parts = {"prompt pass": [], "suffix pass": []}
    for _ in range(a.reps):
        for r in ("shared", "dense"):
            ev = []
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            score.score_options(eng, batch, route=r, events=ev)
            e1.record()
            e1.synchronize()
            total[r].append(e0.elapsed_time(e1))
            for x in ev:
                if x[0] in parts:
                    parts[x[0]].append(ms(x))
    med = {k: statistics.median(v) for k, v in {**total, **parts}.items()}
    for k in ("shared", "dense"):
        v = total[k]
        say(f"score_options {k:6s}: median {med[k]:8.3f} ms  min {min(v):8.3f}  max {max(v):8.3f}  ({a.reps} reps, interleaved)")
    say(f"  shared route, prompt pass alone: median {med['prompt pass']:8.3f} ms; suffix pass alone (layers on "
        f"{B * O * T} rows + head on the scored rows + pick): median {med['suffix pass']:8.3f} ms")
    say(f"  dense / shared = {med['dense'] / med['shared']:.2f}x")
    # which GEMM kernel took the suffix rows' projections
    R = B * O * T
    ops.gemm_timing_enable(True, 1)
    try:
        score.score_options(eng, batch, route="shared")
        rec = ops.gemm_timing_read()
    finally:
        ops.gemm_timing_enable(False)
    fl = {"qkv": 2.0 * R * 3 * eng.D * eng.D, "wo": 2.0 * R * eng.D * eng.D, "w13": 2.0 * R * 2 * eng.Hf * eng.D,
          "w2": 2.0 * R * eng.D * eng.Hf}
    say(f"launch record of one shared call: {len(rec)} launches of the persistent GEMM kernels")
    for name, f in fl.items():
        mine = [(us, k) for (us, flops, k) in rec if abs(flops - f) < 1.0]
        if not mine:
            say(f"  {name:4s} ({R} rows): not the persistent kernel (no launch of {f:.3g} FLOP in the record): the 128 x 128 kernel")
            continue
        kinds = sorted({k for _, k in mine})
        us = statistics.median([u for u, _ in mine if u >= 0] or [float('nan')])
        what = ["4-wave whole-tile kernel" if k & 128 else "persistent 256-row kernel" + (", split-K" if k & 16 else "")
                for k in kinds]
        say(f"  {name:4s} ({R} rows): {len(mine)} launches, kind {kinds} = {what}, median {us:.1f} us")
    keys = ("tm", "tn", "nw_tile", "gran", "gpt", "ts", "mgroups", "n_teams", "full", "rem", "s", "pstride")
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    for name, (N, K) in {"qkv": (3 * eng.D, eng.D), "wo": (eng.D, eng.D), "w13": (2 * eng.Hf, eng.D),
                         "w2": (eng.D, eng.Hf)}.items():
        plan_ = (C.c_int32 * 16)()
        _lib.load().fvqa_gemm_sk_describe(R, N, K, _lib.BF16, min(n_cu, 256), C.cast(plan_, C.c_void_p), -1, None, 0)
        say(f"  fvqa_gemm_sk_describe({R}, {N}, {K}): " + " ".join(f"{k}={v}" for k, v in zip(keys, plan_)))
    return med


def frame_attention_cost(a, say):
    """What score_options(frame_attention=True) costs: the keyword off and on, interleaved in pairs, on both routes (the shared
    route swaps fvqa_attn_suffix for fvqa_attn_suffix_mass in every layer; the dense route adds one fvqa_attn_row_mass launch
    per layer on its arena) — 7B, full depth, bf16, B x five options as `timing`."""
    if a.reps < 3:
        sys.exit("--frame_attention: at least 3 pairs (--reps)")
    cfg = synth.preset("7b", vaq=False, qav=False, batch_size=a.batch_size, n_layers=a.n_layers, adapter_layer=a.n_layers)
    model = make_model(cfg, torch.bfloat16)
    eng = model.ensure_engine()
    batch = synth.make_option_batch(cfg, n_options=a.n_options, seed=1)
    say(f"frame_attention cost: 7B width, {a.n_layers} layers, bf16, B={a.batch_size} x {a.n_options} options, S={cfg.max_seq_len}, "
        f"{a.reps} interleaved (off, on) pairs per route after {a.warmup} warm-up calls of each")
    for r in score.ROUTES:
        for kw in ({}, {"frame_attention": True}):
            for _ in range(a.warmup):
                out = score.score_options(eng, batch, route=r, **kw)
        torch.cuda.synchronize()
        fa = out["frame_attention"]
        t = {False: [], True: []}
        for _ in range(a.reps):
            for on in (False, True):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                score.score_options(eng, batch, route=r, **({"frame_attention": True} if on else {}))
                e1.record()
                e1.synchronize()
                t[on].append(e0.elapsed_time(e1))
        m0, m1 = statistics.median(t[False]), statistics.median(t[True])
        say(f"  {r:6s}: off median {m0:8.3f} ms (min {min(t[False]):8.3f}, max {max(t[False]):8.3f}); on median {m1:8.3f} ms "
            f"(min {min(t[True]):8.3f}, max {max(t[True]):8.3f}); on - off = {m1 - m0:+.3f} ms = {100 * (m1 - m0) / m0:+.2f} %; "
            f"frame_attention {tuple(fa.shape)}")


def errors(say):
    g = dict(np.load(os.path.join(ROOT, "tests", "golden", PIN + ".npz")))
    cfg = synth.preset("7b_l2", vaq=False, qav=False, vocab_size=32000, max_seq_len=128, batch_size=4, peaked_perm=True)
    batch = {"video": torch.from_numpy(g["video"]), "text_id": {"vqa": torch.from_numpy(g["text_id_vqa"])},
             "label": {"vqa": torch.from_numpy(g["label_vqa"])}, "video_start": {"vqa": g["vstart_vqa"].tolist()},
             "prefix_index": {"vqa": g["prefix_vqa"].tolist()}}
    say(f"errors against {PIN} (reference-generated; gaps {np.array2string(g['gap'], precision=5)}):")
    for dtype in (torch.float32, torch.bfloat16, torch.float16):
        model = make_model(cfg, dtype)
        eng = model.ensure_engine()
        for r in ("dense", "shared"):
            out = score.score_options(eng, batch, route=r)
            mean = out["mean"].cpu().numpy()
            e_mean = float((np.abs(mean - g["mean"]) / np.abs(g["mean"])).max())
            il = out["individual_losses"].cpu().numpy()
            e_il = float(np.abs(il - g["individual_losses"]).max() / np.abs(g["individual_losses"]).max())
            pred = out["prediction"].cpu().numpy()
            say(f"  {str(dtype):15s} {r:6s}: per-option mean, largest relative error {e_mean:.4e}; individual_losses / max "
                f"{e_il:.4e}; prediction {pred.tolist()} (fixture {g['prediction'].tolist()})")
        del model, eng
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch_size", type=int, default=8)
    ap.add_argument("--n_options", type=int, default=5)
    ap.add_argument("--n_layers", type=int, default=32)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--errors", action="store_true", help="also measure both routes' errors against the 7B-width fixture")
    ap.add_argument("--no_timing", action="store_true")
    ap.add_argument("--frame_attention", action="store_true",
                    help="measure score_options(frame_attention=True) against the call without it, interleaved, on both routes, and "
                         "nothing else (--log defaults to profiles/score_frame_attention.log)")
    ap.add_argument("--log", default=None)
    a = ap.parse_args()
    if a.log is None:
        a.log = os.path.join(ROOT, "profiles", "score_frame_attention.log" if a.frame_attention else "score_options.log")
    if not torch.cuda.is_available():
        sys.exit("score_bench.py measures on the GPU: no device found")
    os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
    log = open(a.log, "a")

    def say(s):
        print(s, flush=True)
        log.write(s + "\n")
        log.flush()

    say(f"# tools/score_bench.py on {torch.cuda.get_device_name(0)}, kernel sources {build.source_hash()[:12]}")
    with torch.no_grad():
        if a.frame_attention:
            frame_attention_cost(a, say)
            return
        if a.errors:
            errors(say)
        if not a.no_timing:
            timing(a, say)


if __name__ == "__main__":
    main()
