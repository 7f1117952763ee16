#!/usr/bin/env python3
"""Flipped-scoring measurement on the MI355X box (fvqa/flipped.py): `score_flipped` with every task dense and every task shared on
synthetic options with all three streams (synth.make_flipped_option_batch) — 7B full depth, bf16, B = 8, five options, S = 128,
questions of --question_len tokens (the VAQ suffix is the question + up to 6 rows) — interleaved (dense, shared) pairs after a
warm-up of each, the passes of every task bracketed by device events; fvqa_attn_suffix_wide alone at the VAQ suffix's shape, per
layer; which GEMM kernel took the suffix rows' projections. With --errors: the per-option-mean errors of both routes, per task,
against the reference-generated 7B-width fixture in fp32, bf16 and fp16 — the figures the bounds of tests/test_flipped_gpu.py are
set from. Everything is appended to --log (profiles/score_flipped.log). Sibling of tools/score_bench.py."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "flipped-vqa_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
os.environ.setdefault("FVQA_SYNTHETIC_TOKENIZER", "1")
import numpy as np  # noqa: E402
import torch  # noqa: E402

from fvqa import build, flipped, ops, rowpass, synth  # noqa: E402
from score_bench import make_model  # noqa: E402
from tests import flipped_util as FU  # noqa: E402

PIN = "flipped_7b_l2_peakedperm"


def errors(say):
    g = FU.load(PIN)
    say(f"errors against {PIN} (reference-generated; gaps vqa {np.array2string(g['gap_vqa'], precision=5)}, total "
        f"{np.array2string(g['gap_total'], precision=5)}); dense: the four samples, shared: the first three (the fourth's VAQ "
        "suffix is above 64 rows):")
    for dtype in (torch.float32, torch.bfloat16, torch.float16):
        model = make_model(FU.fixture_cfg(PIN), dtype)
        eng = model.ensure_engine()
        for route, samples in (("dense", None), ("shared", (0, 1, 2))):
            r = flipped.score_flipped(eng, FU.golden_batch(g, samples), route=route)
            idx = slice(None) if samples is None else list(samples)
            e = {t: float((np.abs(r[f"mean_{t}"].cpu().numpy() - g[f"mean_{t}"][idx]) / np.abs(g[f"mean_{t}"][idx])).max())
                 for t in flipped.TASKS}
            say(f"  {str(dtype):15s} {route:6s}: per-option mean, largest relative error " +
                "  ".join(f"{t} {e[t]:.4e}" for t in flipped.TASKS) + f"; prediction {r['prediction'].tolist()}")
        del model, eng
        torch.cuda.empty_cache()


def wide_alone(eng, B, O, T, S, say, reps=20):
    """fvqa_attn_suffix_wide on operands of the timed shape (values do not matter to its time), per launch = per layer."""
    dev, dt = eng.device, eng.dtype
    R, D = B * O * T, eng.D
    qkv = torch.randn(R, 3 * D, device=dev).to(dt)
    cache = torch.randn(B * S + eng.A, 3 * D, device=dev).to(dt)
    o = torch.empty(R, D, dtype=dt, device=dev)
    i32 = lambda v: torch.full((B,), v, dtype=torch.int32, device=dev)      # noqa: E731
    g = torch.zeros(eng.H, device=dev)
    args = (g, g, i32(19), i32(S - T - 8), i32(T), (eng.cos, eng.sin), B, O, T, S, eng.H, eng.Dh, eng.A, eng.F)
    for _ in range(3):
        ops.attn_suffix_wide(qkv, cache, o, *args, cache_rotated=rowpass.cache_rotated(eng))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        ops.attn_suffix_wide(qkv, cache, o, *args, cache_rotated=rowpass.cache_rotated(eng))
    e1.record()
    e1.synchronize()
    say(f"  fvqa_attn_suffix_wide alone, {R} suffix rows (B={B}, O={O}, T={T}), {S - T - 8} cached keys, H={eng.H}: "
        f"{1000 * e0.elapsed_time(e1) / reps:.1f} us per launch (= per layer; {reps} launches back to back)")


def timing(a, say, qlen, cfg, eng):
    batch = synth.make_flipped_option_batch(cfg, n_options=a.n_options, seed=1, question_len=(qlen, qlen + 3))
    B, O, S = batch["text_id"]["vaq"].shape
    for r in ("dense", "shared"):
        for _ in range(a.warmup):
            out = flipped.score_flipped(eng, batch, route=r)
    torch.cuda.synchronize()
    T = {t: out["plan"][t].T for t in flipped.TASKS}
    say(f"shape: 7B width, {a.n_layers} layers, bf16, B={B}, O={O}, S={S}, questions of {qlen}..{qlen + 2} tokens; suffix rows per "
        f"option T: {T} (+1 padding row for qav); rows through the layers per task: dense {B * O * S}, shared "
        + ", ".join(f"{t} {B * S + B * O * (T[t] + (t == 'qav'))}" for t in flipped.TASKS))
    rd, rs = flipped.score_flipped(eng, batch, route="dense"), flipped.score_flipped(eng, batch, route="shared")
    for t in flipped.TASKS:
        d = float(((rs[f"mean_{t}"] - rd[f"mean_{t}"]).abs() / rd[f"mean_{t}"].abs()).max())
        say(f"  outputs {t}: per-option mean, shared vs dense, largest relative difference {d:.3e}")
    say(f"  predictions by the total equal on {int((rs['prediction'] == rd['prediction']).sum())} of {B} samples")
    faster = {t: True for t in flipped.TASKS}
    for i in range(a.pairs):
        per = {}
        for r in ("dense", "shared"):
            ev = []
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            flipped.score_flipped(eng, batch, route=r, events=ev)
            e1.record()
            e1.synchronize()
            per[r] = {t: 0.0 for t in flipped.TASKS}
            for name, x0, x1 in ev:
                t = name.split()[0] if name.split()[0] in flipped.TASKS else "vqa"
                per[r][t] += x0.elapsed_time(x1)
            per[r]["call"] = e0.elapsed_time(e1)
        for t in flipped.TASKS:
            faster[t] = faster[t] and per["shared"][t] < per["dense"][t]
        say(f"  pair {i}: " + "; ".join(f"{t} dense {per['dense'][t]:7.3f} ms shared {per['shared'][t]:7.3f} ms" for t in flipped.TASKS)
            + f"; whole call dense {per['dense']['call']:7.3f} ms shared {per['shared']['call']:7.3f} ms")
    say(f"  shared faster than dense in every pair: {faster}")
    wide_alone(eng, B, O, T["vaq"], S, say)
    # which GEMM kernel took the VAQ suffix rows' projections
    R = B * O * T["vaq"]
    ops.gemm_timing_enable(True, 1)
    try:
        flipped.score_flipped(eng, batch, tasks=("vaq",), route="shared")
        rec = ops.gemm_timing_read()
    finally:
        ops.gemm_timing_enable(False)
    fl = {"qkv": 2.0 * R * 3 * eng.D * eng.D, "wo": 2.0 * R * eng.D * eng.D, "w13": 2.0 * R * 2 * eng.Hf * eng.D,
          "w2": 2.0 * R * eng.D * eng.Hf}
    for name, f in fl.items():
        mine = [(us, k) for (us, flops, k) in rec if abs(flops - f) < 1.0]
        if not mine:
            say(f"  {name:4s} ({R} rows): not the persistent kernel (no launch of {f:.3g} FLOP in the record): the 128 x 128 kernel")
            continue
        kinds = sorted({k for _, k in mine})
        us = statistics.median([u for u, _ in mine if u >= 0] or [float("nan")])
        what = ["4-wave whole-tile kernel" if k & 128 else "persistent 256-row kernel" + (", split-K" if k & 16 else "") for k in kinds]
        say(f"  {name:4s} ({R} rows): {len(mine)} launches, kind {kinds} = {what}, median {us:.1f} us")
    return faster


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch_size", type=int, default=8)
    ap.add_argument("--n_options", type=int, default=5)
    ap.add_argument("--n_layers", type=int, default=32)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--question_len", type=int, nargs="+", default=[19, 43], help="VAQ suffixes of about 24 and 48 rows")
    ap.add_argument("--errors", action="store_true", help="also measure both routes' errors against the 7B-width fixture")
    ap.add_argument("--no_timing", action="store_true")
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "score_flipped.log"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("flipped_bench.py measures on the GPU: no device found")
    os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
    log = open(a.log, "a")

    def say(s):
        print(s, flush=True)
        log.write(s + "\n")
        log.flush()

    say(f"# tools/flipped_bench.py on {torch.cuda.get_device_name(0)}, kernel sources {build.source_hash()[:12]}")
    with torch.no_grad():
        if a.errors:
            errors(say)
        if not a.no_timing:
            cfg = synth.preset("7b", vaq=True, qav=True, batch_size=a.batch_size, n_layers=a.n_layers, adapter_layer=a.n_layers)
            eng = make_model(cfg, torch.bfloat16).ensure_engine()
            for q in a.question_len:
                timing(a, say, q, cfg, eng)


if __name__ == "__main__":
    main()
