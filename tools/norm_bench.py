#!/usr/bin/env python3
"""--train_norm on against off on one box: bench.py's C2 workload (7B, 32 layers, bf16, B = 8, S = 128, VQA loss; the same
factory, optimizer, scaler and resident batches) built twice in one process — flag off is the parent's launch sequence — and
timed in interleaved pairs, then fvqa_rmsnorm_dw alone at the step's shape (R = B * S rows, D columns) with its GB/s
(2 * R * D storage values read per call; the chunk partials' round trip through the workspace is not counted).

usage: python tools/norm_bench.py [--pairs 3] [--steps 20] [--warmup 5] [--n_layers N] [--batch_size 8] [--seq_len 128]
Prints one line per arm and pair, a summary, and one JSON line."""
import argparse
import contextlib
import json
import os
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "flipped-vqa_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)
os.environ.setdefault("FVQA_SYNTHETIC_TOKENIZER", "1")

import torch  # noqa: E402


def build(a, train_norm, dev):
    import util.misc as misc
    from fvqa import synth
    from fvqa.optim import FusedAdamW, param_groups_weight_decay
    from fvqa.step import stage_batch
    from llama_vqa import LLaMA_VQA
    args = types.SimpleNamespace(
        llama_model_path="/nonexistent/", model="7B", max_seq_len=a.seq_len, adapter_len=10, adapter_layer=a.n_layers or 32,
        max_feats=10, bias=3.5, tau=100.0, vaq=False, qav=False, audio=False, audio_only=False, audio_merge="none", debug=False,
        synthetic=True, random_init=True, dtype="bf16", accum_iter=1, weight_decay=0.14, train_norm=train_norm)
    kw = {"n_layers": a.n_layers} if a.n_layers else {}
    with contextlib.redirect_stdout(sys.stderr):
        model = LLaMA_VQA(args, **kw)
    model.to(dev)
    opt = FusedAdamW(param_groups_weight_decay(model, args.weight_decay), lr=9e-2 * a.batch_size / 256, betas=(0.9, 0.95),
                     flat=model.flat_params())
    scaler = misc.NativeScalerWithGradNormCount()
    p = model.params
    cfg = synth.SynthConfig(dim=p.dim, n_heads=p.n_heads, n_layers=p.n_layers, vocab_size=model.vocab_size,
                            max_seq_len=a.seq_len, batch_size=a.batch_size)
    batches = [stage_batch(synth.make_batch(cfg, seed=1234 + i), dev) for i in range(4)]

    def one_step(i):
        opt.zero_grad()
        vqa, vaq, qav = model(batches[i % 4])
        scaler(vqa + vaq + qav, opt, parameters=None, update_grad=True)

    return model, one_step


def timed(step, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(n):
        step(i)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / n


def kernel_alone(rows, dim, reps=200):
    from fvqa import ops
    g = torch.randn(rows, dim, device="cuda").to(torch.bfloat16)
    x = torch.randn(rows, dim, device="cuda").to(torch.bfloat16)
    rstd = torch.rsqrt(x.float().pow(2).mean(-1) + 1e-6)
    dw = torch.zeros(dim, device="cuda")
    ws = torch.empty(ops.rmsnorm_dw_workspace(rows, dim, torch.bfloat16), dtype=torch.uint8, device="cuda")
    for _ in range(10):
        ops.rmsnorm_dw(g, x, rstd, dw, ws, True)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        ops.rmsnorm_dw(g, x, rstd, dw, ws, True)
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) * 1e3 / reps
    return us, 2 * rows * dim * 2 / (us * 1e-6) / 1e9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--n_layers", type=int, default=0, help="reduced depth (a rehearsal, not the reported workload)")
    ap.add_argument("--batch_size", type=int, default=8)
    ap.add_argument("--seq_len", type=int, default=128)
    ap.add_argument("--kernel_only", action="store_true", help="time fvqa_rmsnorm_dw alone (7B width) and stop")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    if a.kernel_only:
        us, gbs = kernel_alone(a.batch_size * a.seq_len, 4096)
        print(f"[norm_bench] fvqa_rmsnorm_dw alone at ({a.batch_size * a.seq_len}, 4096) bf16: {us:.1f} us per call, {gbs:.0f} GB/s", flush=True)
        return
    m_off, step_off = build(a, False, dev)
    m_on, step_on = build(a, True, dev)
    L, D = m_on._engine.L, m_on._engine.D
    print(f"[norm_bench] two models built, {torch.cuda.memory_allocated() / 2**30:.1f} GiB allocated; trainables "
          f"{m_off.flat_params().flat.numel()} -> {m_on.flat_params().flat.numel()} (+{(2 * L + 1) * D})", flush=True)
    for step in (step_off, step_on):
        timed(step, a.warmup)
    off, on = [], []
    for k in range(a.pairs):
        off.append(timed(step_off, a.steps))
        on.append(timed(step_on, a.steps))
        print(f"[norm_bench] pair {k + 1}: off {off[-1]:.3f} ms/step   on {on[-1]:.3f} ms/step   +{on[-1] - off[-1]:.3f} ms", flush=True)
    for m in (m_off, m_on):
        m._engine.check_gemm_error()
    us, gbs = kernel_alone(a.batch_size * a.seq_len, D)
    mean = lambda v: sum(v) / len(v)      # noqa: E731
    print(f"[norm_bench] mean off {mean(off):.3f} ms, on {mean(on):.3f} ms, +{mean(on) - mean(off):.3f} ms for {2 * L + 1} reductions; "
          f"fvqa_rmsnorm_dw alone at ({a.batch_size * a.seq_len}, {D}) bf16: {us:.1f} us per call (two launches), {gbs:.0f} GB/s", flush=True)
    print(json.dumps(dict(metric="train_norm_step_ms", off_ms=off, on_ms=on, off_mean_ms=mean(off), on_mean_ms=mean(on),
                          reductions=2 * L + 1, dw_us=us, dw_gb_per_s=gbs, layers=L, batch_size=a.batch_size, seq_len=a.seq_len)),
          flush=True)


if __name__ == "__main__":
    main()
