#!/usr/bin/env python3
"""Headline benchmark: Flipped-VQA training samples/s on MI355X (BASELINE.json metric).

  python bench.py [--gpus N --steps K --warmup W] [--dump-outputs DIR] [--full]     (N>1: launched by torch.distributed.run)

A plain run sets up, warms up, times the K steps, writes the outputs of the last timed step if asked and prints the line;
everything that takes runs or legs of its own (the instrumented `roofline` passes, `other_configs`, `cpu_baseline`) runs only
with --full.

--dump-outputs DIR: after the timed steps (before anything --full adds), rank 0 writes what the last timed step handed its
caller as DIR/<name>.npy (float32, 64 MB at most, see OUTPUTS): the three losses, the gradient norm, the trainables after
AdamW and their gradients. Weights are closed-form and batches seeded, so equal arguments give equal inputs on every run.

One step = one full training step of the hot path on one synthetic batch already resident in
HBM: LLaMA-Adapter forward over the frame-spliced token stream, the flipped loss(es), backward,
loss-scaler unscale + grad norm, [RCCL all-reduce of the flat trainable gradient], AdamW.
Workload at N=1 = BASELINE configs[1]: LLaMA-7B (random-init, closed-form), bf16, seq_len 128,
batch 8 per GPU, max_feats 10, VQA loss only. N>1 = the same per-GPU work on every rank (weak
scaling), one all-reduce(mean) of 4.5 M fp32 gradients per step.

Prints ONE JSON line (rank 0) with the contract fields and step_roofline, plus with --full
  roofline     — the dominant kernel family (the bf16 projection GEMMs: the 4-wave whole-tile kernel gemm4w_k
                 and the split-K kernel gemm_sk_256, every launch of every instantiation): algorithmic
                 FLOPs / launch time against the 2.5 PFLOP/s dense bf16 MFMA peak. Launch times come from
                 HIP events the library records on the launch stream around every 17th launch in an
                 INSTRUMENTED repeat of the same steps under the same native schedule (that pass's own
                 ms_per_step is in the line; a pass with every launch bracketed is reported as
                 `dense_probe`). An empty event pair's ~4.8 us (measured in the same process) is taken off every bracket:
                 round 5 checked that against `rocprofv3 --kernel-trace --stats` of the SAME run (tools/rocprof_frac.py,
                 profiles/r05_rocprof_frac.json): bracket - empty pair = rocprof's kernel duration to 0.1 %, the bracket as
                 measured reads 5 % long (`frac_brackets_as_measured`). Kernel durations cover ~96.5 % of a step; the rest
                 are the ~480 kernel boundaries of a step (~1.9 us each), which `non_gemm_ms_per_step` contains; `alg_bytes_per_launch` (operands + outputs of each launch, from its shape)
                 stands beside `traffic` (fabric bytes per launch from the committed PMC passes);
  step_roofline— (every run) algorithmic FLOPs of the whole step (SURVEY §8d formula) / step time;
  cpu_baseline — the CPU oracle (oracle/ref_cpu.py) timed on this host's cores on BASELINE configs[0]:
                 full-depth 7B, B=2, all three losses, forward+backward+AdamW, one warm-up + timed steps within a
                 host-time budget (rank 0, N=1 only; ONE timed step while the other-config legs are on);
  other_configs— (N=1, default workload only) short legs — 3 warm-up + 10 timed steps each, same step, same GPU, after the
                 C2 legs have freed their model — of BASELINE configs[2..4] as ONE GPU runs them: c3 = 7B three losses,
                 c4 = 7B seq_len 650 batch 1 three losses, c5 = 13B batch 4 three losses: {ms_per_step, samples_per_s,
                 step_roofline} each (what profiles/r0N_bench_c{3,4,5}.json used to hold builder-run only).
"""
import argparse
import json
import os
import sys
import time
import types

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "flipped-vqa_amd"))
sys.path.insert(0, ROOT)
os.environ.setdefault("FVQA_SYNTHETIC_TOKENIZER", "1")

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

MFMA_BF16_PEAK = 2.5e15      # dense, /opt/skills/guides/MI355X_MICROARCH.md
HBM_PEAK = 8.0e12


def step_flops(D, H, L, Hf, V, N, S, A, F, tasks):
    """Algorithmic FLOPs of one training step per GPU: frozen weights => dX only."""
    T = N * S
    tot = 0.0
    for t in tasks:
        lin = 2 * T * (4 * D * D + 3 * D * Hf)
        fwd = L * (lin + 4 * N * S * (A + S) * D + 4 * A * D * D)
        bwd = L * (lin + 10 * N * S * (A + S) * D + 4 * A * D * D)
        head = 2 * T * D * V if t != "qav" else 2 * N * (S - 1) * D * F
        tot += fwd + bwd + head * (2 if t != "qav" else 3)
    tot += 2 * 2 * N * F * 768 * D
    return tot


def step_roofline_of(fl, ms, peak, model, batches, B, S, tasks):
    """The whole step against the dense MFMA peak. `frac` prices the step at the ALGORITHMIC FLOPs of SURVEY 8d — the reference's
    step: every projection of every layer and the LM head at every position (llama/model.py:338-350) — as the contract defines
    "MFMA % of peak" (its 40 % == 292 samples/s at C2). Since round 5 the step runs the last layer's post-attention half (WO, FFN,
    final norm), the heads and all of their backward on the rows a head reads only (identical losses and gradients;
    FVQA_LM_HEAD=all restores the dense form): `executed_flops_per_step` / `frac_executed` count what the kernels actually
    multiplied, so that the skipped rows are not read as matrix-core work."""
    from fvqa import scored
    out = {"bound": "mfma", "achieved": fl / (ms * 1e-3) / 1e12, "peak": peak / 1e12, "unit": "TFLOP/s",
           "frac": fl / (ms * 1e-3) / peak, "flops_per_step": fl, "lm_head_rows": "all"}
    have = [b for b in batches if all(t in b.get(scored.COUNT, {}) for t in tasks)]
    if model.ensure_engine().lm_head_rows == "scored" and len(have) == len(batches):
        D, V = model.params.dim, model.vocab_size
        Hf = model.layers[0].feed_forward.w1.weight.shape[0]
        lm = [t for t in tasks if t in scored.LM_TASKS]
        m_lm = sum(sum(scored.rows_of(int(b[scored.COUNT][t])) for t in lm) for b in have) / len(have)
        m_all = sum(sum(scored.rows_of(int(b[scored.COUNT][t])) for t in tasks) for b in have) / len(have)
        dense_lm, dense_all = len(lm) * B * S, len(tasks) * B * S
        per_row_tail = 2.0 * (2.0 * D * D + 6.0 * D * Hf)     # WO + W1|W3 + W2 of one row, forward; the same again for their dX
        ex = fl - (dense_lm - m_lm) * 2.0 * D * V * 2 - (dense_all - m_all) * per_row_tail * 2
        out.update({"lm_head_rows": "scored", "lm_head_rows_per_step": m_lm, "lm_head_rows_dense": dense_lm,
                    "tail_rows_per_step": m_all, "tail_rows_dense": dense_all,
                    "executed_flops_per_step": ex, "frac_executed": ex / (ms * 1e-3) / peak,
                    "note": "frac = SURVEY 8d algorithmic FLOPs (the reference's dense step) / time / peak; frac_executed = the "
                            "FLOPs the kernels ran (last layer's post-attention half and the heads on the rows a head reads only) "
                            "/ time / peak"})
    return out


def launch_alg_bytes(kind, flops, R, D, Hf, V):
    """Algorithmic bytes of one projection launch of the step, identified by its epilogue kind and FLOP count: operands
    read once + outputs written once (bf16; fp32 logits), epilogue operands included (residual rows; the saved SwiGLU
    factors read by the W2^T launch; z next to (s, t) written by the W1|W3 launch). None for a shape it does not know."""
    shapes = {  # (epilogue, out is fp32) -> [(N, K)]
        (7, False): [(3 * D, D)], (0, False): [(D, D), (D, 3 * D), (D, 2 * Hf), (D, V)], (1, False): [(D, D), (D, Hf)],
        (5, False): [(2 * Hf, D)], (4, False): [(2 * Hf, D)], (6, False): [(Hf, D)], (3, False): [(Hf, D)],
        (0, True): [(V, D)]}
    epi, f32 = kind & 15, bool(kind & 32)
    R_all = R
    for (N, K) in shapes.get((epi, f32), []):
        # launches of the tail rows (the last layer's post-attention half, the LM head, their dX; fvqa/step.py TailRows) carry their
        # own row count: a launch of this shape whose FLOPs are a whole number of rows <= the dense count
        R = R_all
        r = flops / (2.0 * N * K)
        if abs(r - round(r)) < 1e-6 * max(r, 1.0) and 0 < round(r) < R_all:
            R = int(round(r))
        if abs(2.0 * R * N * K - flops) < 1e-6 * flops:
            b = 2.0 * R * K + 2.0 * N * K + (4.0 if f32 else 2.0) * R * N
            if epi == 1:
                b += 2.0 * R * N                        # residual rows
            if epi in (4, 5):
                b += 2.0 * R * N / 2                    # z
            if epi in (3, 6):
                b += 2.0 * R * 2 * N + 2.0 * R * N      # reads (s, t) rows of 2N, writes d(a|b) rows of 2N instead of N
            return b
    return None


DUMP_BUDGET = 60 * 10**6     # array bytes --dump-outputs may write; with the .npy headers the files stay under 64 MB
OUTPUTS = ("losses", "grad_norm", "trainables", "grads")


def step_outputs(outs, opt):
    """What one training step hands its caller, as host float32 arrays: the (vqa, vaq, qav) losses, the gradient norm the loss
    scaler returns, the flat trainables after AdamW and their (unscaled) flat gradient."""
    import numpy as np
    vqa, vaq, qav, norm = outs
    f32 = lambda t: t.detach().float().reshape(-1).cpu().numpy()
    return {"losses": np.concatenate([f32(vqa), f32(vaq), f32(qav)]), "grad_norm": f32(norm),
            "trainables": f32(opt.flat.flat), "grads": f32(opt.flat.flat_grad)}


def write_outputs(out_dir, arrays, budget=DUMP_BUDGET, seed=0):
    """Writes {name: array} as out_dir/<name>.npy (float32 / float64 kept, anything else as float32). If they hold more than
    `budget` bytes, every array is cut to the same fraction of its elements by a sample fixed by `seed` and its size (the same
    indices on every run), flattened. Returns {name: elements written}."""
    import numpy as np
    arrays = {n: (a if a.dtype in (np.float32, np.float64) else a.astype(np.float32)) for n, a in arrays.items()}
    total = sum(a.nbytes for a in arrays.values())
    keep = min(1.0, budget / total) if total else 1.0
    os.makedirs(out_dir, exist_ok=True)
    written = {}
    for n, a in arrays.items():
        if keep < 1.0:
            k = max(1, int(a.size * keep))
            idx = np.sort(np.random.default_rng(seed).choice(a.size, size=k, replace=False))
            a = a.reshape(-1)[idx]
        np.save(os.path.join(out_dir, n + ".npy"), a)
        written[n] = int(a.size)
    return written


def _cpu_extrapolated(seq_len, max_feats):
    """Fallback: oracle fwd+bwd at 7B width for 1 and 2 layers, B=2, VQA only; per-layer and fixed cost separated and
    scaled to 32 layers."""
    from fvqa import synth
    from oracle import ref_cpu
    times = {}
    for L in (1, 2):
        cfg = synth.preset("7b_l2", n_layers=L, adapter_layer=L, max_seq_len=seq_len, max_feats=max_feats,
                           batch_size=2)
        model = ref_cpu.RefModel(cfg, synth.state_dict(cfg), dtype=torch.float32)
        batch = synth.make_batch(cfg, seed=0)
        model.step(batch)                      # warm-up
        best = float("inf")
        for _ in range(3):                     # min of 3: host timings on a shared box are noisy
            t0 = time.perf_counter()
            model.step(batch)
            best = min(best, time.perf_counter() - t0)
        times[L] = best
        del model
    per_layer = times[2] - times[1]
    if not (0.15 * times[2] < per_layer < times[1]):
        per_layer = times[2] / 3.0
    fixed = max(times[1] - per_layer, 0.0)
    full = fixed + 32 * per_layer              # one 7B step on B=2 samples
    return {"value": 2.0 / full, "unit": "samples/s", "cores": torch.get_num_threads(), "kind": "port",
            "method": "extrapolated",
            "sample": f"oracle/ref_cpu.py fp32, 7B width, B=2 S={seq_len} VQA-only, timed at 1 and 2 layers "
                      f"({times[1]:.2f}s, {times[2]:.2f}s) and scaled to 32 layers + head ({full:.1f}s/step)"}


def cpu_baseline_leg(seq_len, max_feats, budget_s=240.0, max_timed=3):
    """The CPU oracle (oracle/ref_cpu.py, fp32) timed on this host's cores on SURVEY §8d's sample: BASELINE configs[0] (C1)
    — the full 32-layer 7B, B = 2 samples of the same sequence length, ALL THREE flipped losses (--vaq --qav) — forward +
    backward + AdamW(0.9, 0.95) on the 4.5 M trainables, one warm-up step (first touch of 27 GB of weights) and up to three
    timed ones within `budget_s` of host time (a slow host stops earlier; how many were timed is stated). The closed-form
    fp32 weights are generated on the GPU tensor by tensor and copied over (same counter hash on either device). `value`
    is samples/s of that workload (3 streams per sample); `per_stream_value` restates it per (sample, stream) pair, the
    unit in which it compares with the VQA-only GPU line. Falls back to the 1- / 2-layer extrapolation if the full-depth
    model cannot be built (host memory)."""
    from fvqa import synth
    from oracle import ref_cpu
    try:
        cfg = synth.preset("7b", max_seq_len=seq_len, max_feats=max_feats, batch_size=2, vaq=True, qav=True)
        dev = "cuda" if torch.cuda.is_available() else "cpu"
        sd = {n: synth.make_tensor(cfg, n, shape, kind, device=dev).cpu() for n, shape, kind in synth.state_spec(cfg)}
        model = ref_cpu.RefModel(cfg, sd, dtype=torch.float32)
        del sd
        batch = synth.make_batch(cfg, seed=0)
        names = [n for n in model.sd if synth.is_trainable(n)]
        params = [torch.nn.Parameter(model.sd[n]) for n in names]       # AdamW updates the oracle's tensors in place
        for n, p_ in zip(names, params):
            model.sd[n] = p_.data
        opt = torch.optim.AdamW(params, lr=9e-2 * 2 / 256, betas=(0.9, 0.95), weight_decay=0.14)

        def one_step():
            out = model.step(batch)
            for n, p_ in zip(names, params):
                p_.grad = out["grads"][n]
            opt.step()

        t_start = time.perf_counter()
        times = []
        for i in range(1 + max_timed):             # warm-up + up to max_timed timed steps
            t0 = time.perf_counter()
            one_step()
            times.append(time.perf_counter() - t0)
            if i >= 1 and (time.perf_counter() - t_start) + times[-1] > budget_s:
                break
            if i == 0 and times[0] > 0.6 * budget_s:
                break                              # a very slow host (> 144 s per step): the warm-up step is the measurement
        timed = times[1:] if len(times) > 1 else times
        dt = min(timed)
        del model
        return {"value": 2.0 / dt, "unit": "samples/s", "per_stream_value": 6.0 / dt, "cores": torch.get_num_threads(),
                "cpus": os.cpu_count(), "kind": "port", "method": "measured_full_depth",
                "sample": f"oracle/ref_cpu.py fp32, BASELINE configs[0]: full LLaMA-7B (32 layers), B=2 samples, S={seq_len}, "
                          f"losses vqa+vaq+qav, forward+backward+AdamW steps: warm-up {times[0]:.1f}s, timed "
                          f"{', '.join(f'{t:.1f}s' for t in times[1:]) or 'none (warm-up used)'}; value = 2 samples / "
                          f"{dt:.1f}s (fastest timed step), {torch.get_num_threads()} torch threads on {os.cpu_count()} CPUs"}
    except (RuntimeError, MemoryError) as e:
        out = _cpu_extrapolated(seq_len, max_feats)
        out["fallback_reason"] = repr(e)[:200]
        return out


def launcher_command(n_gpus, argv, port=None, python=None):
    """argv of the child that runs `bench.py <argv>` as n_gpus ranks of ONE node (one process per GPU,
    RCCL over xGMI): the form the driver itself uses for N>1."""
    if port is None:
        import socket
        with socket.socket() as s:               # a free port on the loopback interface
            s.bind(("127.0.0.1", 0))
            port = s.getsockname()[1]
    return [python or sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n_gpus}",
            "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__), *argv]


def launcher_env(n_gpus, n_devices, env=None):
    """Environment of the child ranks. With fewer devices than ranks (a rehearsal of the N>1 control flow on a
    smaller box) the ranks share devices and use gloo; the JSON line then carries "rehearsal": true."""
    env = dict(os.environ if env is None else env)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", "8")
    if 0 < n_devices < n_gpus:
        env.setdefault("FVQA_DIST_BACKEND", "gloo")
        env["FVQA_BENCH_REHEARSAL"] = "1"
    return env


def self_launch(n_gpus, argv):
    """Start the ranks as a CHILD process group (never an exec of this process), relay rank 0's JSON line, and take the
    whole group down with us: a killed parent (driver time limit, ^C) must not leave torchrun and its ranks on the GPUs."""
    import signal
    import subprocess
    n_dev = torch.cuda.device_count()            # (this parent launches no kernel and creates no context of its own)
    cmd = launcher_command(n_gpus, argv)
    print(f"[bench] starting {n_gpus} ranks: {' '.join(cmd)}", file=sys.stderr, flush=True)
    child = subprocess.Popen(cmd, env=launcher_env(n_gpus, n_dev), stdout=subprocess.PIPE, text=True,
                             start_new_session=True)

    def reap(grace=10.0):
        if child.poll() is not None:
            return
        for sig in (signal.SIGTERM, signal.SIGKILL):
            try:
                os.killpg(child.pid, sig)        # the child's own session: exactly the processes started here
            except ProcessLookupError:
                return
            try:
                child.wait(timeout=grace)
                return
            except subprocess.TimeoutExpired:
                continue

    def on_signal(signum, frame):
        reap()
        raise SystemExit(128 + signum)

    old = {sg: signal.signal(sg, on_signal) for sg in (signal.SIGTERM, signal.SIGINT)}
    try:
        for line in child.stdout:                # stdout carries the ONE JSON line of rank 0; stderr passes through
            sys.stdout.write(line)
            sys.stdout.flush()
        return child.wait()
    finally:
        reap()
        for sg, h in old.items():
            signal.signal(sg, h)


OTHER_CONFIGS = {   # BASELINE configs[2..4] as ONE GPU runs them (reference README.md:62-96 recipes)
    "c3": dict(model="7B", batch_size=8, seq_len=128, vaq=True, qav=True),
    "c4": dict(model="7B", batch_size=1, seq_len=650, vaq=True, qav=True),
    "c5": dict(model="13B", batch_size=4, seq_len=128, vaq=True, qav=True),
    # the headline workload in the reference's DENSE form (every projection of the last layer and the LM head at every position:
    # FVQA_LM_HEAD=all), on the same GPU in the same command — what the tail rows are worth, and the figure to read if one
    # counts the reference's dead rows as work that must be done
    "c2_dense": dict(model="7B", batch_size=8, seq_len=128, vaq=False, qav=False, lm_head="all"),
}


def short_leg(dev, model_name, batch_size, seq_len, vaq, qav, dtype="bf16", steps=10, warmup=3, lm_head=None):
    """One more BASELINE shape on the same GPU: builds its model, runs `warmup` + `steps` full training steps (forward, the
    flipped losses, backward, unscale + norm, AdamW) on cycling resident batches, returns its line fragment. Frees everything
    it built."""
    import contextlib
    import gc
    import util.misc as misc
    from fvqa import synth
    from fvqa.step import stage_batch
    from fvqa.optim import FusedAdamW, param_groups_weight_decay
    from llama_vqa import LLaMA_VQA
    args = types.SimpleNamespace(
        llama_model_path="/nonexistent/", model=model_name, max_seq_len=seq_len, adapter_len=10,
        adapter_layer=40 if model_name == "13B" else 32, max_feats=10, bias=3.5, tau=100.0, vaq=vaq, qav=qav,
        audio=False, audio_only=False, audio_merge="none", debug=False, synthetic=True, random_init=True,
        dtype=dtype, accum_iter=1, weight_decay=0.14)
    with contextlib.redirect_stdout(sys.stderr):
        model = LLaMA_VQA(args)
    model.to(dev)
    p = model.params
    opt = FusedAdamW(param_groups_weight_decay(model, args.weight_decay), lr=9e-2 * batch_size / 256, betas=(0.9, 0.95),
                     flat=model.flat_params())
    scaler = misc.NativeScalerWithGradNormCount()
    if lm_head is not None:
        model.ensure_engine().lm_head_rows = lm_head
    cfg = synth.SynthConfig(dim=p.dim, n_heads=p.n_heads, n_layers=p.n_layers, vocab_size=model.vocab_size,
                            max_seq_len=seq_len, batch_size=batch_size, vaq=vaq, qav=qav)
    batches = []
    for i in range(4):
        # resident batch; the scored-row lists of the LM head are taken while the labels are on the host (fvqa/step.py)
        batches.append(stage_batch(synth.make_batch(cfg, seed=1234 + i), dev))

    def one_step(i):
        opt.zero_grad()
        vqa_l, vaq_l, qav_l = model(batches[i % 4])
        loss = vqa_l + vaq_l + qav_l
        scaler(loss, opt, parameters=None, update_grad=True)
        return loss

    for i in range(warmup):
        one_step(i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        loss = one_step(i)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    err = None
    try:
        model.ensure_engine().check_gemm_error()
    except RuntimeError as e:
        err = str(e)
    tasks = ["vqa"] + (["vaq"] if vaq else []) + (["qav"] if qav else [])
    L = len(model.engine_layer_ids())
    Hf = model.layers[0].feed_forward.w1.weight.shape[0]
    fl = step_flops(p.dim, p.n_heads, L, Hf, model.vocab_size, batch_size, seq_len, 10, 10, tasks)
    ms = dt / steps * 1e3
    out = {"workload": f"LLaMA-{model_name} {dtype} seq_len={seq_len} batch={batch_size}/GPU max_feats=10 "
                       f"losses={'+'.join(tasks)} fwd+bwd+AdamW, {L} layers",
           "steps": steps, "warmup": warmup, "ms_per_step": ms, "samples_per_s": batch_size * steps / dt,
           "loss": float(loss.detach().sum()),
           "step_roofline": step_roofline_of(fl, ms, MFMA_BF16_PEAK, model, batches, batch_size, seq_len, tasks)}
    if err is not None:
        out["invalid"] = err
    del model, opt, scaler, batches
    gc.collect()
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--model", default="7B")
    ap.add_argument("--batch_size", type=int, default=8)
    ap.add_argument("--seq_len", type=int, default=128)
    ap.add_argument("--vaq", action="store_true")
    ap.add_argument("--qav", action="store_true")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp16", "fp32"],
                    help="storage type of activations / frozen weights: bf16 (BASELINE configs), fp16 (the reference's own), fp32 (exact)")
    ap.add_argument("--n_layers", type=int, default=0, help="debug only: reduced depth (marks the line invalid)")
    ap.add_argument("--full", action="store_true",
                    help="also measure what takes runs or legs of its own: the instrumented roofline passes, the other BASELINE "
                         "configs and the CPU baseline (a plain run times the steps and prints the headline line only)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the outputs of the last timed step as DIR/<name>.npy (float32, at most 64 MB in all)")
    ap.add_argument("--no_cpu_baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no_other_configs", action="store_true",
                    help="with --full: skip the short C3 / C4 / C5 legs that follow the default (C2) workload at N = 1")
    a = ap.parse_args()
    if a.steps < 1 or a.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")

    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # plain `python bench.py --gpus N`: this parent has made no GPU call; it starts the N ranks as a CHILD
        # process (never an exec), relays their output and exits with the child's code
        raise SystemExit(self_launch(a.gpus, sys.argv[1:]))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if a.gpus > 1 and world != a.gpus:
        raise SystemExit(f"--gpus {a.gpus} but WORLD_SIZE={world}: launch with --nproc-per-node {a.gpus}")
    local = local % max(1, torch.cuda.device_count())       # (rehearsals put several ranks on one GPU)
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    diag = None
    if world > 1:
        # RCCL over xGMI; FVQA_DIST_BACKEND=gloo only for single-GPU rehearsals of the N>1 control flow
        dist.init_process_group(os.environ.get("FVQA_DIST_BACKEND", "nccl"), init_method="env://",
                                world_size=world, rank=rank)
        # start-up self-diagnosis: RCCL world == --gpus, one rank per whole MI355X (256 CUs, no compute partition), host
        # threads pinned per rank; raises on every rank with the list of problems (fvqa/rankcheck.py)
        sys.path.insert(0, os.path.join(ROOT, "flipped-vqa_amd"))
        from fvqa import rankcheck
        host_threads = rankcheck.pin_host_threads(world)
        diag = rankcheck.check_ranks(a.gpus, rank, int(os.environ.get("LOCAL_RANK", "0")), local,
                                     rehearsal=os.environ.get("FVQA_BENCH_REHEARSAL") == "1")
        diag["host_threads_per_rank"] = host_threads

    import util.misc as misc
    from fvqa import ops, synth
    from fvqa.step import stage_batch
    from fvqa.optim import FusedAdamW, param_groups_weight_decay
    from fvqa.parallel import DataParallel
    from llama_vqa import LLaMA_VQA

    args = types.SimpleNamespace(
        llama_model_path="/nonexistent/", model=a.model, max_seq_len=a.seq_len, adapter_len=10,
        adapter_layer=40 if a.model == "13B" else 32, max_feats=10, bias=3.5, tau=100.0, vaq=a.vaq, qav=a.qav,
        audio=False, audio_only=False, audio_merge="none", debug=False, synthetic=True, random_init=True,
        dtype=a.dtype, accum_iter=1, weight_decay=0.14)
    kw = {}
    if a.n_layers:
        kw["n_layers"] = a.n_layers
        args.adapter_layer = a.n_layers
    t_build = time.time()
    import contextlib
    with contextlib.redirect_stdout(sys.stderr):       # the factory prints the reference's banner; stdout carries ONE JSON line
        model = LLaMA_VQA(args, **kw)
    model.to(dev)
    p = model.params
    eff = a.batch_size * world
    lr = 9e-2 * eff / 256
    opt = FusedAdamW(param_groups_weight_decay(model, args.weight_decay), lr=lr, betas=(0.9, 0.95),
                     flat=model.flat_params())
    net = model
    if world > 1:
        net = DataParallel(model)
        opt.grad_sync = net.sync_grads
    scaler = misc.NativeScalerWithGradNormCount()

    cfg = synth.SynthConfig(dim=p.dim, n_heads=p.n_heads, n_layers=p.n_layers, vocab_size=model.vocab_size,
                            max_seq_len=a.seq_len, batch_size=a.batch_size, vaq=a.vaq, qav=a.qav)
    n_batches = 4
    batches = []
    for i in range(n_batches):
        # resident batch; the scored-row lists of the LM head are taken while the labels are on the host (fvqa/step.py)
        batches.append(stage_batch(synth.make_batch(cfg, seed=1234 + rank + world * i), dev))
    torch.cuda.synchronize()
    if rank == 0:
        print(f"[bench] model built in {time.time() - t_build:.1f}s; "
              f"{torch.cuda.memory_allocated() / 2**30:.1f} GiB allocated", file=sys.stderr, flush=True)

    rehearsal_lock = None
    if world > 1 and os.environ.get("FVQA_BENCH_REHEARSAL") == "1":
        # Rehearsal (several ranks on ONE GPU, control flow only): the persistent GEMM needs the device to itself
        # (include/fvqa.h: one workgroup per CU, partners wait for each other), so two ranks' forward / backward must not
        # share the chip — they take turns under a file lock, released before the gradient all-reduce (where every rank
        # has to be present). On real multi-GPU runs every rank owns its device and none of this exists.
        import fcntl
        import tempfile
        rehearsal_lock = open(os.path.join(tempfile.gettempdir(),
                                           f"fvqa_bench_{os.environ.get('MASTER_PORT', '0')}.lock"), "w")
        sync_grads = net.sync_grads

        def _turn_over():
            torch.cuda.synchronize()
            fcntl.flock(rehearsal_lock, fcntl.LOCK_UN)
            return sync_grads()

        opt.grad_sync = _turn_over

    def one_step(i):
        if rehearsal_lock is not None:
            import fcntl
            fcntl.flock(rehearsal_lock, fcntl.LOCK_EX)
        opt.zero_grad()
        vqa, vaq, qav = net(batches[i % n_batches])
        loss = vqa + vaq + qav
        norm = scaler(loss, opt, parameters=None, update_grad=True)
        return loss, (vqa, vaq, qav, norm)

    def fence():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
            torch.cuda.synchronize()

    for i in range(a.warmup):
        one_step(i)
    fence()
    if os.environ.get("FVQA_BENCH_INJECT_GEMM_ERROR") == "1":
        # test hook (tests/test_bench_gpu.py): what a timed-out split-K exchange leaves behind — the line must come out
        # invalid and the process must fail
        w_ = ops.gemm_error_word(dev)
        if w_ is not None:
            w_.view(torch.int64)[0] = 1
    if world > 1:
        net.comm_events = []                 # an event pair around every gradient all-reduce of the timed steps
    t0 = time.perf_counter()
    for i in range(a.steps):
        loss, outs = one_step(i)
    fence()
    dt = time.perf_counter() - t0
    if a.dump_outputs and rank == 0:         # the last timed step's results, before --full's passes step the model further
        written = write_outputs(a.dump_outputs, step_outputs(outs, opt))
        print(f"[bench] outputs of timed step {a.steps} -> {a.dump_outputs}: {written}", file=sys.stderr, flush=True)
    comm = None
    if world > 1:
        ev, net.comm_events = net.comm_events, None
        comm_ms = [e0.elapsed_time(e1) for e0, e1 in ev]
        t = torch.tensor([dt, sum(comm_ms) / max(1, len(comm_ms))], dtype=torch.float64, device=dev)
        per_rank = [torch.zeros_like(t) for _ in range(world)]
        dist.all_gather(per_rank, t)                      # every rank's own clock and all-reduce time: who is the slow one
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t[0].item())
        rank_ms = [float(x[0].item()) / a.steps * 1e3 for x in per_rank]
        comm = {"allreduce_ms": float(t[1].item()), "allreduce_calls_per_step": len(comm_ms) / a.steps,
                "ms_per_step_per_rank": {"min": min(rank_ms), "max": max(rank_ms), "all": rank_ms},
                # each rank's own rate = what an N = 1 run of the same per-GPU work reads as `value` (compare with BENCH directly)
                "samples_per_s_per_rank": {"min": a.batch_size / max(rank_ms) * 1e3, "max": a.batch_size / min(rank_ms) * 1e3,
                                           "all": [a.batch_size / m * 1e3 for m in rank_ms]},
                "allreduce_ms_per_rank": [float(x[1].item()) for x in per_rank],
                "allreduce_bytes": int(model.flat_params().flat_grad.numel() * 4),
                "rccl_ranks": dist.get_world_size(), "backend": dist.get_backend(),
                "note": "max over ranks of the mean device time between the events bracketing all_reduce(SUM) of the "
                        "flat fp32 gradient buffer; it includes waiting for the slowest rank"}
    loss_val = float(loss.detach().sum())
    ms = dt / a.steps * 1e3
    value = a.batch_size * world * a.steps / dt
    gemm_error = None
    try:                                     # a timed-out split-K exchange anywhere above invalidates the line
        model.ensure_engine().check_gemm_error()
    except RuntimeError as e:
        gemm_error = str(e)

    # ---- instrumented repeats of the same steps under the same native schedule: HIP events recorded by the library on
    # the launch stream around launches of the dominant kernel. SPARSE pass: every 17th launch is bracketed (17 is
    # co-prime with the 258 launches of a step, so every launch position is sampled over the steps), which leaves the
    # duty cycle — and on this power-limited chip the clock — of the timed region in place: its per-launch times are the
    # ones `roofline` quotes. DENSE pass (every launch bracketed, as rounds 1-2 did): kept for comparison only.
    STRIDE = 17

    def instrumented(stride):
        if rank == 0:
            ops.gemm_timing_enable(True, stride)
        fence()
        t0 = time.perf_counter()
        for i in range(a.steps):             # every rank runs it: the step contains the gradient all-reduce
            one_step(i)
        fence()
        ms_pass = (time.perf_counter() - t0) / a.steps * 1e3
        rec = []
        if rank == 0:
            rec = ops.gemm_timing_read()
            ops.gemm_timing_enable(False)
        return ms_pass, rec

    roof = None
    ms_sparse, rec_sparse, ms_dense, rec_dense = None, [], None, []
    if a.full:
        ms_sparse, rec_sparse = instrumented(STRIDE)
        ms_dense, rec_dense = instrumented(1)
    if rank == 0 and rec_sparse:
        # calibration: what an event pair with NOTHING between reads on this stream (the record-to-record spacing that
        # every bracketed launch also contains); taken off per launch so that the figure is the kernel's own duration — checked
        # against rocprofv3's durations of the same run in round 5 (profiles/r05_rocprof_frac.json: equal to 0.1 %)
        evs = [torch.cuda.Event(enable_timing=True) for _ in range(129)]
        for ev in evs:
            ev.record()
        torch.cuda.synchronize()
        gaps = sorted(evs[i].elapsed_time(evs[i + 1]) * 1e3 for i in range(128))
        probe_overhead_us = gaps[len(gaps) // 2]
        epi_name = {0: "none", 1: "residual", 3: "swiglu_bwd", 4: "swiglu_fwd", 5: "swiglu_fwd_st", 6: "swiglu_bwd_st", 7: "rope"}

        def name_of(kind):
            return ("f32" if kind & 64 else "bf16") + "_" + ("f32" if kind & 32 else "bf16") + "_" + \
                epi_name.get(kind & 15, str(kind & 15)) + ("_splitk" if kind & 16 else "") + ("_4w" if kind & 128 else "") + \
                ("_fewrows" if kind & 256 else "")

        R_ = a.batch_size * a.seq_len * (1 + int(a.vaq) + int(a.qav))
        Hf_ = model.layers[0].feed_forward.w1.weight.shape[0]

        raw_ms_acc = [0.0]            # GEMM ms per step from the brackets AS MEASURED (no empty pair taken off), last summarise()

        def summarise(rec):
            """per (kind, FLOPs) = per shape of an instantiation: launches per step, mean duration of the bracketed ones"""
            sh = {}
            for (us, fl, kind) in rec:
                e = sh.setdefault((kind, fl), [0, 0, 0.0])
                e[0] += 1
                if us >= 0:
                    e[1] += 1
                    e[2] += us                      # the bracket as measured; the empty event pair is taken off per shape below
            per, tot_ms, tot_f, n_launch, n_timed, missing = {}, 0.0, 0.0, 0, 0, 0
            raw_ms_acc[0] = 0.0
            for (kind, fl), (cnt, nt, sum_us) in sh.items():
                if nt == 0:
                    missing += cnt
                    continue
                mean_raw = sum_us / nt
                mean_us = max(mean_raw - probe_overhead_us, 0.0)      # = the kernel's own duration (same-run rocprofv3 check)
                raw_ms_acc[0] += cnt / a.steps * mean_raw * 1e-3
                per_step = cnt / a.steps
                tot_ms += per_step * mean_us * 1e-3
                tot_f += per_step * fl
                n_launch += cnt
                n_timed += nt
                p_ = per.setdefault(name_of(kind), [0.0, 0.0, 0.0, 0.0, 0.0])
                p_[0] += per_step
                p_[1] += per_step * mean_us
                p_[2] += per_step * fl
                ab = launch_alg_bytes(kind, fl, R_, p.dim, Hf_, model.vocab_size)
                if ab is not None:
                    p_[3] += per_step * ab
                    p_[4] += per_step
            return per, tot_ms, tot_f, n_launch, n_timed, missing

        per_d, gemm_ms_dense, flops_dense, n_dense, n_timed_d, _ = summarise(rec_dense)
        gemm_ms_raw_dense = raw_ms_acc[0]
        per, gemm_ms, flops_step, n_launch, n_timed, missing = summarise(rec_sparse)
        gemm_ms_raw = raw_ms_acc[0]
        stride_used, ms_pass = STRIDE, ms_sparse
        if missing or gemm_ms <= 0:              # too few steps for the stride to reach every shape: use the dense pass
            per, gemm_ms, flops_step, n_launch, n_timed = per_d, gemm_ms_dense, flops_dense, n_dense, n_timed_d
            stride_used, ms_pass, gemm_ms_raw = 1, ms_dense, gemm_ms_raw_dense
        if gemm_ms > 0:
            peak = MFMA_BF16_PEAK if a.dtype in ("bf16", "fp16") else 157.3e12      # (f16 MFMA = bf16 MFMA rate)
            events_ms = n_timed / a.steps * probe_overhead_us * 1e-3
            non_gemm_ms = ms_pass - gemm_ms - events_ms        # everything of a step that is not this kernel (incl. kernel boundaries)
            achieved = flops_step / (gemm_ms * 1e-3)
            # fabric-side bytes per launch from the rocprofv3 --pmc passes of THIS command (tools/pmc_summary.py:
            # FETCH_SIZE x2 gfx950 correction + WRITE_SIZE), valid only for the kernel sources they were collected with
            traffic, tsrc = None, None
            tj = next((f for f in (os.path.join(ROOT, "profiles", n) for n in ("r05_pmc_mfma_lds.json", "r04_pmc_mfma_lds.json", "r03_pmc_mfma_lds.json"))
                       if os.path.exists(f)), None)
            if a.dtype == "bf16" and a.model == "7B" and not (a.vaq or a.qav) and a.seq_len == 128 and tj:
                pm = json.load(open(tj))
                from fvqa import build as fbuild
                if pm.get("source_hash") == fbuild.source_hash():
                    w_ = [(v["launches_sampled"], v["hbm_bytes_per_launch"]) for k, v in pm.get("kernels", {}).items()
                          if (k.startswith("gemm_sk_256") or "gemm4w_k" in k or "gemm4w_sk_k" in k or "fewrows_partial_k" in k)
                          and "hbm_bytes_per_launch" in v]
                    if w_:
                        traffic = sum(c * b for c, b in w_) / sum(c for c, _ in w_)
                        tsrc = f"profiles/{os.path.basename(tj)} (kernel sources {pm['source_hash'][:12]}, same workload)"
            roof = {"bound": "mfma",
                    "kernel": "projection GEMMs of the step, every launch of every instantiation, all on the one-wave-per-SIMD main loop: gemm4w_k (whole tiles, tile width per problem: *_4w) and gemm4w_sk_k (256x256 tiles cut 2 or 4 ways along K, reduced inside the launch: *_splitk_4w)",
                    "achieved": achieved / 1e12, "peak": peak / 1e12, "unit": "TFLOP/s",
                    "frac": achieved / peak, "traffic": traffic, "traffic_source": tsrc,
                    "method": f"HIP events around every {stride_used}th launch in a repeat of the timed steps "
                              f"({n_timed} of {n_launch} launches bracketed, every launch position sampled); "
                              "per shape: mean bracketed duration x launches per step",
                    "launches_per_step": n_launch / a.steps, "gemm_ms_per_step": gemm_ms,
                    "avg_launch_us": gemm_ms * 1e3 / (n_launch / a.steps),
                    "avg_flops_per_launch": flops_step / (n_launch / a.steps),
                    "ms_per_step_this_pass": ms_pass, "ms_per_step_timed_region": ms,
                    "non_gemm_ms_per_step": non_gemm_ms, "event_pairs_ms_per_step": events_ms,
                    "probe_overhead_us_subtracted": probe_overhead_us,
                    # the same figure with the brackets as measured (lower bound: every bracket also holds the event pair's own
                    # ~4.8 us and the kernel boundary); `frac` is the one that agrees with rocprofv3's kernel durations of the
                    # SAME run to ~0.1 % (tools/rocprof_frac.py, profiles/r05_rocprof_frac.json)
                    "frac_brackets_as_measured": flops_step / (gemm_ms_raw * 1e-3) / peak if gemm_ms_raw > 0 else None,
                    "dense_probe": {"frac": (flops_dense / (gemm_ms_dense * 1e-3) / peak) if gemm_ms_dense > 0 else None,
                                    "gemm_ms_per_step": gemm_ms_dense, "ms_per_step_this_pass": ms_dense,
                                    "note": "every launch bracketed (rounds 1-2 method): lighter duty cycle, reads high"},
                    "alg_bytes_per_launch": (sum(v[3] for v in per.values()) / max(1e-9, sum(v[4] for v in per.values()))
                                             if any(v[4] for v in per.values()) else None),
                    "per_instantiation": {k: {"launches_per_step": v[0], "avg_launch_us": v[1] / v[0],
                                              "TFLOP/s": v[2] / v[1] / 1e6,
                                              "alg_bytes_per_launch": (v[3] / v[4]) if v[4] else None,
                                              "alg_GB/s": (v[3] / v[4]) / (v[1] / v[0]) / 1e3 if v[4] else None}
                                          for k, v in per.items()}}
            # the probe must account for the step it ran in: GEMM + a plausible rest
            if not (0.0 < non_gemm_ms < 0.5 * ms_pass):
                roof["inconsistent"] = "probe GEMM time + event pairs does not fit the pass's own step time"

    if rank == 0:
        tasks = ["vqa"] + (["vaq"] if a.vaq else []) + (["qav"] if a.qav else [])
        L = len(model.engine_layer_ids())
        Hf = model.layers[0].feed_forward.w1.weight.shape[0]
        fl = step_flops(p.dim, p.n_heads, L, Hf, model.vocab_size, a.batch_size, a.seq_len, 10, 10, tasks)
        peak = MFMA_BF16_PEAK if a.dtype in ("bf16", "fp16") else 157.3e12      # (f16 MFMA = bf16 MFMA rate)
        out = {
            # BASELINE.json's metric string verbatim for its workload; `value` is the samples/s part, the
            # "MFMA % of peak" part is step_roofline.frac (whole step) and roofline.frac (dominant kernel)
            "metric": ("train samples/sec LLaMA-7B seq128 max_feats=10 at 1/2/4/8 GPUs; MFMA % of peak"
                       if a.model == "7B" and a.seq_len == 128 else
                       f"train samples/sec LLaMA-{a.model} seq{a.seq_len} max_feats=10"),
            "value": value, "unit": "samples/s", "n_gpus": world, "steps": a.steps, "warmup": a.warmup,
            "ms_per_step": ms, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": a.dtype, "data": "synthetic (closed-form random-init weights, synthetic NExT-QA-shaped batches resident in HBM)",
            "config": {"workload": f"LLaMA-{a.model} {a.dtype} seq_len={a.seq_len} batch={a.batch_size}/GPU max_feats=10 "
                                   f"losses={'+'.join(tasks)} fwd+bwd+AdamW, {L} layers",
                       "global_batch": a.batch_size * world, "seq_len": a.seq_len,
                       "parallelism": f"dp{world}" if world > 1 else "single"},
            "loss": loss_val,
        }
        if a.full:
            out["roofline"] = roof
        out["step_roofline"] = step_roofline_of(fl, ms, peak, model, batches, a.batch_size, a.seq_len, tasks)
        if comm is not None:
            out["comm"] = comm
        if diag is not None:
            out["ranks"] = {"host_threads_per_rank": diag["host_threads_per_rank"], "problems": diag["problems"],
                            "devices": [{k: r.get(k) for k in ("rank", "host", "device_id", "cu_count", "gcn_arch", "hbm_gib")}
                                        for r in diag["reports"]]}
        if a.n_layers:
            out["invalid"] = "reduced depth (debug run)"
        if gemm_error is not None:
            out["invalid"] = gemm_error
        if os.environ.get("FVQA_BENCH_REHEARSAL") == "1":
            out["rehearsal"] = True
            out["invalid"] = "rehearsal: ranks share devices over gloo (not a scaling measurement)"
        if world > 1:
            out["value_per_gpu"] = value / world         # the N = 1-equivalent rate: read it against BENCH's `value`
        default_workload = (a.model == "7B" and a.batch_size == 8 and a.seq_len == 128 and a.dtype == "bf16"
                            and not (a.vaq or a.qav) and not a.n_layers)
        legs_on = a.full and world == 1 and default_workload and not a.no_other_configs
        if legs_on:
            # BASELINE configs[2..4] as one GPU runs them, driver-timed with the C2 line (round-4 verdict #3): free the C2
            # model first (7B: ~30 GiB with the transposed copies; the 13B leg needs ~58)
            import gc
            opt.grad_sync = None
            del net, opt, scaler, batches, model
            gc.collect()
            torch.cuda.empty_cache()
            out["other_configs"] = {}
            for name, c in OTHER_CONFIGS.items():
                t_leg = time.time()
                try:
                    out["other_configs"][name] = short_leg(dev, c["model"], c["batch_size"], c["seq_len"], c["vaq"], c["qav"],
                                                           lm_head=c.get("lm_head"))
                    out["other_configs"][name]["leg_wall_s"] = time.time() - t_leg
                except Exception as e:   # a leg must never take the headline measurement down
                    out["other_configs"][name] = {"error": repr(e)[:300]}
                print(f"[bench] {name}: {out['other_configs'][name]}", file=sys.stderr, flush=True)
        if a.full and world == 1 and not a.no_cpu_baseline:
            try:
                # with the legs on, ONE timed oracle step (warm-up + one: ~170 s on the box's 128 threads) keeps the command < 450 s
                out["cpu_baseline"] = cpu_baseline_leg(a.seq_len, 10, max_timed=1 if legs_on else 3)
            except Exception as e:   # the baseline leg must never take the GPU measurement down
                out["cpu_baseline"] = {"value": None, "error": repr(e)}
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    if gemm_error is not None:
        raise SystemExit(3)


if __name__ == "__main__":
    main()
