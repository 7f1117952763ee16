"""--train_audio on the GPU: the three new kernels against fp64 on the host, the step with the flag on against the fixtures
tools/gen_golden_audio_train.py takes from the reference run with its audio front end trainable, flag on against flag off, and
the trainer / checkpoint / data-parallel layers.

Bounds: the kernels are held to the forward front end's (tests/test_audio_gpu.py VP_F32: 2e-6 of the output's range against
fp64), the step to tests/test_step_gpu.py's FP32_RTOL / BF16_TOL / FP16_TOL. Two exceptions, both reasoned in the tests that
make them: the key bias (its gradient is zero in exact arithmetic) and the 16-bit builds' query / key gradients (held to the
error they inherit from the 16-bit incoming gradient, measured in the test itself through an fp64 restatement)."""
import math
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import engine  # noqa: E402
import util.misc as misc  # noqa: E402
from fvqa import ops, synth  # noqa: E402
from fvqa.optim import FusedAdamW, param_groups_weight_decay  # noqa: E402
from tests import audio_util  # noqa: E402
from tests import train_audio_util as U  # noqa: E402
from tests.parity import compare_with_golden  # noqa: E402
from tests.test_audio_gpu import KA, KV, VP_F32  # noqa: E402
from tests.test_kernels_gpu import DEV, dev, rel, rnd  # noqa: E402
from tests.test_step_gpu import BF16_LOSS_RTOL, BF16_TOL, FP16_LOSS_SCALE, FP16_TOL, FP32_RTOL, _free  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")
CA = "video_audio_cross_attn."
KEY_BIAS = CA + "key.bias"
QK = [CA + f"{m}.{w}" for m in ("query", "key") for w in ("weight", "bias")]      # differences of nearly equal terms


# ------------------------------------------------------------------------------ kernels against fp64
def _cross_attn_ref(q, kv, dx, B, F, T, E):
    qd = q.double().view(B, F, E).requires_grad_(True)
    kd = kv[:, :E].double().reshape(B, T, E).requires_grad_(True)
    vd = kv[:, E:].double().reshape(B, T, E).requires_grad_(True)
    x = torch.softmax(qd @ kd.transpose(1, 2) / math.sqrt(E), -1) @ vd
    x.backward(dx.double().view(B, F, E))
    return qd.grad.reshape(B * F, E), kd.grad.reshape(B * T, E), vd.grad.reshape(B * T, E)


# (F, T, scale of q) — x 30: the softmax is nearly one-hot, the maximum subtraction matters
CROSS_CASES = [(F, T, 1.0) for F in (1, 10) for T in (1, 3, 10, 16)] + [(10, 10, 30.0)]


@pytest.mark.parametrize("F,T,q_scale", CROSS_CASES)
def test_cross_attn_bwd_against_fp64(F, T, q_scale):
    B, E = 3, KV
    q, kv, dx = rnd(B * F, E, seed=1) * q_scale, rnd(B * T, 2 * E, seed=2), rnd(B * F, E, seed=3)
    qd, kvd, dxd = dev(q), dev(kv), dev(dx)
    outs = []
    for _ in range(2):                                        # written, not accumulated: NaN prefill; twice -> bitwise equal
        dq = torch.full((B * F, E), NAN, device=DEV)
        dkv = torch.full((B * T, 2 * E), NAN, device=DEV)     # dk | dv share one pitched buffer, as K | V do
        ops.av_cross_attn_bwd(qd, kvd[:, :E], kvd[:, E:], dxd, dq, dkv[:, :E], dkv[:, E:], B, F, T)
        outs.append((dq, dkv))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    dq, dkv = outs[0]
    rq, rk, rv = _cross_attn_ref(q, kv, dx, B, F, T, E)
    e_v = rel(dkv[:, E:], rv)
    print(f"cross attention bwd F={F} T={T} q x{q_scale}: dv {e_v:.2e}", end=" ")
    assert e_v < VP_F32
    if T == 1:                                                # one key: P is exactly 1, dS exactly 0
        assert not dq.any() and not dkv[:, :E].any()
        assert float(rq.abs().max()) < 1e-15 and float(rk.abs().max()) < 1e-15
        return
    e_q, e_k = rel(dq, rq), rel(dkv[:, :E], rk)
    print(f"dq {e_q:.2e} dk {e_k:.2e}")
    assert e_q < VP_F32 and e_k < VP_F32


def test_cross_attn_bwd_refuses_17_keys_and_bad_operands():
    B, F, E = 2, 4, 64
    q, dx, dq = (torch.zeros(B * F, E, device=DEV) for _ in range(3))
    kv, dkv = torch.zeros(B * 17, 2 * E, device=DEV), torch.zeros(B * 17, 2 * E, device=DEV)
    with pytest.raises(RuntimeError, match="ESHAPE"):
        ops.av_cross_attn_bwd(q, kv[:, :E], kv[:, E:], dx, dq, dkv[:, :E], dkv[:, E:], B, F, 17)
    kv, dkv = kv[:B * 3], dkv[:B * 3]
    with pytest.raises(ValueError):
        ops.av_cross_attn_bwd(q, kv[:, :E], kv[:, E:], dx, dq, dkv[:, :E], dkv[:, E:], B, F, 2)      # key rows != B * T
    with pytest.raises(RuntimeError, match="EALIGN"):
        ops.av_cross_attn_bwd(q, kv[:, 1:E + 1], kv[:, E:], dx, dq, dkv[:, :E], dkv[:, E:], B, F, 3)
    ops.av_cross_attn_bwd(q, kv[:, :E], kv[:, E:], dx, dq, dkv[:, :E], dkv[:, E:], B, F, 3)


@pytest.mark.parametrize("with_g1", [False, True])
@pytest.mark.parametrize("dim,k", [(512, 768), (4096, 768), (1536, 768)])
@pytest.mark.parametrize("rows", [30, 80, 130])               # 130: a second 128-row chunk of the matrix-core form
def test_proj_dx_against_fp64(rows, dim, k, with_g1):
    g0, g1 = rnd(rows, dim, seed=1), rnd(rows, dim, seed=2) if with_g1 else None
    wide = rnd(dim, k + 256, scale=1 / math.sqrt(k), seed=3)  # W = a column range of a wider matrix, at a non-zero start
    wd = dev(wide)[:, 128:128 + k]
    G = g0.double() + (g1.double() if with_g1 else 0)
    ref = G @ wide[:, 128:128 + k].double()
    outs = []
    for _ in range(2):
        dx = torch.full((rows, k), NAN, device=DEV)
        ops.av_proj_dx(dev(g0), dev(g1) if with_g1 else None, wd, dx)
        outs.append(dx)
    assert torch.equal(outs[0], outs[1])
    e = rel(outs[0], ref)
    print(f"proj dx rows={rows} dim={dim} k={k} g1={with_g1}: {e:.2e}")
    assert e < VP_F32
    # pitched gradient rows (dk | dv of the step are one buffer's two halves read as ONE 1536-wide g: here a real sub-range)
    if dim == 512:
        gw = dev(rnd(rows, dim + 64, seed=4))
        dx = torch.full((rows, k), NAN, device=DEV)
        ops.av_proj_dx(gw[:, 64:], None, wd, dx)
        assert rel(dx, gw[:, 64:].double().cpu() @ wide[:, 128:128 + k].double()) < VP_F32


def test_proj_dx_refuses_what_it_cannot_do():
    g, w, dx = torch.zeros(8, 96, device=DEV), torch.zeros(96, 64, device=DEV), torch.zeros(8, 64, device=DEV)
    with pytest.raises(RuntimeError, match="ESHAPE"):
        ops.av_proj_dx(g, None, w, dx)                        # dim % 64 != 0
    with pytest.raises(ValueError):
        ops.av_proj_dx(g[:, :64], None, w, dx)                # g and w disagree on dim


@pytest.mark.parametrize("rows", [8, 30, 80, 130])
def test_linear_bwd_weight_and_bias_against_fp64(rows):
    D, E = 1536, KV
    gw = rnd(rows, D + 128, seed=4)                           # pitched g: a column range of a wider matrix
    x, a = rnd(rows, E, seed=6), rnd(rows, KA, seed=7)
    gd = dev(gw)[:, 128:]
    G = gw[:, 128:].double()
    # accumulates (ones prefill): twice -> twice; into a column range: the columns outside keep their values
    runs = []
    for _ in range(2):
        dW, db = torch.ones(D, E + KA, device=DEV), torch.ones(D, device=DEV)
        for _ in range(2):
            ops.av_linear_bwd(gd, [(dev(x), dW[:, KA:])], db)
        runs.append((dW, db))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    dW, db = runs[0]
    assert torch.equal(dW[:, :KA], torch.ones(D, KA, device=DEV))
    e_w, e_b = rel(dW[:, KA:] - 1, 2 * (G.T @ x.double())), rel(db - 1, 2 * G.sum(0))
    print(f"linear bwd rows={rows}: dW {e_w:.2e} dbias {e_b:.2e}")
    assert e_w < VP_F32 and e_b < VP_F32
    # no bias; a 1024-wide source (audio_proj's); a 768-row g that is a whole matrix
    g2 = rnd(rows, E, seed=8)
    dW = torch.ones(E, KA, device=DEV)
    ops.av_linear_bwd(dev(g2), [(dev(a), dW)])
    assert rel(dW - 1, g2.double().T @ a.double()) < VP_F32
    # two sources in one call, the bias added once
    dW, db = torch.ones(D, E + KA, device=DEV), torch.ones(D, device=DEV)
    ops.av_linear_bwd(gd, [(dev(x), dW[:, :E]), (dev(a), dW[:, E:])], db)
    assert rel(dW - 1, G.T @ torch.cat([x, a], 1).double()) < VP_F32 and rel(db - 1, G.sum(0)) < VP_F32
    # a source wider than 1024 columns: the two-features-per-wave form, one launch per source, the bias on the first
    w = rnd(rows, E + KA, seed=9)
    dW, db = torch.ones(D, E + KA, device=DEV), torch.ones(D, device=DEV)
    ops.av_linear_bwd(gd, [(dev(w), dW)], db)
    assert rel(dW - 1, G.T @ w.double()) < VP_F32 and rel(db - 1, G.sum(0)) < VP_F32
    # a wide source and a narrow one in one call: one launch each, the bias still added once
    dW, db = torch.ones(D, 2 * E + KA, device=DEV), torch.ones(D, device=DEV)
    ops.av_linear_bwd(gd, [(dev(w), dW[:, :E + KA]), (dev(x), dW[:, E + KA:])], db)
    assert rel(dW - 1, G.T @ torch.cat([w, x], 1).double()) < VP_F32 and rel(db - 1, G.sum(0)) < VP_F32


def test_av_proj_bwd_keeps_its_results_beside_the_grown_kernel():
    """fvqa_av_proj_bwd shares its kernel body with fvqa_av_linear_bwd: G = d_tok alone through either entry is the same fma
    chain — bitwise equal."""
    R, F, D = 80, 10, 4096
    d_tok, v = dev(rnd(R, D, seed=4)), dev(rnd(R, KV, seed=6))
    dW0, dT0, dW1 = torch.zeros(D, KV, device=DEV), torch.zeros(F, D, device=DEV), torch.zeros(D, KV, device=DEV)
    ops.av_proj_bwd(d_tok, None, [(v, dW0)], dT0)
    ops.av_linear_bwd(d_tok, [(v, dW1)])
    assert torch.equal(dW0, dW1)


# ------------------------------------------------------------------------------ the step against the reference's fixtures
def _grad_err(g, name, grad):
    """tests.parity.compare_with_golden's error of one gradient record."""
    key = name.replace(".", "__")
    gr = grad.detach().double().cpu()
    nref = float(g[f"gradnorm__{key}"])
    e = abs(float(gr.norm()) - nref) / nref
    if f"grad__{key}" in g:
        ref = g[f"grad__{key}"]
        return max(e, float(np.abs(gr.numpy() - ref).max() / np.abs(ref).max()))
    ref = g[f"gradsample__{key}"]
    return max(e, float(np.abs(gr.flatten()[torch.from_numpy(g[f"gradpick__{key}"])].numpy() - ref).max() / np.abs(ref).max()))


def _without(g, names):
    drop = {f"gradnorm__{n.replace('.', '__')}" for n in names}
    return {k: v for k, v in g.items() if k not in drop}


def _front_bwd_fp64(model, batch, G, T):
    """The front end's backward of `attention`, restated in fp64 torch: gradients of audio_proj and the cross-attention for the
    incoming gradient G = d_tok + d_qav (vf = X·Wv^T, so the loss's dependence on the front end is sum(vf o G))."""
    dd = lambda t: t.detach().double().cpu()                  # noqa: E731
    p = {n: dd(t).requires_grad_(True) for n, t in model.named_parameters() if n.startswith(U.AUDIO_PREFIXES)}
    Wv = dd(model.visual_proj.weight)
    B, F = batch["video"].shape[0], model.max_feats
    video, audio = batch["video"].double().reshape(B, F, -1), batch["audio"].double().reshape(B, T, -1)
    a = audio @ p["audio_proj.weight"].T
    lin = lambda x, m: x @ p[CA + m + ".weight"].T + p[CA + m + ".bias"]      # noqa: E731
    q, k, v = lin(video, "query"), lin(a, "key"), lin(a, "value")
    x = torch.softmax(q @ k.transpose(1, 2) / math.sqrt(q.shape[-1]), -1) @ v
    ((x @ Wv.T) * G.view(B, F, -1)).sum().backward()
    return {n: t.grad for n, t in p.items()}


def _step_against_fixture(name, dtype):
    g, cfg = audio_util.golden_cfg(name)
    model, _ = U.build_model(cfg, dtype)
    batch = synth.make_batch(cfg, seed=0)
    w = FP16_LOSS_SCALE if dtype == torch.float16 else 1.0
    losses, grads, logits, layer_out = audio_util.run_step(model, batch, loss_weights=(w, w, w))
    grads = {n: x / w for n, x in grads.items()}
    assert all(torch.isfinite(x).all() for x in grads.values())
    flat = model.flat_params()
    assert set(flat.offsets) == {str(n) for n, t in zip(g["param_names"], g["param_trainable"]) if t}
    attention = cfg.audio == "attention"
    if dtype == torch.float32:
        kw = dict(rtol=FP32_RTOL, min_decided=0.99)
        held_out = [KEY_BIAS] if attention else []
    else:
        kw = dict(rtol=BF16_LOSS_RTOL, tol=BF16_TOL if dtype == torch.bfloat16 else FP16_TOL, min_decided=0.95)
        held_out = QK if attention else []
    rep = compare_with_golden(_without(g, held_out), losses, grads, logits, layer_out, **kw)
    print(name, dtype, losses, {k: f"{v:.2e}" if isinstance(v, float) else v for k, v in rep.items()})
    for n in U.audio_names(model):
        if n not in held_out:
            assert f"grad:{n}" in rep or float(g[f"gradnorm__{n.replace('.', '__')}"]) == 0.0, n
    if attention:
        # the key bias shifts every score of a query alike: its gradient is zero in exact arithmetic, the reference holds
        # rounding residue (1e-6 of the query bias's). Not compared: bounded against the query bias's gradient of the same step
        nk, nq = float(grads[KEY_BIAS].norm()), float(grads[CA + "query.bias"].norm())
        print(f"  key.bias norm {nk:.3e}, query.bias norm {nq:.3e}")
        assert nk <= 1e-4 * nq
    if attention and dtype != torch.float32:
        # query / key gradients of a 16-bit build: differences of nearly equal terms, fed by a G that went through 16-bit layers.
        # What G alone costs is measured: the product's own G through the fp64 restatement, against the fixture; the kernels
        # may add their own fp32 bound to at most twice that
        eng = model._engine
        ar = eng.arena(eng.n_streams * cfg.batch_size, batch["text_id"]["vqa"].shape[-1])
        G = (ar.d_tok.double() + ar.d_qav.double()).cpu() / w
        restated = _front_bwd_fp64(model, batch, G, cfg.audio_rows)
        for n in QK:
            if n == KEY_BIAS:
                continue
            inherited, own = _grad_err(g, n, restated[n]), _grad_err(g, n, grads[n])
            print(f"  {n}: inherited {inherited:.3e} kernels {own:.3e} bound {2 * inherited + VP_F32:.3e}")
            assert own <= 2 * inherited + VP_F32, n
    model._engine.check_gemm_error()
    _free(model)


@pytest.mark.parametrize("name", U.GOLDENS)
def test_fp32_step_with_trainable_audio_matches_the_reference(name):
    _step_against_fixture(name, torch.float32)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("name", U.WIDE)
def test_16bit_step_with_trainable_audio_against_the_reference(name, dtype):
    _step_against_fixture(name, dtype)


# ------------------------------------------------------------------------------ flag on against flag off, repeatability
def _run(model, batch):
    flat = model.flat_params()
    flat.zero_grad()
    vqa, vaq, qav = model(batch)
    (vqa + vaq + qav).sum().backward()
    torch.cuda.synchronize()
    return [float(x.detach()) for x in (vqa, vaq, qav)], flat.flat_grad.clone()


@pytest.mark.parametrize("mode,T", U.MODES)
def test_flag_on_changes_nothing_it_does_not_own(mode, T):
    cfg = synth.preset("tiny", vaq=True, qav=True, audio=mode, audio_len=T)
    batch = synth.make_batch(cfg, seed=4)
    off, _ = U.build_model(cfg, torch.bfloat16, train_audio=False)
    on, _ = U.build_model(cfg, torch.bfloat16, train_audio=True)
    l_off, g_off = _run(off, batch)
    l_on, g_on = _run(on, batch)
    assert l_off == l_on and all(math.isfinite(x) for x in l_on)
    f_off, f_on = off.flat_params(), on.flat_params()
    shared = [n for n in f_off.offsets]
    assert shared and set(shared) < set(f_on.offsets)
    for n in shared:
        assert torch.equal(f_off.grad_view(n), f_on.grad_view(n)), n
    for n in U.audio_names(on):
        assert n not in f_off.offsets and n in f_on.offsets
        if not (T == 1 and n in QK):                          # (one key: the query / key gradients are exact zeros)
            assert float(f_on.grad_view(n).abs().max()) > 0, n
    # flag off: the parent's layout and size
    D, A, L, F, H = cfg.dim, cfg.adapter_len, cfg.adapter_layer, cfg.max_feats, cfg.n_heads
    sizes = [A * L * D] + ([D * KV] if mode != "only" else []) + [F * D]
    assert f_off.gate_off == sum(sizes) and f_off.flat.numel() == sum(sizes) + cfg.n_layers * 2 * H
    assert [f_off.offsets[n][0] for n in f_off.names] == [sum(sizes[:i]) for i in range(len(sizes))]
    assert len(g_off) == f_off.flat.numel() < len(g_on)
    _free(off)
    _free(on)


@pytest.mark.parametrize("mode,T", U.MODES)
def test_step_with_the_flag_is_bitwise_repeatable_in_both_schedules(mode, T, monkeypatch):
    cfg = synth.preset("tiny", vaq=True, qav=True, audio=mode, audio_len=T)
    model, _ = U.build_model(cfg, torch.bfloat16)
    batch = synth.make_batch(cfg, seed=5)
    runs = {}
    for sched in ("native", "python"):
        if sched == "python":
            monkeypatch.setenv("FVQA_PY_SCHEDULE", "1")
        else:
            monkeypatch.delenv("FVQA_PY_SCHEDULE", raising=False)
        a, b = _run(model, batch), _run(model, batch)
        assert a[0] == b[0] and torch.equal(a[1], b[1]), sched
        runs[sched] = a
    assert runs["native"][0] == runs["python"][0] and torch.equal(runs["native"][1], runs["python"][1])
    _free(model)


# ------------------------------------------------------------------------------ trainer, optimizer, checkpoint
def _trainer(mode, accum, train_audio, dtype=torch.bfloat16):
    cfg = synth.preset("tiny", vaq=True, qav=True, audio=mode, audio_len=3 if mode == "attention" else 0)
    model, args = U.build_model(cfg, dtype, train_audio=train_audio)
    opt = FusedAdamW(param_groups_weight_decay(model, args.weight_decay), lr=0.01, betas=(0.9, 0.95), flat=model.flat_params())
    args.accum_iter, args.lr, args.warmup_epochs, args.epochs = accum, 0.01, 0, 1
    return cfg, model, args, opt


@pytest.mark.parametrize("accum", [1, 2])
@pytest.mark.parametrize("mode", ["sum", "attention"])
def test_training_moves_the_audio_tensors_only_with_the_flag(mode, accum):
    for train_audio in (True, False):
        cfg, model, args, opt = _trainer(mode, accum, train_audio)
        model.ensure_engine()
        before = {n: dict(model.named_parameters())[n].detach().clone() for n in U.audio_names(model)}
        stats = engine.train_one_epoch(model, synth.SyntheticLoader(cfg, 3), opt, 0, misc.NativeScalerWithGradNormCount(),
                                       args=args)
        torch.cuda.synchronize()
        assert all(math.isfinite(v) for v in stats.values())
        assert opt.step_dev.item() == 3 // accum
        own = dict(model.named_parameters())
        for n, t in before.items():
            if n != KEY_BIAS or not train_audio:              # (the key bias's gradient is rounding residue around zero)
                assert torch.equal(own[n].detach(), t) != train_audio, (n, train_audio)
        model._engine.check_gemm_error()
        _free(model)


def test_one_fused_adamw_step_on_the_audio_segments_matches_torch_adamw():
    """The bound of tests/test_train_gpu.py::test_one_optimizer_step_matches_oracle_plus_torch_adamw: the UPDATES of the
    sign-stable elements within rtol 2e-2, atol 1e-6 — against torch.optim.AdamW on the same values and gradients."""
    cfg, model, args, opt = _trainer("attention", 1, True, torch.float32)
    flat = model.flat_params()
    scaler = misc.NativeScalerWithGradNormCount()
    opt.zero_grad()
    start = {n: p.detach().double().cpu().clone() for n, p in model.named_parameters() if p.requires_grad}
    a, b, c = model(synth.make_batch(cfg, seed=7))
    scaler(a + b + c, opt, parameters=model.parameters(), update_grad=True)
    torch.cuda.synchronize()
    assert opt.step_dev.item() == 1.0
    grads = {n: flat.grad_view(n).detach().double().cpu().clone() for n in start}      # unscaled in place by the scaler
    own = dict(model.named_parameters())
    for n in U.audio_names(model):
        p = torch.nn.Parameter(start[n].clone())
        p.grad = grads[n].clone()
        wd = 0.0 if n.endswith(".bias") else args.weight_decay
        torch.optim.AdamW([p], lr=0.01, betas=(0.9, 0.95), weight_decay=wd).step()
        upd_ref, upd_got = p.detach() - start[n], own[n].detach().double().cpu() - start[n]
        big = grads[n].abs() > 1e-3 * grads[n].abs().max()
        assert big.any(), n
        assert torch.allclose(upd_got[big], upd_ref[big], rtol=2e-2, atol=1e-6), n
    _free(model)


def _reseed_audio(model, seed):
    """What another process seed does to the frozen audio front end (nn.Linear's rule, drawn from torch's generator)."""
    torch.manual_seed(seed)
    with torch.no_grad():
        for n, p in model.named_parameters():
            if n.startswith(U.AUDIO_PREFIXES):
                bound = 1 / math.sqrt(768 if n.startswith(CA) else KA)
                p.copy_((torch.rand(p.shape) * 2 - 1).to(p.device) * bound)


@pytest.mark.parametrize("mode", ["sum", "attention"])
def test_checkpoint_carries_the_trained_audio_front_end(tmp_path, mode):
    cfg, model, args, opt = _trainer(mode, 1, True)
    scaler = misc.NativeScalerWithGradNormCount()
    engine.train_one_epoch(model, synth.SyntheticLoader(cfg, 3), opt, 0, scaler, args=args)
    args.output_dir = str(tmp_path)
    misc.save_model(args, 0, model, model, opt, scaler, "checkpoint_best")
    ck = torch.load(tmp_path / "checkpoint_best.pth", map_location="cpu", weights_only=False)
    audio = U.audio_names(model)
    assert set(audio) <= set(ck["model"]) and set(ck["model"]) == set(model.flat_params().offsets)
    own = dict(model.named_parameters())
    assert all(torch.equal(ck["model"][n], own[n].detach().cpu()) for n in audio)
    batch = synth.make_batch(cfg, seed=21)
    with torch.no_grad():
        want = [float(x) for x in model(batch)]
    # an evaluation-only run in another process (another seed), WITHOUT the flag: it must see the trained audio front end
    other, args2 = U.build_model(cfg, torch.bfloat16, train_audio=False)
    _reseed_audio(other, 1234)
    with torch.no_grad():
        assert [float(x) for x in other(batch)] != want
    args2.resume, args2.eval = str(tmp_path / "checkpoint_best.pth"), True
    misc.load_model(args2, other, None, None)
    with torch.no_grad():
        assert [float(x) for x in other(batch)] == want
    # resuming with the flag: parameters, moments and step of the new segments come back
    cfg3, model3, args3, opt3 = _trainer(mode, 1, True)
    _reseed_audio(model3, 99)
    args3.resume = str(tmp_path / "checkpoint_best.pth")
    scaler3 = misc.NativeScalerWithGradNormCount()
    misc.load_model(args3, model3, opt3, scaler3)
    assert args3.start_epoch == 1
    assert torch.equal(model3.flat_params().flat, model.flat_params().flat)
    assert torch.equal(opt3.exp_avg, opt.exp_avg) and torch.equal(opt3.exp_avg_sq, opt.exp_avg_sq)
    assert opt3.step_dev.item() == opt.step_dev.item() == 3.0
    f3 = model3.flat_params()
    for n in audio:
        o, sz, _ = f3.offsets[n]
        if n != KEY_BIAS:                                     # (a zero gradient leaves zero moments)
            assert float(opt3.exp_avg_sq[o:o + sz].max()) > 0, n
    for m in (model, other, model3):
        _free(m)


def test_train_py_with_the_flag_end_to_end(tmp_path):
    """`python train.py --audio --audio_merge attention --train_audio` on synthetic batches (a two-layer model described by a
    params.json, closed-form weights): the run ends, the checkpoint holds the audio tensors beside the reference's keys, and a
    second run resumes from it."""
    import json
    pkg = os.path.join(ROOT, "flipped-vqa_amd")
    (tmp_path / "assets" / "tinyX").mkdir(parents=True)
    (tmp_path / "assets" / "tinyX" / "params.json").write_text(json.dumps(dict(dim=256, multiple_of=128, n_heads=2, n_layers=2,
                                                                               norm_eps=1e-5, vocab_size=-1)))
    env = dict(os.environ, FVQA_SYNTHETIC_TOKENIZER="1")
    out = str(tmp_path / "run")
    base = [sys.executable, "train.py", "--model", "tinyX", "--llama_model_path", str(tmp_path / "assets") + "/", "--random_init",
            "--synthetic", "--synthetic_batches", "3", "--batch_size", "2", "--max_seq_len", "32", "--adapter_layer", "2",
            "--warmup_epochs", "0", "--blr", "0.64", "--output_dir", out, "--vaq", "--qav", "--audio", "--audio_merge", "attention",
            "--train_audio"]
    r = subprocess.run(base + ["--epochs", "1"], cwd=pkg, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    ck = torch.load(os.path.join(out, "checkpoint_best.pth"), map_location="cpu", weights_only=False)
    audio = {"audio_proj.weight"} | {CA + f"{m}.{w}" for m in ("query", "key", "value") for w in ("weight", "bias")}
    assert audio <= set(ck["model"]) and len(ck["model"]) == 3 + 2 * 2 + len(audio)
    assert all(ck["model"][n].dtype == torch.float32 for n in audio)
    assert sum(len(g["params"]) for g in ck["optimizer"]["param_groups"]) == len(ck["model"])
    r2 = subprocess.run(base + ["--epochs", "2", "--resume", os.path.join(out, "checkpoint_best.pth")], cwd=pkg, env=env,
                        capture_output=True, text=True, timeout=300)
    assert r2.returncode == 0, (r2.stdout[-1500:], r2.stderr[-1500:])
    log = [json.loads(x) for x in open(os.path.join(out, "log.txt"))]
    assert [x["epoch"] for x in log] == [0, 1] and all(math.isfinite(x["train_loss"]) for x in log)
    ck2 = torch.load(os.path.join(out, "checkpoint_best.pth"), map_location="cpu", weights_only=False)
    assert not torch.equal(ck2["model"]["audio_proj.weight"], ck["model"]["audio_proj.weight"])


# ------------------------------------------------------------------------------ data parallel
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_two_replicas_with_trainable_audio_stay_bitwise_equal(tmp_path):
    """Two ranks (tests/train_audio_dp_worker.py: train.py's wiring, mode `attention`, three audio rows) that start from different
    trainables — the audio front end among them, now part of the flat buffer — leave DataParallel's constructor with rank 0's and
    hold bitwise-equal flat buffers after each of two steps; the audio segments moved."""
    from tests import train_audio_dp_worker as W
    world, port = 2, str(_free_port())
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="4")
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "train_audio_dp_worker.py"), str(r), str(world), port,
                               str(tmp_path)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
             for r in range(world)]
    outs = [p.communicate(timeout=600)[0] for p in procs]
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o[-3000:]
    t0, t1 = (torch.load(tmp_path / f"rank{r}.pt") for r in range(world))
    assert t0["names"] == t1["names"] and t0["numel"] == t1["numel"]
    assert not torch.equal(t0["p_start"], t1["p_start"])      # the ranks were built different ...
    assert torch.equal(t0["p_init"], t1["p_init"]) and torch.equal(t0["p_init"], t0["p_start"])      # ... rank 0's on both
    prev = t0["p_init"]
    for i in range(W.N_STEPS):
        assert torch.equal(t0[f"p{i}"], t1[f"p{i}"]), f"replicas diverged at step {i}"
        assert math.isfinite(t0[f"loss{i}"]) and math.isfinite(t1[f"loss{i}"])
        for n, (off, size, _) in t0["audio_segments"].items():
            if n != KEY_BIAS:                                 # (zero gradient, no decay on a bias: it stays)
                assert not torch.equal(t0[f"p{i}"][off:off + size], prev[off:off + size]), (i, n)
        prev = t0[f"p{i}"]
    assert set(t0["audio_segments"]) == {"audio_proj.weight"} | {CA + f"{m}.{w}" for m in ("query", "key", "value")
                                                                 for w in ("weight", "bias")}
