"""--train_norm on the GPU: fvqa_rmsnorm_dw against an fp64 restatement, the step with the flag on against the fixtures
tools/gen_golden_norm_train.py takes from the reference run with its norm weights trainable, flag on against flag off, the
masters / working copies through the optimizer, the checkpoint, evaluation, train.py and two data-parallel ranks.

Bounds. The kernel: per column rows * 2^-23 * sum_r |g * xhat| — the bound of an fp32 sum of that many fp32 products (each
product and each of the rows - 1 additions rounds once, unit roundoff 2^-24, in whatever order; the factor 2 covers the second
order terms), derived, not measured; with `accumulate` one more fp32 addition onto the prefill, 2^-24 of the result. The step:
tests/test_step_gpu.py's FP32_RTOL / BF16_TOL / FP16_TOL, every gradient record of the fixture, the norm weights' included."""
import json
import math
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import util.misc as misc  # noqa: E402
from fvqa import _lib, ops, synth  # noqa: E402
from fvqa.optim import FusedAdamW, param_groups_weight_decay  # noqa: E402
from tests import audio_util, gpu_util  # noqa: E402
from tests import train_norm_util as U  # noqa: E402
from tests.parity import compare_with_golden  # noqa: E402
from tests.test_kernels_gpu import DEV, DTYPES, dev, rnd  # noqa: E402
from tests.test_step_gpu import BF16_LOSS_RTOL, BF16_TOL, FP16_LOSS_SCALE, FP16_TOL, FP32_RTOL, _free  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")
SHAPES = [(1, 256), (7, 256), (130, 4096), (33, 5120), (1025, 8192)]


# ------------------------------------------------------------------------------ the kernel against fp64
def _operands(rows, dim, dtype, seed=0):
    """g, x in storage precision (CPU), rstd fp32 as the forward leaves it: rsqrt(mean(x^2) + eps) in fp32."""
    g, x = rnd(rows, dim, dtype=dtype, seed=seed + 1), rnd(rows, dim, dtype=dtype, scale=3.0, seed=seed + 2)
    rstd = torch.rsqrt(x.float().pow(2).mean(-1) + 1e-6)
    return g, x, rstd


def _restate(g, x, rstd, rounded=True):
    """fp64: dw[c] = sum_r g[r,c] * xhat[r,c], xhat = the fp32 product x * rstd rounded to the storage type (the forward's
    `.type_as(x)`), or left unrounded. -> (dw, per-column bound rows * 2^-23 * sum_r |g * xhat|)."""
    xh = x.float() * rstd[:, None]
    xh = xh.to(x.dtype).double() if rounded else xh.double()
    prod = g.double() * xh
    return prod.sum(0), x.shape[0] * 2.0 ** -23 * prod.abs().sum(0)


def _dw(g, x, rstd, accumulate=False, prefill=None):
    rows, dim = x.shape
    ws = torch.empty(ops.rmsnorm_dw_workspace(rows, dim, x.dtype), dtype=torch.uint8, device=DEV)
    ws.fill_(0xFF)                                             # (no initial state is assumed: NaN patterns)
    dw = torch.full((dim,), NAN, device=DEV) if prefill is None else dev(prefill.clone())
    ops.rmsnorm_dw(dev(g), dev(x), dev(rstd), dw, ws, accumulate)
    torch.cuda.synchronize()
    return dw.double().cpu()


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows,dim", SHAPES)
def test_rmsnorm_dw_against_fp64(rows, dim, dtype, accumulate):
    g, x, rstd = _operands(rows, dim, dtype)
    ref, bound = _restate(g, x, rstd)
    pre = rnd(dim, seed=9) if accumulate else None
    runs = [_dw(g, x, rstd, accumulate, pre) for _ in range(2)]
    assert torch.equal(runs[0], runs[1])                        # two launches, equal bits
    got = runs[0]
    assert torch.isfinite(got).all()
    if accumulate:
        want = pre.double() + ref
        bound = bound + 2.0 ** -24 * want.abs()
    else:
        want = ref
    err = (got - want).abs()
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"rmsnorm_dw rows={rows} dim={dim} {dtype} accumulate={accumulate}: worst err / bound {worst:.3f}")
    assert bool((err <= bound).all()), worst


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows,dim", SHAPES)
def test_rmsnorm_dw_sees_the_last_row_and_the_last_columns(rows, dim, dtype):
    g, x, rstd = _operands(rows, dim, dtype, seed=3)
    last_row = torch.zeros_like(g)
    last_row[-1] = g[-1]
    ref, bound = _restate(last_row, x, rstd)
    assert float(ref.abs().min()) >= 0 and float(ref.abs().max()) > 0
    got = _dw(last_row, x, rstd)
    assert bool(((got - ref).abs() <= bound).all())
    assert int((got != 0).sum()) >= int(0.9 * dim)              # a dropped row tail would leave zeros
    last_cols = torch.zeros_like(g)
    last_cols[:, -8:] = g[:, -8:]
    ref, bound = _restate(last_cols, x, rstd)
    got = _dw(last_cols, x, rstd)
    assert bool(((got - ref).abs() <= bound).all())
    assert not got[:-8].any() and bool((got[-8:] != 0).all())


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_rmsnorm_dw_rounds_the_normalised_value_as_the_forward_does(dtype):
    """(7, 256): few rows keep the bound (rows^2 * 2^-23 of a mean product) far below what the rounding of x * rstd to 16 bits moves
    (2^-9 / 2^-12 of a product, times sqrt(rows)): the kernel must sit on the rounded restatement and off the unrounded one."""
    g, x, rstd = _operands(7, 256, dtype, seed=5)
    ref_r, bound = _restate(g, x, rstd, rounded=True)
    ref_u, bound_u = _restate(g, x, rstd, rounded=False)
    assert int(((ref_r - ref_u).abs() > bound + bound_u).sum()) > 128      # the two restatements are apart on most columns
    got = _dw(g, x, rstd)
    assert bool(((got - ref_r).abs() <= bound).all())
    missed = int(((got - ref_u).abs() > bound_u).sum())
    print(f"{dtype}: off the unrounded restatement on {missed} of 256 columns")
    assert missed > 128


def test_rmsnorm_dw_refuses_bad_operands():
    g, x, rstd = (dev(t) for t in _operands(8, 256, torch.bfloat16))
    dw = torch.zeros(256, device=DEV)
    ws = torch.empty(ops.rmsnorm_dw_workspace(8, 256, torch.bfloat16), dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError):
        ops.rmsnorm_dw(g, x.float(), rstd, dw, ws)              # dtypes differ
    with pytest.raises(ValueError):
        ops.rmsnorm_dw(g, x, rstd, dw[:128], ws)                # dw is not (dim,)
    with pytest.raises(ValueError):
        ops.rmsnorm_dw(g, x, rstd, dw, ws[:-1])                 # short workspace
    with pytest.raises(ValueError):
        ops.rmsnorm_dw(g, x, rstd[:4], dw, ws)
    with pytest.raises(RuntimeError, match="ESHAPE"):           # dim % 8
        ops.rmsnorm_dw(g.view(-1)[:8 * 252].view(8, 252), x.view(-1)[:8 * 252].view(8, 252), rstd, torch.zeros(252, device=DEV), ws)
    with pytest.raises(RuntimeError, match="EALIGN"):
        ops.rmsnorm_dw(g, x, rstd, dw, torch.empty(ws.numel() + 16, dtype=torch.uint8, device=DEV)[8:])
    ops.rmsnorm_dw(g, x, rstd, dw, ws, False)
    assert float(dw.abs().max()) > 0


# ------------------------------------------------------------------------------ the step against the reference's fixtures
def _grad_err(g, name, grad):
    """tests.parity.compare_with_golden's error of one gradient record."""
    key = name.replace(".", "__")
    gr = grad.detach().double().cpu()
    nref = float(g[f"gradnorm__{key}"])
    e = abs(float(gr.norm()) - nref) / nref
    ref = g[f"grad__{key}"]
    return max(e, float(np.abs(gr.numpy() - ref).max() / np.abs(ref).max()))


def _step_against_fixture(name, dtype, monkeypatch):
    """One model, four steps: the native schedule with the dense and the scored-rows head against the fixture, then the Python
    schedule of both, which must leave the native schedule's bits."""
    g, cfg = audio_util.golden_cfg(name)
    model, _ = U.build_model(cfg, dtype)
    batch = synth.make_batch(cfg, seed=0)
    w = FP16_LOSS_SCALE if dtype == torch.float16 else 1.0
    flat = model.flat_params()
    # (the gates of an unwalked layer are segments of the flat buffer as ever; its norms, which the generator unfroze, are not)
    assert {n for n in flat.offsets if "gate" not in n} == {
        str(n) for n, t in zip(g["param_names"], g["param_trainable"])
        if t and "gate" not in str(n) and f"gradnone__{str(n).replace('.', '__')}" not in g}
    if dtype == torch.float32:
        kw = dict(rtol=FP32_RTOL)
    else:
        kw = dict(rtol=BF16_LOSS_RTOL, tol=BF16_TOL if dtype == torch.bfloat16 else FP16_TOL)
    # the decided fraction of the argmax rows, as tests/test_step_gpu.py asks: 0.99 in fp32; 16 bit: 0.95 peaked, 0.7 random heads
    decided = 0.99 if dtype == torch.float32 else (0.95 if name.endswith("_peaked") else 0.7)
    native = {}
    for head in ("all", "scored"):
        monkeypatch.delenv("FVQA_PY_SCHEDULE", raising=False)
        losses, grads, logits, layer_out = gpu_util.run_step(model, batch, loss_weights=(w, w, w), lm_head=head)
        native[head] = (losses, {n: x.clone() for n, x in grads.items()})
        grads = {n: x / w for n, x in grads.items()}
        assert all(torch.isfinite(x).all() for x in grads.values())
        errs = {n: _grad_err(g, n, grads[n]) for n in U.norm_names(model)}
        print(name, dtype, head, "norm gradients: worst", f"{max(errs.values()):.3e}", {n: f"{e:.2e}" for n, e in errs.items()})
        rep = compare_with_golden(g, losses, grads, logits, layer_out, scored_rows_only=head == "scored",
                                  min_decided=decided if head == "all" else 0.0, **kw)
        print(name, dtype, head, losses, {k: f"{v:.2e}" if isinstance(v, float) else v for k, v in rep.items()})
        for n in U.norm_names(model):                           # every norm the flag trains was compared, and is not zero
            assert f"grad:{n}" in rep and float(grads[n].abs().max()) > 0, n
    monkeypatch.setenv("FVQA_PY_SCHEDULE", "1")
    for head in ("all", "scored"):
        losses, grads, _, _ = gpu_util.run_step(model, batch, loss_weights=(w, w, w), lm_head=head)
        assert losses == native[head][0], head
        for n, x in grads.items():
            assert torch.equal(x, native[head][1][n]), (head, n)
    monkeypatch.delenv("FVQA_PY_SCHEDULE", raising=False)
    model._engine.check_gemm_error()
    _free(model)


@pytest.mark.parametrize("name", U.GOLDENS)
def test_fp32_step_with_trainable_norms_matches_the_reference(name, monkeypatch):
    _step_against_fixture(name, torch.float32, monkeypatch)


@pytest.mark.parametrize("name,dtype", [(U.WIDE[0], torch.bfloat16), (U.WIDE[0], torch.float16), ("norm_train_tiny_all", torch.float16)])
def test_16bit_step_with_trainable_norms_against_the_reference(name, dtype, monkeypatch):
    _step_against_fixture(name, dtype, monkeypatch)


def test_unwalked_layers_keep_frozen_norms_and_record_no_gradient():
    g, cfg = audio_util.golden_cfg("norm_train_tiny_l3_a2_all")
    assert cfg.adapter_layer < cfg.n_layers
    model, _ = U.build_model(cfg, torch.float32)
    flat = model.flat_params()
    for m in ("attention_norm", "ffn_norm"):
        key = f"layers__0__{m}__weight"
        assert f"gradnone__{key}" in g and f"gradnorm__{key}" not in g
        assert f"layers.0.{m}.weight" not in flat.offsets
    _free(model)


# ------------------------------------------------------------------------------ isolation
def _run(model, batch):
    flat = model.flat_params()
    flat.zero_grad()
    vqa, vaq, qav = model(batch)
    (vqa + vaq + qav).sum().backward()
    torch.cuda.synchronize()
    return [float(x.detach()) for x in (vqa, vaq, qav)], flat.flat_grad.clone()


@pytest.mark.parametrize("over", [dict(), dict(n_layers=3, adapter_layer=2)])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_flag_on_changes_nothing_it_does_not_own(dtype, over):
    cfg = synth.preset("tiny", vaq=True, qav=True, **over)
    batch = synth.make_batch(cfg, seed=4)
    off, _ = U.build_model(cfg, dtype, train_norm=False)
    on, _ = U.build_model(cfg, dtype, train_norm=True)
    l_off, g_off = _run(off, batch)
    l_on, g_on = _run(on, batch)
    assert l_off == l_on and all(math.isfinite(x) for x in l_on)
    f_off, f_on = off.flat_params(), on.flat_params()
    shared = list(f_off.offsets)
    assert shared and set(shared) < set(f_on.offsets)
    for n in shared:
        assert torch.equal(f_off.grad_view(n), f_on.grad_view(n)), n
    for n in U.norm_names(on):
        assert n not in f_off.offsets and float(f_on.grad_view(n).abs().max()) > 0, n
    assert set(f_on.offsets) - set(shared) == set(U.norm_names(on))
    # flag off: the parent's layout and size
    D, A, L, F, H = cfg.dim, cfg.adapter_len, cfg.adapter_layer, cfg.max_feats, cfg.n_heads
    assert f_off.gate_off == A * L * D + D * 768 + F * D and f_off.flat.numel() == f_off.gate_off + cfg.n_layers * 2 * H
    assert len(g_on) == len(g_off) + (2 * L + 1) * D
    assert off._engine.norm_work is None and not hasattr(off._engine.arena(3 * cfg.batch_size, cfg.max_seq_len), "dw_ws")
    _free(off)
    _free(on)


@pytest.mark.parametrize("head", ["all", "scored"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_layers_bwd_norm_with_a_null_struct_is_layers_bwd(dtype, head, monkeypatch):
    cfg = synth.preset("tiny", vaq=True, qav=True)
    model, _ = U.build_model(cfg, dtype, train_norm=False)
    model.ensure_engine().lm_head_rows = head
    batch = synth.make_batch(cfg, seed=6)
    monkeypatch.delenv("FVQA_PY_SCHEDULE", raising=False)
    plain = _run(model, batch)
    lib, calls = _lib.load(dtype), []

    def through_the_new_entry(plan, dxnf, out, stream):
        calls.append(1)
        return lib.fvqa_layers_bwd_norm(plan, dxnf, out, None, stream)

    monkeypatch.setattr(lib, "fvqa_layers_bwd", through_the_new_entry)
    other = _run(model, batch)
    assert calls == [1]
    assert plain[0] == other[0] and torch.equal(plain[1], other[1])
    _free(model)


# ------------------------------------------------------------------------------ optimizer and working copies
def _trainer(dtype=torch.bfloat16, over=None, train_norm=True):
    cfg = synth.preset("tiny", vaq=True, qav=True, **(over or {}))
    model, args = U.build_model(cfg, dtype, train_norm=train_norm)
    opt = FusedAdamW(param_groups_weight_decay(model, args.weight_decay), lr=0.01, betas=(0.9, 0.95), flat=model.flat_params())
    args.accum_iter, args.lr, args.warmup_epochs, args.epochs = 1, 0.01, 0, 1
    return cfg, model, args, opt


def _working_equals_rounded_masters(model):
    eng = model._engine
    blk = model.flat_params().norm_block(model.flat_params().flat)
    assert eng.norm_master.data_ptr() == blk.data_ptr() and tuple(eng.norm_work.shape) == tuple(blk.shape)
    assert torch.equal(eng.norm_work, blk.to(eng.dtype))
    L = eng.L
    for i in range(L):
        assert eng.pack.an[i].data_ptr() == eng.norm_work[i].data_ptr() and eng.pack.fn[i].data_ptr() == eng.norm_work[L + i].data_ptr()
    assert eng.pack.norm.data_ptr() == eng.norm_work[2 * L].data_ptr()
    if eng.dtype == torch.float32:
        assert eng.norm_work.data_ptr() == blk.data_ptr()       # the fp32 build reads the masters themselves


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
def test_one_fused_adamw_step_on_the_norm_masters_matches_torch_adamw(dtype):
    """The bound of tests/test_train_audio_gpu.py::test_one_fused_adamw_step_on_the_audio_segments_matches_torch_adamw: the UPDATES
    of the sign-stable elements within rtol 2e-2, atol 1e-6 — against torch.optim.AdamW (no decay: the norms are 1-D) on the same
    values and gradients. Then an overflow step: found_inf is set, neither the masters nor the working copies move."""
    cfg, model, args, opt = _trainer(dtype)
    flat = model.flat_params()
    _working_equals_rounded_masters(model)
    scaler = misc.NativeScalerWithGradNormCount(init_scale=FP16_LOSS_SCALE)      # (a scale the fp16 build does not overflow at)
    opt.zero_grad()
    names = U.norm_names(model)
    start = {n: dict(model.named_parameters())[n].detach().double().cpu().clone() for n in names}
    a, b, c = model(synth.make_batch(cfg, seed=7))
    scaler(a + b + c, opt, parameters=model.parameters(), update_grad=True)
    torch.cuda.synchronize()
    assert opt.step_dev.item() == 1.0 and float(scaler._found.item()) == 0.0
    grads = {n: flat.grad_view(n).detach().double().cpu().clone() for n in names}      # unscaled in place by the scaler
    own = dict(model.named_parameters())
    for n in names:
        p = torch.nn.Parameter(start[n].clone())
        p.grad = grads[n].clone()
        torch.optim.AdamW([p], lr=0.01, betas=(0.9, 0.95), weight_decay=0.0).step()
        upd_ref, upd_got = p.detach() - start[n], own[n].detach().double().cpu() - start[n]
        big = grads[n].abs() > 1e-3 * grads[n].abs().max()
        assert big.any() and float(upd_got.abs().max()) > 0, n
        assert torch.allclose(upd_got[big], upd_ref[big], rtol=2e-2, atol=1e-6), n
    _working_equals_rounded_masters(model)
    # an overflow step
    masters, work = flat.flat.clone(), model._engine.norm_work.clone()
    o_norm = flat.offsets["norm.weight"][0]
    opt.grad_sync = lambda: (flat.flat_grad[o_norm + 7].fill_(float("inf")), 1)[1]      # after the backward, ahead of the unscale
    opt.zero_grad()
    a, b, c = model(synth.make_batch(cfg, seed=8))
    scaler(a + b + c, opt, parameters=model.parameters(), update_grad=True)
    torch.cuda.synchronize()
    assert float(scaler._found.item()) == 1.0 and opt.step_dev.item() == 1.0
    assert torch.equal(flat.flat, masters) and torch.equal(model._engine.norm_work, work)
    _free(model)


# ------------------------------------------------------------------------------ evaluation sees what was trained
@pytest.mark.parametrize("over", [dict(), dict(n_layers=3, adapter_layer=2)])
def test_score_options_after_training_equals_a_fresh_model_from_the_checkpoint(tmp_path, over):
    cfg, model, args, opt = _trainer(torch.bfloat16, over)
    scaler = misc.NativeScalerWithGradNormCount()
    val = synth.make_option_batch(cfg, 5, seed=2)
    with torch.no_grad():
        before = model.score_options(val).clone()
    for i in range(2):
        opt.zero_grad()
        a, b, c = model(synth.make_batch(cfg, seed=30 + i))
        scaler(a + b + c, opt, parameters=model.parameters(), update_grad=True)
    with torch.no_grad():
        want = model.score_options(val).clone()
    assert not torch.equal(want, before)                        # the trained norms reached the scoring path
    _working_equals_rounded_masters(model)
    args.output_dir = str(tmp_path)
    misc.save_model(args, 0, model, model, opt, scaler, "checkpoint_best")
    ck = torch.load(tmp_path / "checkpoint_best.pth", map_location="cpu", weights_only=False)
    names = U.norm_names(model)
    assert set(names) <= set(ck["model"]) and set(ck["model"]) == set(model.flat_params().offsets)
    own = dict(model.named_parameters())
    assert all(torch.equal(ck["model"][n], own[n].detach().cpu()) and ck["model"][n].dtype == torch.float32 for n in names)
    # a fresh model with the flag, its engine built BEFORE the load: the working copies must follow the loaded masters
    fresh, args2 = U.build_model(cfg, torch.bfloat16)
    fresh.ensure_engine()
    with torch.no_grad():
        assert torch.equal(fresh.score_options(val), before)
    args2.resume, args2.eval = str(tmp_path / "checkpoint_best.pth"), True
    misc.load_model(args2, fresh, None, None)
    _working_equals_rounded_masters(fresh)
    with torch.no_grad():
        assert torch.equal(fresh.score_options(val), want)
    # a run WITHOUT the flag takes the norm weights of the checkpoint as frozen values: the rounded masters, the same bits
    other, args3 = U.build_model(cfg, torch.bfloat16, train_norm=False)
    args3.resume, args3.eval = str(tmp_path / "checkpoint_best.pth"), True
    misc.load_model(args3, other, None, None)
    with torch.no_grad():
        assert torch.equal(other.score_options(val), want)
    # resuming with the flag: parameters, moments and step come back
    cfg4, model4, args4, opt4 = _trainer(torch.bfloat16, over)
    args4.resume = str(tmp_path / "checkpoint_best.pth")
    misc.load_model(args4, model4, opt4, misc.NativeScalerWithGradNormCount())
    assert args4.start_epoch == 1 and torch.equal(model4.flat_params().flat, model.flat_params().flat)
    assert torch.equal(opt4.exp_avg, opt.exp_avg) and torch.equal(opt4.exp_avg_sq, opt.exp_avg_sq) and opt4.step_dev.item() == 2.0
    o, sz, _ = model4.flat_params().offsets["norm.weight"]
    assert float(opt4.exp_avg_sq[o:o + sz].max()) > 0
    for m in (model, fresh, other, model4):
        _free(m)


# ------------------------------------------------------------------------------ train.py end to end
def test_train_py_with_the_flag_resumes_where_the_uninterrupted_run_went(tmp_path):
    """`python train.py --random_init --synthetic --train_norm` on a three-layer model (two walked) described by a params.json:
    two epochs in one run, against one epoch + a resumed second one. A constant learning rate (--lr == --min_lr) keeps the two
    schedules alike; the checkpoints after epoch 1 must then hold the same bits."""
    pkg = os.path.join(ROOT, "flipped-vqa_amd")
    (tmp_path / "assets" / "tinyX").mkdir(parents=True)
    (tmp_path / "assets" / "tinyX" / "params.json").write_text(json.dumps(dict(dim=256, multiple_of=128, n_heads=2, n_layers=3,
                                                                               norm_eps=1e-5, vocab_size=-1)))
    env = dict(os.environ, FVQA_SYNTHETIC_TOKENIZER="1")

    def run(out, *extra):
        cmd = [sys.executable, "train.py", "--model", "tinyX", "--llama_model_path", str(tmp_path / "assets") + "/", "--random_init",
               "--synthetic", "--synthetic_batches", "3", "--batch_size", "2", "--max_seq_len", "32", "--adapter_layer", "2",
               "--warmup_epochs", "0", "--lr", "0.005", "--min_lr", "0.005", "--output_dir", str(tmp_path / out), "--vaq", "--qav",
               "--train_norm", *extra]
        r = subprocess.run(cmd, cwd=pkg, env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
        return torch.load(tmp_path / out / "checkpoint_best.pth", map_location="cpu", weights_only=False)

    whole = run("whole", "--epochs", "2")
    first = run("parts", "--epochs", "1")
    norms = synth.norm_train_names([1, 2])
    assert set(norms) <= set(first["model"]) and len(first["model"]) == 3 + 2 * 3 + len(norms)
    assert not any(n.startswith("layers.0.") and "norm" in n for n in first["model"])
    assert all(first["model"][n].dtype == torch.float32 and tuple(first["model"][n].shape) == (256,) for n in norms)
    assert sum(len(g["params"]) for g in first["optimizer"]["param_groups"]) == len(first["model"])
    assert len(first["optimizer"]["param_groups"][0]["params"]) == len(norms) and first["optimizer"]["param_groups"][0]["weight_decay"] == 0.0
    second = run("parts", "--epochs", "2", "--resume", str(tmp_path / "parts" / "checkpoint_best.pth"))
    log = [json.loads(x) for x in open(tmp_path / "parts" / "log.txt")]
    assert [x["epoch"] for x in log] == [0, 1] and all(math.isfinite(x["train_loss"]) for x in log)
    assert whole["epoch"] == second["epoch"] == 1 and set(whole["model"]) == set(second["model"])
    for n in whole["model"]:
        assert torch.equal(whole["model"][n], second["model"][n]), n
    for n in norms:
        assert not torch.equal(second["model"][n], first["model"][n]), n
    log_whole = [json.loads(x) for x in open(tmp_path / "whole" / "log.txt")]
    assert log_whole[1]["train_loss"] == log[1]["train_loss"]


# ------------------------------------------------------------------------------ data parallel
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_two_replicas_with_trainable_norms_stay_bitwise_equal_and_match_the_one_process_average(tmp_path):
    """Two ranks (tests/train_norm_dp_worker.py: train.py's wiring on a bf16 model) that start from different trainables — the norm
    masters among them — leave DataParallel's constructor with rank 0's masters AND working copies, hold bitwise-equal flat
    buffers after each of two steps, and equal ONE process that runs both shards and averages itself."""
    from tests import dp_worker, train_norm_dp_worker as W
    world, port = 2, str(_free_port())
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="4")
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "train_norm_dp_worker.py"), str(r), str(world), port,
                               str(tmp_path)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
             for r in range(world)]
    outs = [p.communicate(timeout=600)[0] for p in procs]
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o[-3000:]
    t0, t1 = (torch.load(tmp_path / f"rank{r}.pt") for r in range(world))
    assert t0["names"] == t1["names"] and t0["numel"] == t1["numel"]
    assert not torch.equal(t0["p_start"], t1["p_start"])      # the ranks were built different ...
    assert torch.equal(t0["p_init"], t1["p_init"]) and torch.equal(t0["p_init"], t0["p_start"])      # ... rank 0's on both
    assert torch.equal(t0["work_init"], t1["work_init"])      # and the working copies followed the broadcast
    segs = t0["norm_segments"]
    off0 = min(o for o, _, _ in segs.values())
    n_norm = sum(sz for _, sz, _ in segs.values())
    assert torch.equal(t0["work_init"].view(-1), t0["p_init"][off0:off0 + n_norm].to(W.DTYPE).float())
    prev = t0["p_init"]
    for i in range(W.N_STEPS):
        assert torch.equal(t0[f"p{i}"], t1[f"p{i}"]), f"replicas diverged at step {i}"
        assert torch.equal(t0[f"work{i}"], t1[f"work{i}"])
        assert torch.equal(t0[f"work{i}"].view(-1), t0[f"p{i}"][off0:off0 + n_norm].to(W.DTYPE).float())
        assert math.isfinite(t0[f"loss{i}"]) and math.isfinite(t1[f"loss{i}"])
        for n, (off, size, _) in segs.items():
            assert not torch.equal(t0[f"p{i}"][off:off + size], prev[off:off + size]), (i, n)
        prev = t0[f"p{i}"]
    # ONE process doing both shards and the mean itself (what the all-reduce computes)
    cfg = synth.preset("tiny", vaq=True, qav=True)
    model, args = U.build_model(cfg, W.DTYPE)
    dp_worker.perturb_trainables(model, seed=1000)             # rank 0's start, written behind the engine's back:
    model.refresh_norm_working()                               # whoever writes the masters refreshes the working copies
    flat = model.flat_params()
    assert torch.equal(flat.flat.cpu(), t0["p_init"])
    opt = FusedAdamW(param_groups_weight_decay(model, args.weight_decay), lr=0.01, betas=(0.9, 0.95), flat=flat)
    scaler = misc.NativeScalerWithGradNormCount()
    scaler._lazy(flat.flat.device)
    for i in range(W.N_STEPS):
        opt.zero_grad()
        a, b, c = model(synth.make_batch(cfg, seed=dp_worker.batch_seed(1, world, i)))
        ((a + b + c) * scaler._scale).sum().backward()
        g1 = flat.flat_grad.clone()
        opt.zero_grad()
        a, b, c = model(synth.make_batch(cfg, seed=dp_worker.batch_seed(0, world, i)))
        opt.grad_sync = lambda: (flat.flat_grad.add_(g1), world)[1]      # SUM + replica count, as DataParallel.sync_grads
        scaler(a + b + c, opt, parameters=None, update_grad=True)
        torch.cuda.synchronize()
        assert torch.equal(flat.flat.cpu(), t0[f"p{i}"]), f"2-rank result != single-process average at step {i}"
    _free(model)
