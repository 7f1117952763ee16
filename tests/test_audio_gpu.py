"""Audio fusion on the GPU (reference llama/model.py:209-227,306-324: --audio with concat / sum / attention / audio_only):
the three front-end kernels against fp64 on the host, and the whole step in every mode against the goldens that
tools/gen_golden_audio.py takes from the reference itself.

Bounds are the ones the video-only path is held to, taken from where they are stated: tests/test_kernels_gpu.py's
test_visual_proj for the kernels (2e-6 of the output's range against fp64; 5e-3 for a 16-bit cast output), tests/test_step_gpu.py's
FP32_RTOL / BF16_TOL / FP16_TOL (and its decided-row floors: 0.99 fp32, 0.95 on peaked fixtures, 0.7 fp16 on random-head ones)
for the step. That file binds no bf16 step of the `tiny` preset to a golden, so the bf16 build is bound at 7B width only; the
fp16 build is bound at both, as there."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from fvqa import ops, synth  # noqa: E402
from tests import audio_util  # noqa: E402
from tests.parity import compare_with_golden  # noqa: E402
from tests.test_kernels_gpu import DEV, DTYPES, dev, rel, rnd, tol  # noqa: E402
from tests.test_step_gpu import BF16_LOSS_RTOL, BF16_TOL, FP16_LOSS_SCALE, FP16_TOL, FP32_RTOL, _free  # noqa: E402

VP_F32, VP_H16 = 2e-6, 5e-3        # tests/test_kernels_gpu.py::test_visual_proj: raw output / cast output of a 16-bit build
KV, KA = 768, 1024


# ------------------------------------------------------------------------------ kernels
def _layout(layout, R, D, seed):
    """-> ([(x, w)] host tensors, fp64 reference of sum x·w^T). Weights of `concat` are two column ranges of ONE matrix."""
    if layout == "concat":
        v, a, W = rnd(R, KV, seed=seed), rnd(R, KA, seed=seed + 1), rnd(D, KV + KA, scale=1 / math.sqrt(KV + KA), seed=seed + 2)
        return [(v, W, 0), (a, W, KV)], torch.cat([v, a], 1).double() @ W.double().T
    if layout == "sum":
        v, a = rnd(R, KV, seed=seed), rnd(R, KA, seed=seed + 1)
        Wv, Wa = rnd(D, KV, scale=1 / math.sqrt(KV), seed=seed + 2), rnd(D, KA, scale=1 / math.sqrt(KA), seed=seed + 3)
        return [(a, Wa, 0), (v, Wv, 0)], a.double() @ Wa.double().T + v.double() @ Wv.double().T
    # "proj": the one-source projections of `attention`; "wide": one source past the 2048 columns the wave-per-feature kernel
    # holds in registers, K % 64 != 0: streamed by it at every row count
    k = {"only": KA, "proj": KV, "wide": 2052}[layout]
    x, W = rnd(R, k, seed=seed), rnd(D, k, scale=1 / math.sqrt(k), seed=seed + 2)
    return [(x, W, 0)], x.double() @ W.double().T


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows", [8, 80, 128, 130])           # 130: beyond the MFMA form's 128 rows, the wave-per-feature fallback
@pytest.mark.parametrize("layout", ["concat", "sum", "only", "proj", "wide"])
def test_av_proj_fwd_against_fp64(layout, rows, dtype):
    F = 10 if rows % 10 == 0 else 8
    for D in (256, 4096, 5120):
        for with_bias in (False, True):
            for with_temporal in (True, False):
                if not with_temporal and dtype != torch.float32:
                    continue                                  # no cast output: the storage type plays no part
                srcs_h, ref = _layout(layout, rows, D, seed=rows + D)
                held = {}
                srcs = []
                for x, W, c0 in srcs_h:
                    Wd = held.setdefault(id(W), dev(W))
                    srcs.append((dev(x), Wd[:, c0:c0 + x.shape[1]]))
                bias = rnd(D, scale=0.05, seed=5) if with_bias else None
                temp = rnd(F, D, seed=6) if with_temporal else None
                raw = torch.full((rows, D), float("nan"), device=DEV)
                tok = torch.full((rows, D), float("nan"), dtype=dtype, device=DEV) if with_temporal else None
                ops.av_proj_fwd(srcs, raw, bias=None if bias is None else dev(bias),
                                temporal=None if temp is None else dev(temp), out_tok=tok)
                if with_bias:
                    ref = ref + bias.double()[None, :]
                what = (layout, rows, D, with_bias, with_temporal)
                e_raw = rel(raw, ref)
                print(what, dtype, f"raw {e_raw:.2e}")
                assert e_raw < VP_F32, what
                if with_temporal:
                    e_tok = rel(tok, ref + temp.double().repeat(rows // F + 1, 1)[:rows])
                    print(what, dtype, f"tok {e_tok:.2e}")
                    assert e_tok < tol(dtype, VP_F32, VP_H16), what


def test_av_proj_fwd_equals_visual_proj_on_one_source():
    """One contiguous 768-wide source is the video-only projection: the grown kernel keeps its fma chain — bitwise equal."""
    B, F, D = 8, 10, 4096
    video, W, temp = dev(rnd(B * F, KV, seed=1)), dev(rnd(D, KV, scale=1 / math.sqrt(KV), seed=2)), dev(rnd(F, D, seed=3))
    raw0, tok0 = torch.empty(B * F, D, device=DEV), torch.empty(B * F, D, dtype=torch.bfloat16, device=DEV)
    raw1, tok1 = torch.empty_like(raw0), torch.empty_like(tok0)
    ops.visual_proj_fwd(video, W, temp, raw0, tok0)
    ops.av_proj_fwd([(video, W)], raw1, temporal=temp, out_tok=tok1)
    assert torch.equal(raw0, raw1) and torch.equal(tok0, tok1)


def test_av_proj_rejects_bad_operands():
    x, W, out = dev(rnd(8, 64)), dev(rnd(16, 64)), torch.empty(8, 16, device=DEV)
    with pytest.raises(ValueError):
        ops.av_proj_fwd([(x, W[:, :32])], out)                # source and weight widths differ
    with pytest.raises(ValueError):
        ops.av_proj_fwd([], out)
    with pytest.raises(RuntimeError):
        ops.av_proj_fwd([(x[:, 1:5], W[:, 1:5])], out)        # not 16-byte aligned: refused before any launch
    with pytest.raises(ValueError):
        ops.av_proj_fwd([(x, W)], out, temporal=dev(rnd(4, 16)))   # temporal without out_tok


@pytest.mark.parametrize("T", [1, 3, 10])
def test_av_cross_attn_against_fp64(T):
    B, F, E = 3, 10, KV
    q, kv = rnd(B * F, E, seed=1), rnd(B * T, 2 * E, seed=2)  # K | V side by side, as the step's fused projection leaves them
    kvd = dev(kv)
    x = torch.full((B * F, E), float("nan"), device=DEV)
    ops.av_cross_attn_fwd(dev(q), kvd[:, :E], kvd[:, E:], x, B, F, T)
    qd, kd, vd = q.double().view(B, F, E), kv[:, :E].double().reshape(B, T, E), kv[:, E:].double().reshape(B, T, E)
    ref = torch.softmax(qd @ kd.transpose(1, 2) / math.sqrt(E), -1) @ vd
    e = rel(x, ref.reshape(B * F, E))
    print("cross attention T =", T, f"{e:.2e}")
    assert e < VP_F32
    if T == 1:                                                # one key: the weights are exactly 1
        assert torch.equal(x.cpu().view(B, F, E), kv[:, E:].view(B, 1, E).expand(B, F, E))


@pytest.mark.parametrize("R,F", [(30, 10), (80, 10), (130, 10)])
def test_av_proj_bwd_into_pitched_gradient(R, F):
    D = 512
    d_tok, d_qav = rnd(R, D, seed=4), rnd(R, D, seed=5)
    v, a = rnd(R, KV, seed=6), rnd(R, KA, seed=7)
    G = (d_tok + d_qav).double()
    # concat: both sources in one call, each into its column range of a (D, 1792) gradient; accumulates: twice -> twice
    dW, dT = torch.ones(D, KV + KA, device=DEV), torch.ones(F, D, device=DEV)
    for _ in range(2):
        ops.av_proj_bwd(dev(d_tok), dev(d_qav), [(dev(v), dW[:, :KV]), (dev(a), dW[:, KV:])], dT)
    assert rel(dW - 1, 2 * (G.T @ torch.cat([v, a], 1).double())) < VP_F32
    assert rel(dT - 1, 2 * d_tok.double().view(R // F, F, D).sum(0)) < VP_F32
    # one source at a non-zero start: the columns before it are not touched
    dW = torch.ones(D, KV + KA, device=DEV)
    for _ in range(2):
        ops.av_proj_bwd(dev(d_tok), None, [(dev(a), dW[:, KV:])], dT)
    assert torch.equal(dW[:, :KV], torch.ones(D, KV, device=DEV))
    assert rel(dW[:, KV:] - 1, 2 * (d_tok.double().T @ a.double())) < VP_F32
    # a source wider than 1024 columns (the two-features-per-wave form), and no trainable source at all (audio_only)
    w = rnd(R, KV + KA, seed=8)
    dW, dT = torch.ones(D, KV + KA, device=DEV), torch.ones(F, D, device=DEV)
    ops.av_proj_bwd(dev(d_tok), dev(d_qav), [(dev(w), dW)], dT)
    assert rel(dW - 1, G.T @ w.double()) < VP_F32
    ops.av_proj_bwd(dev(d_tok), dev(d_qav), [], dT)
    assert rel(dT - 1, 2 * d_tok.double().view(R // F, F, D).sum(0)) < VP_F32


def test_av_proj_bwd_equals_visual_proj_bwd_on_one_source():
    R, F, D = 80, 10, 4096
    d_tok, d_qav, v = dev(rnd(R, D, seed=4)), dev(rnd(R, D, seed=5)), dev(rnd(R, KV, seed=6))
    dW0, dT0 = torch.zeros(D, KV, device=DEV), torch.zeros(F, D, device=DEV)
    dW1, dT1 = torch.zeros_like(dW0), torch.zeros_like(dT0)
    ops.visual_proj_bwd(d_tok, d_qav, v, dW0, dT0)
    ops.av_proj_bwd(d_tok, d_qav, [(v, dW1)], dT1)
    assert torch.equal(dW0, dW1) and torch.equal(dT0, dT1)


# ------------------------------------------------------------------------------ whole step against the reference's goldens
def _step_against_golden(name, dtype, lm_head):
    g, cfg = audio_util.golden_cfg(name)
    model, _ = audio_util.build_model(cfg, dtype)
    batch = synth.make_batch(cfg, seed=0)
    w = FP16_LOSS_SCALE if dtype == torch.float16 else 1.0
    losses, grads, logits, layer_out = audio_util.run_step(model, batch, loss_weights=(w, w, w), lm_head=lm_head)
    grads = {n: x / w for n, x in grads.items()}
    assert all(torch.isfinite(x).all() for x in grads.values())
    peaked = name.endswith("_peaked")
    if dtype == torch.float32:
        kw = dict(rtol=FP32_RTOL, min_decided=0.99)
    elif dtype == torch.bfloat16:
        kw = dict(rtol=BF16_LOSS_RTOL, tol=BF16_TOL, min_decided=0.95)
    else:
        kw = dict(rtol=BF16_LOSS_RTOL, tol=FP16_TOL, min_decided=0.95 if peaked else 0.7)
    if lm_head == "scored":
        kw.update(min_decided=0.0, scored_rows_only=True)     # as tests/test_step_gpu.py's scored-rows test
        sc = model._engine.last_scored
        assert sc is not None and sc.M < cfg.batch_size * cfg.max_seq_len
    rep = compare_with_golden(g, losses, grads, logits, layer_out, **kw)
    print(name, dtype, lm_head, losses, {k: f"{v:.2e}" if isinstance(v, float) else v for k, v in rep.items()})
    if dtype == torch.float32:
        assert rep["loss_vqa"] < 1e-4
    # the golden's gradient records <-> the flat buffer: every parameter the reference trains and reaches has a segment, a
    # `gradnone__` one (never reached: no .grad in the reference) is not written by the step, nothing else is in the buffer
    flat = model.flat_params()
    trained = {str(n) for n, t in zip(g["param_names"], g["param_trainable"]) if t}
    assert set(flat.offsets) == trained
    idle = set(flat.idle_offsets())
    for k in g:
        if k.startswith("gradnone__"):
            n = k[len("gradnone__"):].replace("__", ".")
            assert flat.offsets[n][0] in idle or float(grads[n].abs().max()) == 0.0, n
    model._engine.check_gemm_error()
    _free(model)


@pytest.mark.parametrize("name", audio_util.GOLDENS)
def test_fp32_audio_step_matches_reference_golden(name):
    _step_against_golden(name, torch.float32, "all")


@pytest.mark.parametrize("name", [n for n in audio_util.GOLDENS if "7b_l2" in n])
def test_bf16_audio_step_against_reference_golden(name):
    _step_against_golden(name, torch.bfloat16, "all")


@pytest.mark.parametrize("name", audio_util.GOLDENS)
def test_fp16_audio_step_against_reference_golden(name):
    _step_against_golden(name, torch.float16, "all")


@pytest.mark.parametrize("name,dtype", [("audio_tiny_concat", torch.float32), ("audio_tiny_only", torch.float32),
                                        ("audio_tiny_attnF", torch.float32),
                                        ("audio_7b_l2_b8_concat_peaked", torch.bfloat16),
                                        ("audio_7b_l2_b8_attn1_peaked", torch.float16)])
def test_audio_step_on_the_tail_rows_matches_reference_golden(name, dtype):
    """lm_head_rows = "scored", the product default, in an audio mode."""
    _step_against_golden(name, dtype, "scored")


@pytest.mark.parametrize("lm_head", ["all", "scored"])
def test_audio_native_schedule_equals_python_schedule(lm_head, monkeypatch):
    cfg = synth.preset("tiny", vaq=True, qav=True, audio="concat")
    model, _ = audio_util.build_model(cfg, torch.bfloat16)
    batch = synth.make_batch(cfg, seed=6)
    monkeypatch.delenv("FVQA_PY_SCHEDULE", raising=False)
    l_nat, g_nat, _, lo_nat = audio_util.run_step(model, batch, lm_head=lm_head)
    monkeypatch.setenv("FVQA_PY_SCHEDULE", "1")
    l_py, g_py, _, lo_py = audio_util.run_step(model, batch, lm_head=lm_head)
    assert l_nat == l_py
    for a, b in zip(lo_nat, lo_py):
        assert torch.equal(torch.nan_to_num(a, nan=-7.0), torch.nan_to_num(b, nan=-7.0))
    for n in g_nat:
        assert torch.equal(g_nat[n], g_py[n]), n
    _free(model)


@pytest.mark.parametrize("mode,T", [("only", 0), ("concat", 0), ("sum", 0), ("attention", 1), ("attention", 3)])
def test_audio_step_is_bitwise_repeatable(mode, T):
    """Two runs of the same batch -> bitwise equal losses and gradients in every mode (no float atomics in the front end). The batch
    is handed to the model as it is: the audio-only one has no "video"."""
    cfg = synth.preset("tiny", vaq=True, qav=True, audio=mode, audio_len=T)
    model, _ = audio_util.build_model(cfg, torch.bfloat16)
    batch = synth.make_batch(cfg, seed=4)
    assert ("video" in batch) == (mode != "only") and batch["audio"].shape[1] == (T or cfg.max_feats)
    flat = model.flat_params()
    runs = []
    for _ in range(2):
        flat.zero_grad()
        vqa, vaq, qav = model(batch)
        (vqa + vaq + qav).sum().backward()
        torch.cuda.synchronize()
        runs.append(([float(x.detach()) for x in (vqa, vaq, qav)], flat.flat_grad.clone()))
    assert runs[0][0] == runs[1][0] and all(math.isfinite(x) for x in runs[0][0])
    assert torch.equal(runs[0][1], runs[1][1])
    assert float(flat.grad_view("temporal_emb.weight").abs().max()) > 0
    if mode != "only":
        assert float(flat.grad_view("visual_proj.weight").abs().max()) > 0
    _free(model)


# ------------------------------------------------------------------------------ what each mode launches
FRONT_OPS = ("visual_proj_fwd", "visual_proj_bwd", "av_proj_fwd", "av_cross_attn_fwd", "av_proj_bwd")


def _front_calls(monkeypatch, mode, T=0):
    cfg = synth.preset("tiny", vaq=True, qav=True, audio=mode, audio_len=T)
    model, _ = audio_util.build_model(cfg, torch.float32)
    calls = {n: 0 for n in FRONT_OPS}
    for n in FRONT_OPS:
        real = getattr(ops, n)

        def counted(*a, _n=n, _real=real, **k):
            calls[_n] += 1
            return _real(*a, **k)

        monkeypatch.setattr(ops, n, counted)
    audio_util.run_step(model, synth.make_batch(cfg, seed=0), lm_head="scored")
    _free(model)
    return calls


def test_video_only_step_calls_the_entries_it_did(monkeypatch):
    """With args.audio false the front end is fvqa_visual_proj_fwd / fvqa_visual_proj_bwd, once each, and none of the new entries."""
    assert _front_calls(monkeypatch, "none") == dict(visual_proj_fwd=1, visual_proj_bwd=1, av_proj_fwd=0, av_cross_attn_fwd=0,
                                                     av_proj_bwd=0)


@pytest.mark.parametrize("mode,fwd,attn", [("only", 1, 0), ("concat", 1, 0), ("sum", 1, 0), ("attention", 4, 1)])
def test_audio_modes_launch_one_projection_each(monkeypatch, mode, fwd, attn):
    """No mode's forward front end is more than one launch per projection it really has: one for only / concat / sum; audio_proj,
    Q, K|V, softmax·V, visual_proj for attention. One backward call in every mode."""
    assert _front_calls(monkeypatch, mode, 1 if mode == "attention" else 0) == dict(
        visual_proj_fwd=0, visual_proj_bwd=0, av_proj_fwd=fwd, av_cross_attn_fwd=attn, av_proj_bwd=1)


def test_audio_shape_is_checked_before_any_launch():
    cfg = synth.preset("tiny", audio="concat")
    model, _ = audio_util.build_model(cfg, torch.float32)
    batch = synth.make_batch(cfg, seed=0)
    batch["audio"] = batch["audio"][:, :3]                    # T != max_feats outside `attention`
    with pytest.raises(ValueError):
        model(batch)
    _free(model)
