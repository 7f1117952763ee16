"""Option scoring on the GPU (fvqa/score.py, csrc/score.hip): the suffix attention against the fp64 oracle, the per-option
reduction against torch, `score_options` in both routes against fixtures generated from the reference's own multiple-choice
branch (tools/gen_golden_score.py), and what has to keep working on the same engine afterwards. Run with -m gpu."""
import os
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import engine  # noqa: E402
from fvqa import ops, score, synth  # noqa: E402
from oracle import ref_cpu  # noqa: E402
from tests.test_kernels_gpu import DEV, DTYPES, dev, rel, rnd, tol  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FP32_RTOL = 1e-3                      # the project's fp32 bar against a reference-generated fixture
# The 16-bit pins use score_7b_l2_peakedperm: of the three 7B-width variants tools/gen_golden_score.py makes, the one whose
# recorded gaps between the two lowest option means are largest (min / median over the four samples: random LM head
# 1.7e-4 / 8.4e-4, peaked 4.2e-3 / 4.2e-3, peakedperm 5.1e-3 / 5.2e-3).
PIN = "score_7b_l2_peakedperm"
# Largest relative error of the DENSE route's per-option means against that fixture, measured on an MI355X
# (profiles/score_options.log, "errors" section: bf16 3.4505e-04, fp16 9.5496e-06; the shared route read 3.5845e-04 and
# 9.6728e-06 in the same run), rounded up in the third digit. The dense route is the existing forward, whose kernels the parity
# tests pin; the shared route sums its attention in another order and rounds the suffix keys at another point: it gets twice that.
DENSE_MEAN_ERR = {torch.bfloat16: 3.46e-4, torch.float16: 9.56e-6}


def load(name):
    return dict(np.load(os.path.join(GOLDEN, name + ".npz")))


def golden_batch(g):
    B = g["answer"].shape[0]
    return {"video": torch.from_numpy(g["video"]), "text_id": {"vqa": torch.from_numpy(g["text_id_vqa"])},
            "label": {"vqa": torch.from_numpy(g["label_vqa"])}, "video_start": {"vqa": g["vstart_vqa"].tolist()},
            "prefix_index": {"vqa": g["prefix_vqa"].tolist()}, "answer": torch.from_numpy(g["answer"]),
            "qtype": torch.from_numpy(g["qtype"]), "vid": [f"v{i}" for i in range(B)]}


def fixture_cfg(name, **over):
    perm, peaked = name.endswith("_peakedperm"), name.endswith("_peaked")
    base = name[len("score_"):].replace("_peakedperm", "").replace("_peaked", "")
    return synth.preset(base, vaq=False, qav=False, vocab_size=32000, max_seq_len=128, batch_size=4, peaked=peaked,
                        peaked_perm=perm, **over)


# ------------------------------------------------------------------------------ fvqa_attn_suffix
SUFFIX_CASES = [
    # N, S, H, O, T, vstart, start, len
    (3, 128, 2, 5, 16, [19, -1, 35], [40, 100, 40], [1, 16, 16]),      # len 1 and 16; biased suffix queries; frame keys IN a suffix
    (2, 300, 1, 7, 16, [8, -1], [290, 33], [9, 16]),                   # ten prompt chunks; 112 queries = four query tiles
    (2, 64, 2, 3, 4, [3, 20], [60, 31], [4, 2]),                       # the shipped shape: T = 4, suffix at the end of S
]


def _suffix_case(dtype, cache_rotated, N, S, H, O, T, vstart, start, length, seed):
    A, F = 10, 10
    Dh, D = 128, H * 128
    base = rnd(N * S + A, 3 * D, dtype=dtype, seed=seed)
    g1 = rnd(H, seed=seed + 1).float()
    g2 = rnd(H, seed=seed + 2).float() - 3.0
    cos, sin = ref_cpu.rope_tables(2 * S, Dh, torch.float32)
    c64, s64 = cos[:S].double(), sin[:S].double()
    # the N*O full sequences: option c of sample n = the sample's rows in front of start[n], rows of its own from there on
    full = base[: N * S].view(N, 1, S, 3 * D).repeat(1, O, 1, 1)
    own = rnd(N * O * S, 3 * D, dtype=dtype, seed=seed + 3).view(N, O, S, 3 * D)
    for n in range(N):
        full[n, :, start[n]:] = own[n, :, start[n]:]
    q = full[..., :D].double().reshape(N * O, S, H, Dh)
    k = full[..., D:2 * D].double().reshape(N * O, S, H, Dh)
    v = full[..., 2 * D:].double().reshape(N * O, S, H, Dh)
    ak = base[N * S:, D:2 * D].double().view(A, H, Dh)
    av = base[N * S:, 2 * D:].double().view(A, H, Dh)
    qr, kr = ref_cpu.rope_apply(q, c64, s64), ref_cpu.rope_apply(k, c64, s64)
    vs_all = [vstart[n] for n in range(N) for _ in range(O)]
    o_ref, _ = ref_cpu.attn_fwd(qr, kr, v, ak, av, g1.double(), g2.double(), vs_all, F)
    o_ref = o_ref.reshape(N, O, S, D)
    # the cache: the prompt rows (raw or rotated keys); everything from start[n] on is poison — the kernel must not read it
    cache = base.clone()
    if cache_rotated:
        cache[: N * S, D:2 * D] = kr.reshape(N, O, S, D)[:, 0].reshape(N * S, D).to(dtype)
    for n in range(N):
        cache[n * S + start[n]:(n + 1) * S] = float("nan")
    suf = torch.full((N, O, T, 3 * D), float("nan"), dtype=dtype)           # padding rows: NaN
    want = torch.zeros(N, O, T, D, dtype=torch.float64)
    valid = torch.zeros(N, O, T, dtype=torch.bool)
    for n in range(N):
        L = length[n]
        suf[n, :, :L] = full[n, :, start[n]:start[n] + L]
        want[n, :, :L] = o_ref[n, :, start[n]:start[n] + L]
        valid[n, :, :L] = True
    return dict(suf=suf.reshape(N * O * T, 3 * D), cache=cache, g1=g1, g2=g2, cos=cos, sin=sin, want=want.reshape(-1, D),
                valid=valid.reshape(-1), A=A, F=F, Dh=Dh, D=D)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cache_rotated", [False, True])
@pytest.mark.parametrize("N,S,H,O,T,vstart,start,length", SUFFIX_CASES)
def test_attention_suffix_rows(dtype, cache_rotated, N, S, H, O, T, vstart, start, length):
    """fvqa_attn_suffix: for option c of sample n, suffix row j (position start[n] + j; RAW q, k, v in qkv_suf; keys / values of
    the positions in front of start[n] in the cache, raw or rotated) equals row start[n] + j of the full-sequence oracle on the
    rotated operands (llama/model.py:87-128) run over that option's whole sequence — the decode test's comparison and bounds.
    The cache is bit-identical afterwards, cache rows from start[n] on and the padding rows of qkv_suf are NaN and change no
    valid output, padding output rows are finite, two runs are bitwise equal."""
    c = _suffix_case(dtype, cache_rotated, N, S, H, O, T, vstart, start, length, seed=S + 11)
    cache_d, suf_d = dev(c["cache"]), dev(c["suf"])
    args = (dev(c["g1"]), dev(c["g2"]), dev(torch.tensor(vstart, dtype=torch.int32)),
            dev(torch.tensor(start, dtype=torch.int32)), dev(torch.tensor(length, dtype=torch.int32)),
            (dev(c["cos"]), dev(c["sin"])), N, O, T, S, H, c["Dh"], c["A"], c["F"])
    outs = []
    for _ in range(2):
        o = torch.full((N * O * T, c["D"]), float("nan"), dtype=dtype, device=DEV)
        ops.attn_suffix(suf_d, cache_d, o, *args, cache_rotated=cache_rotated)
        outs.append(o.cpu())
    got = outs[0]
    assert torch.equal(outs[0].view(torch.uint8), outs[1].view(torch.uint8))             # bitwise repeatable
    assert bool(torch.isfinite(got.float()).all())                                       # padding rows included
    err = rel(got[c["valid"]], c["want"][c["valid"]])
    print(f"attn_suffix {dtype} rot={cache_rotated} N={N} S={S} O={O} T={T}: rel err {err:.3e}")
    assert err < tol(dtype, 3e-5, 1e-2)
    back = cache_d.cpu()
    assert torch.equal(back.view(torch.uint8), c["cache"].view(torch.uint8))             # the cache did not move (NaNs included)
    # the padding rows hold anything: other values there, same valid output
    suf2 = c["suf"].clone()
    suf2[torch.isnan(suf2)] = 7.0
    o2 = torch.empty_like(outs[0], device=DEV)
    ops.attn_suffix(dev(suf2), cache_d, o2, *args, cache_rotated=cache_rotated)
    assert torch.equal(o2.cpu()[c["valid"]], got[c["valid"]])


def test_attention_suffix_rejects_bad_shapes():
    c = _suffix_case(torch.float32, True, 1, 32, 1, 2, 4, [3], [20], [4], seed=5)
    i32 = lambda x: dev(torch.tensor(x, dtype=torch.int32))                               # noqa: E731
    o = torch.empty(8, c["D"], device=DEV)
    a = (dev(c["g1"]), dev(c["g2"]), i32([3]), i32([20]), i32([4]), (dev(c["cos"]), dev(c["sin"])))
    with pytest.raises(ValueError):                                                       # 17 suffix rows
        ops.attn_suffix(dev(c["suf"]), dev(c["cache"]), o, *a, 1, 2, 17, 32, 1, 128, 10, 10, cache_rotated=True)
    with pytest.raises(ValueError):                                                       # o of the wrong row count
        ops.attn_suffix(dev(c["suf"]), dev(c["cache"]), o[:4], *a, 1, 2, 4, 32, 1, 128, 10, 10, cache_rotated=True)
    with pytest.raises(ValueError):                                                       # start as int64
        ops.attn_suffix(dev(c["suf"]), dev(c["cache"]), o, a[0], a[1], a[2], dev(torch.tensor([20])), a[4], a[5],
                        1, 2, 4, 32, 1, 128, 10, 10, cache_rotated=True)


# ------------------------------------------------------------------------------ fvqa_option_pick
def _pick_case():
    """B = 4, O = 3, S = 9. Sample 0: plain; 1: option 1 all ignored (NaN mean -> picked, as torch); 2: options 0 and 2 tie
    exactly (-> 0); 3: a scored row whose loss is exactly 0 (not counted)."""
    B, O, S = 4, 3, 9
    il = torch.zeros(B, O, S - 1)
    il[0, 0, 3:6] = torch.tensor([2.0, 1.5, 0.25]); il[0, 1, 3:5] = torch.tensor([0.5, 0.75]); il[0, 2, 3:7] = 1.0
    il[1, 0, 2:4] = 1.0; il[1, 2, 2:4] = 0.5
    il[2, 0, 4:6] = torch.tensor([1.0, 3.0]); il[2, 1, 4:6] = 2.5; il[2, 2, 4:8] = 2.0
    il[3, 0, 1:4] = torch.tensor([3.0, 0.0, 3.0]); il[3, 1, 1:4] = torch.tensor([2.5, 2.5, 2.5]); il[3, 2, 1:3] = 4.0
    scored = il != 0
    scored[3, 0, 2] = True                                   # the exact-zero loss IS a scored row
    n, c, t = torch.nonzero(scored, as_tuple=True)
    perm = torch.randperm(n.numel(), generator=torch.Generator().manual_seed(3))          # compact rows in any order
    n, c, t = n[perm], c[perm], t[perm]
    rowloss = torch.cat([il[n, c, t], torch.tensor([9.0, 9.0])])                          # two pad rows behind
    row_map = torch.cat([((n * O + c) * (S - 1) + t), torch.tensor([-1, -1])]).to(torch.int32)
    return il, rowloss, row_map, B, O, S


def test_option_pick_matches_torch():
    il, rowloss, row_map, B, O, S = _pick_case()
    count = (il != 0).sum(-1)                                # reference engine.py:88
    mean = il.sum(-1) / count
    want = mean.argmin(-1)                                   # engine.py:93
    assert want.tolist() == [1, 1, 0, 1] and bool(torch.isnan(mean[1, 1])) and count[3, 0] == 2
    assert torch.argmin(torch.tensor([1.0, float("nan"), 0.5])) == 1                      # torch's rule, as the header states it
    outs = []
    for _ in range(2):
        got = ops.option_pick(dev(rowloss), dev(row_map), rowloss.numel(), B, O, S)
        outs.append([x.cpu() for x in got])
    g_il, g_sum, g_cnt, g_mean, g_pred = outs[0]
    assert torch.equal(g_il, il) and g_cnt.dtype == torch.int64 and torch.equal(g_cnt, count)
    assert torch.equal(g_sum, il.sum(-1)) and torch.equal(torch.nan_to_num(g_mean, nan=-1.0), torch.nan_to_num(mean, nan=-1.0))
    assert g_pred.dtype == torch.int64 and torch.equal(g_pred, want)
    for a, b in zip(outs[0], outs[1]):
        assert torch.equal(torch.nan_to_num(a.float(), nan=-1.0), torch.nan_to_num(b.float(), nan=-1.0))
    # n_rows stops the scan: with the last scored row left out its entry stays zero
    short = ops.option_pick(dev(rowloss), dev(row_map), rowloss.numel() - 3, B, O, S)[0].cpu()
    assert int((short != il).sum()) == 1


# ------------------------------------------------------------------------------ score_options against the reference's fixtures
def run_route(model, batch, route, monkeypatch):
    monkeypatch.setenv("FVQA_SCORE", route)
    il = model.score_options(batch)
    last = model.last_scoring
    assert last["route"] == route and set(last) == {"prediction", "mean", "count", "route"}
    assert il.is_cuda and il.dtype == torch.float32 and last["prediction"].is_cuda
    return il.cpu().numpy(), last["mean"].cpu().numpy(), last["count"].cpu().numpy(), last["prediction"].cpu().numpy()


@pytest.mark.parametrize("name", ["score_tiny", "score_7b_l2"])
def test_fp32_scores_match_the_reference(name, monkeypatch):
    """fp32 build, tiny width and 7B width: both routes give the reference's individual_losses within FP32_RTOL of its largest
    entry, zeros exactly where it has zeros, equal counts and predictions (every sample's gap is > 1e-4, tests/test_score_cpu.py)."""
    from tests.gpu_util import build_model
    g = load(name)
    model, _ = build_model(fixture_cfg(name), torch.float32)
    model.eval()
    batch = golden_batch(g)
    ref = g["individual_losses"]
    for route in ("shared", "dense"):
        il, mean, count, pred = run_route(model, batch, route, monkeypatch)
        err = float(np.abs(il - ref).max() / np.abs(ref).max())
        print(f"{name} fp32 {route}: individual_losses rel err {err:.3e}")
        assert il.shape == ref.shape and err <= FP32_RTOL
        assert np.array_equal(il == 0, ref == 0)
        assert np.array_equal(count, g["count"]) and np.array_equal(pred, g["prediction"])
        assert np.allclose(mean, g["mean"], rtol=FP32_RTOL)


def mean_err(mean, g):
    return float((np.abs(mean - g["mean"]) / np.abs(g["mean"])).max())


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_16bit_scores_are_pinned(dtype, monkeypatch):
    """bf16 / fp16 builds on the 7B-width fixture with the largest gaps (PIN). Per-option means: the dense route within the
    error measured for it (DENSE_MEAN_ERR: the kernels are deterministic), the shared route within twice that.
    Predictions equal the fixture's on every DECIDED sample — gap > 8 x the measured error, the rule of tests/parity.py."""
    from tests.gpu_util import build_model
    g = load(PIN)
    bound = DENSE_MEAN_ERR[dtype]
    assert bound > 0, "measure the dense route first (tools/score_bench.py --errors)"
    decided = g["gap"] > 8 * bound
    assert decided.sum() * 2 >= decided.size, f"only {int(decided.sum())} of {decided.size} samples decided under {8 * bound:.2e}"
    model, _ = build_model(fixture_cfg(PIN), dtype)
    model.eval()
    batch = golden_batch(g)
    for route, limit in (("dense", bound), ("shared", 2 * bound)):
        il, mean, count, pred = run_route(model, batch, route, monkeypatch)
        err = mean_err(mean, g)
        print(f"{PIN} {dtype} {route}: per-option mean rel err {err:.3e} (limit {limit:.3e})")
        assert err <= limit
        assert np.array_equal(il == 0, g["individual_losses"] == 0) and np.array_equal(count, g["count"])
        assert np.array_equal(pred[decided], g["prediction"][decided])


def test_val_one_epoch_scores_the_references_accuracy(monkeypatch):
    """engine.val_one_epoch without --is_generation_task driving the real model (fp32 build, 7B width) over the reference's
    validation batch: accuracy and meters are those of the reference's own predictions."""
    from tests.gpu_util import build_model
    monkeypatch.delenv("FVQA_SCORE", raising=False)
    g = load("score_7b_l2")
    model, _ = build_model(fixture_cfg("score_7b_l2"), torch.float32)
    opt = types.SimpleNamespace(param_groups=[{"lr": 0.25}])
    args = types.SimpleNamespace(is_generation_task=False, dataset="nextqa", debug=False, output_dir=None)
    stats = engine.val_one_epoch(model, [golden_batch(g), golden_batch(g)], opt, epoch=1, args=args)
    want = float((g["prediction"] == g["answer"]).mean())
    assert stats["acc"] == pytest.approx(want) and stats["Total"] == pytest.approx(want) and stats["lr"] == 0.25
    assert model.last_scoring["route"] == score.DEFAULT_ROUTE


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_training_and_generation_survive_scoring(dtype, monkeypatch):
    """Scoring runs in arenas of its own and puts the engine's configuration back: a training step taken after both routes
    equals the step taken before them bit for bit (loss and every gradient), and generation still reproduces eval_tiny."""
    from tests.gpu_util import build_model, run_step
    from tests.test_eval import GOLDS, golden_batch as eval_batch
    cfg = synth.preset("tiny", vaq=True, qav=True, vocab_size=32000, max_seq_len=128, batch_size=4)
    model, _ = build_model(cfg, dtype)
    tb = synth.make_batch(cfg, seed=0)
    l1, g1, _, _ = run_step(model, tb, lm_head="scored")
    assert all(np.isfinite(v) for v in l1.values())
    g = load("score_tiny")
    for route in ("shared", "dense"):
        run_route(model, golden_batch(g), route, monkeypatch)
    eng = model._engine
    assert eng.tasks == ["vqa", "vaq", "qav"] and eng.n_streams == 3 and eng.lm_head_rows == "scored"
    l2, g2, _, _ = run_step(model, tb, lm_head="scored")
    assert l1 == l2 and set(g1) == set(g2)
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k
    if dtype == torch.float32:
        E = GOLDS["tiny"]
        model.eval()
        best, _ = model(eval_batch(E), inference=True)
        assert np.array_equal(model.last_generation["ids"].cpu().numpy(), E["ids_after"])
        assert np.array_equal(best.cpu().numpy(), E["best"])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_audio_concat_routes_agree(dtype, monkeypatch):
    """An audio mode (`concat`: two sources against one 1792-wide projection): both routes run — the shared one calls the front
    end once per batch, the dense one on inputs repeated per option — and agree within the bounds above."""
    from tests.audio_util import build_model
    cfg = synth.preset("7b_l2", vaq=False, qav=False, batch_size=3, audio="concat", peaked_perm=True)   # (PIN's weights)
    model, _ = build_model(cfg, dtype)
    model.eval()
    batch = synth.make_option_batch(cfg, n_options=5, seed=2)
    out = {r: run_route(model, batch, r, monkeypatch) for r in ("shared", "dense")}
    (il_s, mean_s, cnt_s, _), (il_d, mean_d, cnt_d, _) = out["shared"], out["dense"]
    assert np.array_equal(cnt_s, cnt_d) and np.array_equal(il_s == 0, il_d == 0) and int(cnt_s.min()) >= 3
    assert np.isfinite(mean_s).all() and np.isfinite(mean_d).all()
    err = float((np.abs(mean_s - mean_d) / np.abs(mean_d)).max())
    print(f"audio concat {dtype}: shared vs dense per-option mean rel err {err:.3e}")
    assert err <= (FP32_RTOL if dtype == torch.float32 else 3 * DENSE_MEAN_ERR[dtype])
