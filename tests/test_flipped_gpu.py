"""Option scoring by all three flipped tasks on the GPU (fvqa/flipped.py, csrc/flipped.hip): the wide suffix attention per row
and head against fp64, the suffix inputs bit for bit, the pick against the numpy rule, and `score_flipped` in both routes against
fixtures generated from the reference's training forward (tools/gen_golden_flipped.py). Run with -m gpu."""
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import engine  # noqa: E402
from fvqa import _lib, flipped, ops, synth  # noqa: E402
from tests import cached_attn_util as U  # noqa: E402
from tests import flipped_util as FU  # noqa: E402
from tests.test_flipped_cpu import pick_case  # noqa: E402
from tests.test_kernels_gpu import DEV, DTYPES, dev  # noqa: E402

FP32_RTOL = 1e-3                      # the project's fp32 bar against a reference-generated fixture
PIN = "flipped_7b_l2_peakedperm"
# Largest relative error of the DENSE route's per-option means against PIN, per task, measured on an MI355X
# (profiles/score_flipped.log, "errors" section), rounded up in the third digit; the shared route — another summation order in
# its attention, suffix keys rounded at another point — gets twice that: the rule tests/test_score_gpu.py states for
# DENSE_MEAN_ERR.
DENSE_MEAN_ERR = {
    torch.bfloat16: {"vqa": 2.20e-4, "vaq": 1.70e-4, "qav": 1.63e-4},      # measured 2.1968e-04, 1.6989e-04, 1.6250e-04
    torch.float16: {"vqa": 1.52e-5, "vaq": 8.76e-6, "qav": 3.41e-5},       # measured 1.5127e-05, 8.7569e-06, 3.4006e-05
}


# ------------------------------------------------------------------------------ fvqa_attn_suffix_wide
def launch_wide(c, dtype, cache_rotated, entry="attn_suffix_wide", suf=None):
    """One launch on the operands of a flipped_util.wide_case -> o (rows, D) on the host. A = 0 goes to the library directly
    (ops' shared attention check wants an adapter row)."""
    N, S, H, O, T, A, Fw, D = c["N"], c["S"], c["H"], c["O"], c["T"], c["A"], c["F"], c["D"]
    suf_d, cache_d = dev(c["suf"] if suf is None else suf), dev(c["cache"])
    o = torch.full((N * O * T, D), float("nan"), dtype=dtype, device=DEV)
    g1, g2, vs, st, ln, cos, sin = (dev(c[k]) for k in ("g1", "g2", "vstart", "start", "length", "cos", "sin"))
    if A == 0:
        rc = _lib.load(dtype).fvqa_attn_suffix_wide(
            suf_d.data_ptr(), cache_d.data_ptr(), o.data_ptr(), g1.data_ptr(), g2.data_ptr(), vs.data_ptr(), st.data_ptr(),
            ln.data_ptr(), cos.data_ptr(), sin.data_ptr(), N, O, T, S, H, U.DH, 0, Fw, 1 if cache_rotated else 0,
            ops.dt_code(dtype), torch.cuda.current_stream().cuda_stream)
        assert rc == 0
    else:
        getattr(ops, entry)(suf_d, cache_d, o, g1, g2, vs, st, ln, (cos, sin), N, O, T, S, H, U.DH, A, Fw,
                            cache_rotated=cache_rotated)
    back = cache_d.cpu()
    assert torch.equal(U.bits(back), U.bits(c["cache"]))                                  # the cache did not move (NaNs included)
    return o.cpu()


def worst(got, c):
    v = c["valid"]
    if not bool(v.any()):
        return 0.0
    assert U.ref_floor(c["want"][v]) >= U.FLOOR
    return float(U.row_figures(got[v], c["want"][v]).max())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("cache_rotated", [False, True])
@pytest.mark.parametrize("T", FU.WIDE_T)
def test_wide_attention_rows(dtype, cache_rotated, T):
    """fvqa_attn_suffix_wide at H = 2, B = 2, S = 96 over flipped_util.wide_schedule(T): every (row, head) vector within
    cached_attn_util.BOUND of the fp64 reference (the full-sequence oracle's rows; the restatement where A = 0). The padding rows
    of qkv_suf and the cache rows from start[n] on are NaN and reach nothing; padding output rows are zeros; two launches are
    bitwise equal; at T <= 16 fvqa_attn_suffix agrees within the same bound."""
    bound = U.BOUND[dtype]
    for i, (O, st, ln, A, Fw, vs) in enumerate(FU.wide_schedule(T)):
        c = FU.wide_case(dtype, cache_rotated, T, O, st, ln, A, Fw, vs, seed=100 + 7 * T + i)
        got = launch_wide(c, dtype, cache_rotated)
        assert torch.equal(U.bits(got), U.bits(launch_wide(c, dtype, cache_rotated)))      # bitwise repeatable
        assert bool(torch.isfinite(got.float()).all()) and not bool(got[~c["valid"]].float().any())
        w = worst(got, c)
        print(f"attn_suffix_wide {dtype} rot={cache_rotated} T={T} O={O} start={st} len={ln} A={A} F={Fw} vs={vs}: worst row {w:.3e}")
        assert w <= bound
        suf2 = c["suf"].clone()
        suf2[torch.isnan(suf2)] = 7.0                        # the padding rows hold anything: same output bits
        assert torch.equal(U.bits(launch_wide(c, dtype, cache_rotated, suf=suf2)), U.bits(got))
        if T <= 16 and A:
            old = launch_wide(c, dtype, cache_rotated, entry="attn_suffix")
            assert worst(old, c) <= bound
            v = c["valid"]
            if bool(v.any()):
                assert float(U.row_figures(got[v], old[v].double()).max()) <= bound


@pytest.mark.parametrize("dtype", DTYPES)
def test_wide_attention_check_sees_planted_defects(dtype):
    """The comparison above can see errors: against a restatement with ONE planted defect — the causal edge off by one, option c
    reading option c - 1's suffix keys, gate2 dropped for a window inside the suffix — the kernel's rows miss the bound, on cases
    of the same schedule; against the clean restatement they hold it."""
    bound = U.BOUND[dtype]
    seen = set()
    for T in (17, 64):
        for i, (O, st, ln, A, Fw, vs) in enumerate(FU.wide_schedule(T)):
            if A == 0:
                continue
            c = FU.wide_case(dtype, True, T, O, st, ln, A, Fw, vs, seed=100 + 7 * T + i)
            got, v = launch_wide(c, dtype, True), c["valid"]
            assert float(U.row_figures(got[v], FU.wide_restated(c, dtype, True)[v]).max()) <= bound
            for d in ("causal", "option", "gate2"):
                bad = FU.wide_restated(c, dtype, True, defect=d)
                if float((bad[v] - c["want"][v]).abs().max()) > 0.05:          # the defect applies to this case
                    assert float(U.row_figures(got[v], bad[v]).max()) > bound, (d, T, i)
                    seen.add(d)
    assert seen == {"causal", "option", "gate2"}


def test_wide_attention_rejects_bad_shapes():
    c = FU.wide_case(torch.float32, True, 17, 3, [31, 33], [17, 16], 10, 10, [-1, 20], seed=3)
    a = [dev(c[k]) for k in ("g1", "g2", "vstart", "start", "length")] + [(dev(c["cos"]), dev(c["sin"]))]
    suf, cache = dev(c["suf"]), dev(c["cache"])
    o = torch.empty(2 * 3 * 17, c["D"], device=DEV)
    with pytest.raises(ValueError):                                                       # 65 suffix rows
        ops.attn_suffix_wide(suf, cache, o, *a, 2, 3, 65, 96, 2, 128, 10, 10, cache_rotated=True)
    with pytest.raises(ValueError):                                                       # o of the wrong row count
        ops.attn_suffix_wide(suf, cache, o[:8], *a, 2, 3, 17, 96, 2, 128, 10, 10, cache_rotated=True)
    with pytest.raises(ValueError):                                                       # start as int64
        ops.attn_suffix_wide(suf, cache, o, a[0], a[1], a[2], a[3].long(), a[4], a[5], 2, 3, 17, 96, 2, 128, 10, 10,
                             cache_rotated=True)


# ------------------------------------------------------------------------------ fvqa_suffix_embed
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T", [1, 5])
def test_suffix_embed_bit_for_bit(dtype, T):
    B, O, D, V, Fw = 3, 2, 256, 50, 4
    g = torch.Generator().manual_seed(T)
    emb = torch.randn(V, D, generator=g).to(dtype)
    vf = torch.randn(B, Fw, D, generator=g).to(dtype)
    ids = torch.randint(0, V, (B, O, T), generator=g)
    slot = torch.randint(-1, Fw, (B, O, T), generator=g).to(torch.int32)
    length = torch.tensor([T, 0, max(T - 2, 1)], dtype=torch.int32)
    live = torch.arange(T)[None, None, :] < length[:, None, None]
    want = emb[ids]
    fr = vf[torch.arange(B)[:, None, None], slot.clamp(min=0).long()]
    want = torch.where((slot >= 0)[..., None], fr, want)
    want = torch.where(live[..., None].expand_as(want), want, torch.zeros_like(want)).reshape(-1, D)
    x = torch.full((B * O * T, D), float("nan"), dtype=dtype, device=DEV)
    ops.suffix_embed(dev(ids.reshape(-1)), dev(slot.reshape(-1)), dev(emb), dev(vf), dev(length), x, B, O, T, Fw)
    assert torch.equal(U.bits(x.cpu()), U.bits(want))
    # without a slot map: token rows and padding only
    want = torch.where(live[..., None].expand(B, O, T, D), emb[ids], torch.zeros(B, O, T, D, dtype=dtype)).reshape(-1, D)
    ops.suffix_embed(dev(ids.reshape(-1)), None, dev(emb), None, dev(length), x, B, O, T, 0)
    assert torch.equal(U.bits(x.cpu()), U.bits(want))
    with pytest.raises(ValueError):
        ops.suffix_embed(dev(ids.reshape(-1)), dev(slot.reshape(-1).long()), dev(emb), dev(vf), dev(length), x, B, O, T, Fw)
    with pytest.raises(ValueError):
        ops.suffix_embed(dev(ids.reshape(-1)), None, dev(emb), None, dev(length), x[:-1], B, O, T, 0)


# ------------------------------------------------------------------------------ fvqa_flipped_pick
def run_pick(m, c, w, ans):
    out = ops.flipped_pick({t: dev(torch.from_numpy(v)) for t, v in m.items()}, {t: dev(torch.from_numpy(v)) for t, v in c.items()},
                           w, None if ans is None else dev(torch.from_numpy(ans)))
    return [None if x is None else x.cpu().numpy() for x in out]


def same(a, b):
    return a.shape == b.shape and np.array_equal(np.nan_to_num(a, nan=-7.0), np.nan_to_num(b, nan=-7.0))


def test_flipped_pick_matches_the_numpy_rule():
    """Against fvqa.flipped.pick_rule, bit for bit in the total: ties, a NaN, no eligible option, an option one task did not
    score; a zero and a negative weight; two tasks; answer absent; O = 1 and O = 64."""
    m, c, ans = pick_case()
    cases = [(m, c, (1.0, 1.0, 1.0), ans), (m, c, (0.0, 1.0, 0.0), ans), (m, c, (1.0, -1.0, 0.3), None),
             ({t: m[t] for t in ("vqa", "qav")}, {t: c[t] for t in ("vqa", "qav")}, (1.0, 5.0, 2.0), ans),
             ({"vaq": m["vaq"]}, {"vaq": c["vaq"]}, (1.0, 0.7, 1.0), None)]
    rng = np.random.default_rng(5)
    for O in (1, 64):
        mm = {t: rng.random((7, O), dtype=np.float32).round(1) for t in flipped.TASKS}     # one decimal: ties happen
        cc = {t: rng.integers(0, 3, (7, O)).astype(np.int64) for t in flipped.TASKS}
        mm["qav"][2, O // 2] = np.nan
        cases.append((mm, cc, (1.0, 0.37, 2.5), rng.integers(0, O, 7).astype(np.int64)))
    for mm, cc, w, a in cases:
        want = flipped.pick_rule(mm, cc, w, a)
        got = run_pick(mm, cc, w, a)
        assert same(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
        assert (got[3] is None and want[3] is None) or same(got[3], want[3])
        assert all(same(x, y) for x, y in zip(run_pick(mm, cc, w, a)[:3], got[:3]))        # repeatable


# ------------------------------------------------------------------------------ score_flipped against the reference's fixtures
def run(model, batch, route, monkeypatch, **kw):
    """route None: the defaults; "shared" / "dense" through FVQA_SCORE — a stream the planner turns down goes dense."""
    if route is None:
        monkeypatch.delenv("FVQA_SCORE", raising=False)
    else:
        monkeypatch.setenv("FVQA_SCORE", route)
    r = model.score_flipped(batch, **kw)
    assert r is model.last_scoring and r["total"].is_cuda and r["prediction"].dtype == torch.int64
    return r


def np_of(r, key):
    return {t: r[f"{key}_{t}"].cpu().numpy() for t in flipped.TASKS if f"{key}_{t}" in r}


def check_pick(r, answer=None):
    """prediction / prediction_t / total / gold_loss are the rule applied to the returned means and counts."""
    mean, count = np_of(r, "mean"), np_of(r, "count")
    total, pred, pred_t, gold = flipped.pick_rule(mean, count, (1.0, 1.0, 1.0), answer)
    assert same(r["total"].cpu().numpy(), total) and np.array_equal(r["prediction"].cpu().numpy(), pred)
    for t in mean:
        assert np.array_equal(r[f"prediction_{t}"].cpu().numpy(), pred_t[flipped.TASKS.index(t)])
    if answer is not None:
        assert same(r["gold_loss"].cpu().numpy(), gold)


def mean_errs(r, g, samples=None):
    idx = slice(None) if samples is None else list(samples)
    return {t: float((np.abs(m - g[f"mean_{t}"][idx]) / np.abs(g[f"mean_{t}"][idx])).max()) for t, m in np_of(r, "mean").items()}


def decided_match(r, g, bound, samples=None):
    """Predictions equal the fixture's wherever its recorded gap exceeds four times the bound on the means."""
    idx = np.arange(g["answer"].shape[0]) if samples is None else np.array(list(samples))
    for t in flipped.TASKS + ("total",):
        ref = (sum(g[f"mean_{k}"] for k in flipped.TASKS) if t == "total" else g[f"mean_{t}"])[idx].argmin(-1)
        got = r["prediction" if t == "total" else f"prediction_{t}"].cpu().numpy()
        b = max(bound.values()) if t == "total" else bound[t]
        ok = g[f"gap_{t}"][idx] > 4 * b
        assert np.array_equal(got[ok], ref[ok]), (t, got, ref, ok)


@pytest.mark.parametrize("name", FU.FIXTURES)
def test_fp32_means_match_the_reference(name, monkeypatch):
    """fp32 build, tiny width (letter options and free-text options) and 7B width: per-option means of all three tasks within
    FP32_RTOL of the reference's training forward, equal counts, on both routes. The whole batch holds a VAQ suffix above 64 rows:
    its VAQ stream goes dense whatever is asked (asserted); the first three samples alone take the shared form. The vqa entries
    are score_options' own bits."""
    from tests.gpu_util import build_model
    g = FU.load(name)
    model, _ = build_model(FU.fixture_cfg(name), torch.float32)
    model.eval()
    bound = {t: FP32_RTOL for t in flipped.TASKS}
    for samples in (None, (0, 1, 2)):
        batch = FU.golden_batch(g, samples)
        ans = batch["answer"].numpy()
        for route in ("dense", "shared"):
            r = run(model, batch, route, monkeypatch, answer=batch["answer"])
            gen = name.endswith("_gen")
            want_vaq = "dense" if route == "dense" or (samples is None and not gen) else "shared"
            if not gen:
                assert r["route"] == {"vqa": route, "vaq": want_vaq, "qav": route}, r["route"]
            errs = mean_errs(r, g, samples)
            print(f"{name} fp32 {route} samples={samples} routes={r['route']}: mean rel err {errs}")
            assert all(e <= FP32_RTOL for e in errs.values())
            idx = slice(None) if samples is None else list(samples)
            for t, cnt in np_of(r, "count").items():
                assert np.array_equal(cnt, g[f"count_{t}"][idx])
            check_pick(r, ans)
            decided_match(r, g, bound, samples)
            monkeypatch.setenv("FVQA_SCORE", route)
            model.score_options(batch)
            for k in ("mean", "count"):
                assert torch.equal(U.bits(r[f"{k}_vqa"].cpu()), U.bits(model.last_scoring[k].cpu()))
    # a subset of the tasks, and a forced route the planner turned down
    batch = FU.golden_batch(g)
    r = run(model, batch, None, monkeypatch, tasks=("qav", "vqa"))
    assert set(r["route"]) == {"vqa", "qav"} and "mean_vaq" not in r and "gold_loss" not in r
    assert r["route"]["qav"] == flipped.DEFAULT_ROUTE["qav"]
    if not name.endswith("_gen"):
        with pytest.raises(ValueError):
            model.score_flipped(batch, route="shared")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_16bit_means_are_pinned(dtype, monkeypatch):
    """bf16 / fp16 builds on the 7B-width fixture: per task, the dense route within the error measured for it (DENSE_MEAN_ERR),
    the shared route (the first three samples: the fourth's VAQ suffix is too long) within twice that. Predictions equal the
    fixture's wherever its gap exceeds four times the bound."""
    from tests.gpu_util import build_model
    g = FU.load(PIN)
    bound = DENSE_MEAN_ERR[dtype]
    assert all(b > 0 for b in bound.values()), "measure the dense route first (tools/flipped_bench.py --errors)"
    assert int((g["gap_vqa"] > 4 * bound["vqa"]).sum()) >= 3
    model, _ = build_model(FU.fixture_cfg(PIN), dtype)
    model.eval()
    for route, samples, k in (("dense", None, 1), ("shared", (0, 1, 2), 2)):
        batch = FU.golden_batch(g, samples)
        r = run(model, batch, route, monkeypatch, answer=batch["answer"])
        assert set(r["route"].values()) == {route}
        errs = mean_errs(r, g, samples)
        print(f"{PIN} {dtype} {route}: per-option mean rel err {errs} (limits {k} x {bound})")
        assert all(errs[t] <= k * bound[t] for t in errs)
        check_pick(r, batch["answer"].numpy())
        decided_match(r, g, {t: k * b for t, b in bound.items()}, samples)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_audio_sum_routes_agree(dtype, monkeypatch):
    """An audio mode (`sum`, tiny width, no fixture) on synthetic options of different lengths: the two routes agree within the
    shared route's bound."""
    from tests.audio_util import build_model
    cfg = synth.preset("tiny", vaq=True, qav=True, vocab_size=32000, max_seq_len=128, batch_size=3, audio="sum")
    model, _ = build_model(cfg, dtype)
    model.eval()
    batch = synth.make_flipped_option_batch(cfg, n_options=5, seed=2)
    out = {route: run(model, batch, route, monkeypatch) for route in ("shared", "dense")}
    assert set(out["shared"]["route"].values()) == {"shared"} and set(out["dense"]["route"].values()) == {"dense"}
    for t in flipped.TASKS:
        s, d = out["shared"][f"mean_{t}"].cpu().numpy(), out["dense"][f"mean_{t}"].cpu().numpy()
        assert np.isfinite(s).all() and np.isfinite(d).all()
        assert torch.equal(out["shared"][f"count_{t}"].cpu(), out["dense"][f"count_{t}"].cpu())
        err = float((np.abs(s - d) / np.abs(d)).max())
        print(f"audio sum {dtype} {t}: shared vs dense per-option mean rel err {err:.3e}")
        assert err <= (FP32_RTOL if dtype == torch.float32 else 2 * DENSE_MEAN_ERR[dtype][t])
    check_pick(out["shared"])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_training_survives_flipped_scoring(dtype, monkeypatch):
    """score_flipped runs single streams in the scoring arenas and puts the engine's configuration back: a training step taken
    after both routes equals the step taken before them bit for bit (loss and every gradient)."""
    from tests.gpu_util import build_model, run_step
    cfg = synth.preset("tiny", vaq=True, qav=True, vocab_size=32000, max_seq_len=FU.S_FIX, batch_size=4)
    model, _ = build_model(cfg, dtype)
    tb = synth.make_batch(cfg, seed=0)
    l1, g1, _, _ = run_step(model, tb, lm_head="scored")
    assert all(np.isfinite(v) for v in l1.values())
    g = FU.load("flipped_tiny")
    for route in ("shared", "dense"):
        run(model, FU.golden_batch(g, (0, 1, 2)), route, monkeypatch)
    eng = model._engine
    assert eng.tasks == ["vqa", "vaq", "qav"] and eng.n_streams == 3 and eng.lm_head_rows == "scored"
    l2, g2, _, _ = run_step(model, tb, lm_head="scored")
    assert l1 == l2 and set(g1) == set(g2)
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k


def test_val_one_epoch_flipped_logs_the_six_meters(monkeypatch):
    """engine.val_one_epoch under --val_flipped driving the real model over synthetic option batches: acc, acc_vqa, acc_vaq,
    acc_qav, vaq_loss and qav_loss are logged, the losses are those of the gold options."""
    from tests.gpu_util import build_model
    monkeypatch.delenv("FVQA_SCORE", raising=False)
    cfg = synth.preset("tiny", vaq=True, qav=True, vocab_size=32000, max_seq_len=128, batch_size=4)
    model, _ = build_model(cfg, torch.float32)
    batches = [synth.make_flipped_option_batch(cfg, 5, seed=s) for s in (1, 2)]
    opt = types.SimpleNamespace(param_groups=[{"lr": 0.25}])
    args = types.SimpleNamespace(is_generation_task=False, dataset="nextqa", debug=False, output_dir=None, val_flipped=True,
                                 val_flipped_weights=None)
    stats = engine.val_one_epoch(model, batches, opt, epoch=1, args=args)
    assert {"acc", "acc_vqa", "acc_vaq", "acc_qav", "vaq_loss", "qav_loss", "Total", "lr"} <= set(stats)
    want = {"acc": [], "vaq_loss": [], "qav_loss": []}
    for b in batches:
        r = model.score_flipped(b, answer=b["answer"])
        want["acc"].append(float((r["prediction"].cpu() == b["answer"]).float().mean()))
        want["vaq_loss"].append(float(r["gold_loss"][:, 1].mean()))
        want["qav_loss"].append(float(r["gold_loss"][:, 2].mean()))
    for k, v in want.items():
        assert stats[k] == pytest.approx(sum(v) / len(v), rel=1e-6), k
    assert np.isfinite([stats["vaq_loss"], stats["qav_loss"]]).all()
