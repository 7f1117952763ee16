"""The helpers of tests/test_attn_edges_gpu.py (tests/attn_edges_util.py), checked without a GPU: the formulas with hooks are the
oracle's, the per-row measure stays finite on exactly-zero rows, every planted key carries its row, every half plant has a weight
near one half, every decoy is invisible to the reference — and a reference corrupted the way a kernel would be (the pair dropped,
the decoy leaked, the frame window shifted by one, the bias omitted) is off by at least ten times the 16-bit bound on the rows
that corruption targets and by exactly nothing on the rows it cannot reach. Every case's operands are finite in fp16."""
import math

import pytest
import torch

from oracle import ref_cpu
from tests import attn_edges_util as U

DTYPES = U.DTYPES
SEE_O = 10 * U.BOUND_O[U.BF16]          # what a corruption must move a targeted row by
SEE_G = 10 * U.BOUND_G[U.BF16]
NAN = float("nan")


def seq_scores(c, n):
    s_a, s_t = U.scores(c["q"][n:n + 1], c["k"][n:n + 1], c["ak"], c["g2"].double(), c["vstart_list"][n:n + 1], c["F"])
    return s_a, s_t


def o_of(c, n, s_a, s_t, extra_v=None):
    v = c["v"][n:n + 1] if extra_v is None else torch.cat([c["v"][n:n + 1], extra_v[None, None]], 1)
    return U.fwd_from_scores(s_a, s_t, v, c["av"], c["g1"].double())


def fig_rows(got, ref):
    """(S, H) figures of one sequence's o / gradient (1, S, H, DH) against the reference's, floor from the reference tensor."""
    return U.row_figures(got.reshape(-1, U.DH), ref.reshape(-1, U.DH)).view(ref.shape[1], ref.shape[2])


# ------------------------------------------------------------------------------------------------ the formulas
@pytest.mark.parametrize("rope", [False, True])
def test_formulas_with_hooks_are_the_oracles(rope):
    c = U.make_case(U.BF16, 2, 70, 10, 10, [19, -1], seed=1, rope=rope)
    s_a, s_t = U.scores(c["q"], c["k"], c["ak"], c["g2"].double(), c["vstart_list"], c["F"])
    o, _, Pt = U.fwd_from_scores(s_a, s_t, c["v"], c["av"], c["g1"].double())
    assert torch.allclose(o, c["o"], rtol=0, atol=1e-13) and torch.allclose(Pt, c["Pt"], rtol=0, atol=1e-14)
    m = U.model_fwd_bwd(c, torch.float64)                  # no rounding: the oracle's backward
    ref = dict(c, dq=c["dq_rot"], dk=c["dk_rot"])
    assert torch.equal(c["dq"], c["dq_rot"]) != rope
    for t in ("o", "dq", "dk", "dv", "dak", "dav"):
        assert torch.allclose(m[t], ref[t], rtol=0, atol=1e-11), t
    fig = U.model_figures(c)                               # rounded: small, and not nothing
    assert all(0 < fig[t] < U.BOUND_G[U.BF16] for t in fig), fig


def test_row_measure_floors_zero_rows_and_sees_small_rows():
    ref = torch.zeros(4, U.DH, dtype=torch.float64)
    ref[0], ref[1] = 1.0, 1e-3
    got = ref.clone()
    got[1, 5] += 1e-3                                      # a small row off by itself: 10 % of the floor 1e-2
    got[2, 7] = 1e-3                                       # an exactly-zero row
    f = U.row_figures(got, ref)
    assert torch.allclose(f, torch.tensor([0.0, 0.1, 0.1, 0.0], dtype=torch.float64))
    whole = float((got - ref).abs().max() / ref.abs().max())
    assert whole == pytest.approx(1e-3)                    # the whole-tensor measure: a hundred times smaller


def test_gate2_has_one_head_of_each_sign():
    for seed in (100, 300, 500, 700):
        g1, g2 = U.gates(2, seed)
        assert -4 <= float(g2[0]) <= -2 and 2 <= float(g2[1]) <= 4 and float(g1.abs().max()) <= 1


# ------------------------------------------------------------------------------------------------ case 1 and 2
@pytest.mark.parametrize("dtype", DTYPES)
def test_sweep_and_window_cases_are_what_they_say(dtype):
    assert U.SWEEP_S == [1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 159, 160, 161, 255, 256, 257, 385]
    for S in (1, 2, 15, 129, 385):
        c = U.sweep_case(dtype, S)
        assert c["vstart_list"] == [-1, max(0, min(19, S - 10))] and (c["N"], c["H"], c["A"], c["F"]) == (2, 2, 10, 10)
        assert bool(torch.isfinite(c["qkv"].to(U.F16).float()).all()) and bool(torch.isfinite(c["d_o"].to(U.F16).float()).all())
        b = U.blocks(c)
        for t in b:
            assert bool(torch.isfinite(U.row_figures(b[t], b[t])).all())
        if S == 1:                                         # one key: a constant softmax, dk is exactly zero; the floor comes
            assert not bool(c["dk"].any()) and bool(c["dak"].any())          # from the adapter rows of the k block
    for S in U.WINDOW_S:
        for A, F in U.AF_PAIRS:
            assert set(U.window_vstarts(S, F)) == {0, 6, 22, 27, 118, S - F} and len(U.window_vstarts(S, F)) == len(set(U.window_vstarts(S, F)))
    c = U.window_case(dtype, 128, 1, 10, 6)                # A = 1: the adapter's dk is exactly zero, dq of row 0 too
    assert not bool(c["dak"].any()) and not bool(c["dq"][:, 0].any()) and bool(c["dk"].any())
    c = U.window_case(dtype, 160, 16, 6, 22)               # adapter rows are no smaller than the floor of their block: the
    b = U.blocks(c)                                        # per-row bound is at least as tight as a bound on their own maximum
    assert float(c["dak"].abs().max()) >= U.FLOOR_REL * float(b["dk"].abs().max())
    assert float(c["dav"].abs().max()) >= U.FLOOR_REL * float(b["dv"].abs().max())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("S", U.WINDOW_S)
@pytest.mark.parametrize("A,F", [p for p in U.AF_PAIRS if p[1] > 0])
def test_a_wrong_window_or_no_bias_is_seen_on_the_targeted_row(S, A, F, dtype):
    """The window shifted by one key, and the bias omitted, against the exact reference: the last row, whose half plant sits on
    the first frame key, moves by ten times the 16-bit bound on BOTH heads (gate2 in [-4, -2] and in [2, 4]); rows in front of
    vs + F and the sequence without a window are not touched at all."""
    targets = 0
    for vs in U.window_vstarts(S, F):
        c = U.window_case(dtype, S, A, F, vs)
        assert bool(torch.isfinite(c["qkv"].to(U.F16).float()).all())
        i = U.window_target(S, F, vs)
        s_a, s_t = seq_scores(c, 0)
        bias = lambda at: ref_cpu._text_bias(S, F, at, c["g2"].double(), torch.float64)[None]      # noqa: E731
        nobias = s_t + torch.nan_to_num(bias(-1) - bias(vs), nan=0.0)          # (-inf - -inf above the diagonal)
        shifted = s_t + torch.nan_to_num(bias(vs + 1) - bias(vs), nan=0.0)
        if i is not None:
            targets += 1
            w = c["Pt"][0, :, i, vs]
            assert i >= vs + F and 0.3 <= float(w.min()) and float(w.max()) <= 0.7, (vs, w.tolist())
        for what, s_bad in (("no bias", nobias), ("shifted", shifted)):
            f = fig_rows(c["o"][0:1], o_of(c, 0, s_a, s_bad)[0])
            assert not bool(f[:vs + F].any()), (what, vs)
            if i is not None:
                assert float(f[i].min()) >= SEE_O, (what, vs, f[i].tolist())
    assert targets >= 4                                    # every placement but the ones flush with (or over) the end


# ------------------------------------------------------------------------------------------------ case 3
def test_plant_grid_and_packing():
    g = U.plant_grid(U.PLANT_S)
    assert (0, 0) in g and (1, 0) in g and (128, 0) in g and (256, 0) in g and (256, 256) in g and (128, 127) in g
    assert (129, 128) in g and (256, 128) in g and (160, 159) in g and (256, 255) in g and len(g) == len(set(g))
    for j in U.PLANT_J:
        want = {i for i in (j, j + 1, (j // 128 + 1) * 128, 256) if i < 257}
        assert {i for (i, jj) in g if jj == j} == want
    assert U.decoys_of(15, 257) == [16, 32, 128] and U.decoys_of(16, 257) == [17, 32, 128] and U.decoys_of(128, 257) == [129, 144, 160, 256]
    for half in (False, True):
        for S in ([U.PLANT_S] if not half else U.HALF_S):
            packed = U.pack_pairs(S, half)
            flat = [(i, j) for seq in packed for (i, j, _) in seq]
            assert sorted(flat) == sorted(p for p in U.plant_grid(S) if not (half and p[0] == 0))
            for seq in packed:
                keys = [p for (_, j, dec) in seq for p in [j, *dec]]
                assert len(keys) == len(set(keys)) and len({i for (i, _, _) in seq}) == len(seq)


@pytest.mark.parametrize("dtype", DTYPES)
def test_planted_keys_carry_their_rows_and_decoys_are_invisible(dtype):
    cases = U.planted_cases(dtype)
    seen_pairs, cross = [], 0
    for c in cases:
        assert bool(torch.isfinite(c["qkv"].to(U.F16).float()).all())
        for (n, i, j, where) in c["pairs"]:
            seen_pairs.append((i, j))
            w = c["Pt"][n, :, i, j]
            assert float(w.min()) >= 0.99, f"planted key {j} of query {i}: weight {float(w.min()):.4f}"
            s_a, s_t = seq_scores(c, n)
            ref_o = c["o"][n:n + 1]
            dropped = s_t.clone()
            dropped[0, :, i, j] = float("-inf")
            if i > 0:                                      # (query 0 has no other key to fall back on)
                f = fig_rows(ref_o, o_of(c, n, s_a, dropped)[0])
                assert float(f[i].min()) >= SEE_O, (i, j, float(f[i].min()))
                f[i] = 0
                assert not bool(f.any())
            qi = c["q"][n, i]
            for (nk, p) in where:                          # the decoy leaks: one more key for query i alone
                ext = torch.cat([s_t, torch.full_like(s_t[..., :1], float("-inf"))], -1)
                ext[0, :, i, -1] = torch.einsum("hd,hd->h", qi, c["k"][nk, p]) / math.sqrt(U.DH)
                assert float(ext[0, :, i, -1].min()) > 29
                f = fig_rows(ref_o, o_of(c, n, s_a, ext, extra_v=c["v"][nk, p])[0])
                assert float(f[i].min()) >= SEE_O, (i, p, float(f[i].min()))
                f[i] = 0
                assert not bool(f.any())
                cross += nk != n
                assert nk != n or p > i                    # the reference never reads it: causally hidden, or another sequence
    assert sorted(seen_pairs) == sorted(U.plant_grid(U.PLANT_S)) and cross == 1


# ------------------------------------------------------------------------------------------------ case 4
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("S", U.HALF_S)
def test_half_plants_weigh_a_half_and_a_dropped_pair_moves_its_three_rows(dtype, S):
    cases = U.planted_cases(dtype, S, half=True)
    n_pairs = 0
    for c in cases:
        assert bool(torch.isfinite(c["qkv"].to(U.F16).float()).all())
        g1, g2 = c["g1"].double(), c["g2"].double()
        for (n, i, j, _) in c["pairs"]:
            n_pairs += 1
            w = c["Pt"][n, :, i, j]
            assert 0.3 <= float(w.min()) and float(w.max()) <= 0.7, f"half plant {j} of query {i}: weight {w.tolist()}"
            s_a, s_t = seq_scores(c, n)
            s_t[0, :, i, j] = float("-inf")
            _, Pa, Pt = o_of(c, n, s_a, s_t)
            sl = slice(n, n + 1)
            dq, dk, dv, *_ = ref_cpu.attn_bwd(c["do"][sl], c["q"][sl], c["k"][sl], c["v"][sl], c["ak"], c["av"], g1, g2,
                                              c["vstart_list"][sl], c["F"], (Pa, Pt))
            fq = fig_rows(c["dq"][sl], dq)
            fk, fv = fig_rows(c["dk"][sl], dk), fig_rows(c["dv"][sl], dv)
            assert float(fq[i].min()) >= SEE_G and float(fk[j].min()) >= SEE_G and float(fv[j].min()) >= SEE_G, \
                (i, j, fq[i].tolist(), fk[j].tolist(), fv[j].tolist())
            fq[i] = 0
            assert not bool(fq.any())                      # dq of every other row reads its own row of P only
    assert n_pairs == len([p for p in U.plant_grid(S) if p[0] > 0])


# ------------------------------------------------------------------------------------------------ case 5, 6 and the log
@pytest.mark.parametrize("dtype", [U.BF16, U.F16])
def test_rope_cases_are_the_oracle_on_rotated_rounded_operands(dtype):
    c = U.sweep_case(dtype, 17, rope=True)
    q_raw = c["qkv"][: 2 * 17].view(2, 17, 3, 2, U.DH)[:, :, 0]
    assert torch.equal(c["q"], U.rotated_rounded(q_raw, c["c64"], c["s64"], dtype)) and not torch.equal(c["q"], q_raw.double())
    for cc in [c] + U.planted_cases(dtype, 128, half=True, rope=True):
        # rotated in float32, as the kernels do, the operands round to the same storage values (tiny ones within TIE_STEP)
        N, S = cc["N"], cc["S"]
        raw = cc["qkv"][: N * S].view(N, S, 3, 2, U.DH)
        for w, t in ((0, "q"), (1, "k")):
            r32 = ref_cpu.rope_apply(raw[:, :, w].float(), cc["cos"][:S], cc["sin"][:S]).to(dtype)
            assert float((r32.double() - cc[t]).abs().max()) <= U.TIE_STEP, t
    for cc in U.planted_cases(dtype, 128, half=True, rope=True):
        assert bool(torch.isfinite(cc["qkv"].to(U.F16).float()).all())
        for (n, i, j, _) in cc["pairs"]:
            w = cc["Pt"][n, :, i, j]
            assert 0.3 <= float(w.min()) and float(w.max()) <= 0.7, (i, j, w.tolist())


def test_reuse_case_and_the_fp32_logsumexp():
    c = U.reuse_case(U.BF16, 129)
    assert (c["N"], c["H"]) == (3, 2) and bool(torch.isfinite(c["qkv"].to(U.F16).float()).all())
    worst = max(U.lse_fp32_emulation(U.sweep_case(U.F32, S)) for S in (17, 257))
    print(f"logsumexp of the sweep's scores in float32 on the CPU against fp64: {worst:.3e} (bound {U.BOUND_LSE:.1e})")
    assert worst < U.BOUND_LSE / 4


@pytest.mark.parametrize("dtype", [U.BF16, U.F16])
def test_rounding_model_passes_the_judge_and_names_its_classes(dtype):
    """What the rule of the bounds rests on: the model's output, rounded to storage as a kernel's would be, is inside the
    project's bounds on every row outside MODEL_CLASSES, and on those rows its figure is printed with the bound it sets. A
    reference with one pair dropped does not pass."""
    for S in (1, 2, 16, 17, 128, 257):
        c = U.sweep_case(dtype, S)
        m = U.model_fwd_bwd(c, dtype)
        b = dict({t: x.to(dtype) for t, x in U.blocks(c, m).items()}, dg1=m["dg1"].float(), dg2=m["dg2"].float())
        U.judge(f"rounding model, sweep S={S} {dtype}", c, b)
    masks = U.class_masks(c)
    assert int(masks["dq"].sum()) == 2 * U.FEW_KEYS * 2 and not bool(masks["dk"].any())
    assert bool(U.class_masks(U.sweep_case(dtype, 2))["dk"][:4].all())
    bad = {t: x.clone() for t, x in b.items()}
    bad["dq"][300] = 0                                     # one row of dq lost, outside the classes
    with pytest.raises(AssertionError, match="dq"):
        U.judge("a lost row", c, bad, log=lambda s: None)
    bad = dict(b, dg2=b["dg2"] * 1.5)
    with pytest.raises(AssertionError, match="dg2"):
        U.judge("a wrong gate gradient", c, bad, log=lambda s: None)
