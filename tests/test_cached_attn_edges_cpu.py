"""The helpers of tests/test_cached_attn_edges_gpu.py (tests/cached_attn_util.py), checked without a GPU: the one-row reference
is the oracle's row, a planted key carries the softmax and a decoy is invisible to the reference for every placement the GPU
tests use, and no reference vector of any case is so small that the per-row figure would divide by nothing."""
import pytest
import torch

from oracle import ref_cpu
from tests import cached_attn_util as U

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
MODES = [(d, r) for d in DTYPES for r in (False, True)]


@pytest.mark.parametrize("A", [1, 10, 16])
def test_one_row_reference_is_the_oracles_row(A):
    """S = 320: rows in front of, inside and behind the frame window (unbiased, unbiased, biased), no window, and a window that
    runs over the end of the sequence."""
    N, S, H, F = 6, 320, 2, 10
    pos, vstart = [150, 204, 205, 319, 7, 319], [200, 195, 195, -1, 0, 315]
    qkv = U.rnd(N * S + A, 3 * H * U.DH, seed=3 + A).double()
    g1, g2 = (t.double() for t in U.gates(H, 3))
    _, _, c64, s64 = U.tables(S)
    seqs = qkv[: N * S].view(N, S, 3, H, U.DH)
    qr, kr = ref_cpu.rope_apply(seqs[:, :, 0], c64, s64), ref_cpu.rope_apply(seqs[:, :, 1], c64, s64)
    v = seqs[:, :, 2]
    ak, av = (qkv[N * S:].view(A, 3, H, U.DH)[:, i] for i in (1, 2))
    o_ref, (_, pt_ref) = ref_cpu.attn_fwd(qr, kr, v, ak, av, g1, g2, vstart, F)
    for n, p in enumerate(pos):
        o, pt = U.one_row_ref(qr[n, p], kr[n], v[n], ak, av, g1, g2, vstart[n], F, p)
        assert torch.allclose(o, o_ref[n, p], rtol=0, atol=1e-13)
        assert torch.allclose(pt, pt_ref[n, :, p, : p + 1], rtol=0, atol=1e-14)
    biased = [vs >= 0 and p >= vs + F for p, vs in zip(pos, vstart)]
    assert biased == [False, False, True, False, False, False]
    o_nob, _ = U.one_row_ref(qr[2, 205], kr[2], v[2], ak, av, g1, g2, -1, F, 205)
    assert float((o_nob - o_ref[2, 205]).abs().max()) > 1e-3          # the bias is not a no-op on the biased row


def test_bias_edge_rows_hold_both_sides_of_the_edge():
    for A, F in U.AF_PAIRS:
        rows = U.bias_edge_rows(64, F)
        for vs in (0, 7):
            assert (vs + F, vs) in rows and (vs, vs) in rows and (63, vs) in rows
            assert F == 0 or (vs + F - 1, vs) in rows
        assert (63, -1) in rows and (F == 0 or any(vs + F > 64 for _, vs in rows))
        assert all(0 <= p < 64 for p, _ in rows)


def test_plant_pairs_are_the_listed_ones():
    pairs, vstart = U.plant_pairs()
    assert len(pairs) == len(set(pairs)) == 7 + 7 + 13 and all(j <= p for p, j in pairs)
    for p in (127, 128, 319):
        assert {j for q, j in pairs if q == p} == {j for j in U.PLANT_J + [p - 1, p] if j <= p}
    biased_frame = [(p, j) for (p, j), vs in zip(pairs, vstart) if vs >= 0 and vs <= j < vs + 10 and p >= vs + 10]
    assert (319, 15) in biased_frame and (319, 16) in biased_frame


def _floor_ok(want, what):
    f = U.ref_floor(want)
    assert f >= U.FLOOR, f"{what}: a reference vector of max {f:.2e}"


@pytest.mark.parametrize("dtype,rot", MODES)
def test_decode_cases_plants_carry_the_row_and_no_reference_row_is_tiny(dtype, rot):
    _floor_ok(U.sweep_case(dtype, rot)["want"], "sweep")
    for A, F in U.AF_PAIRS:
        _floor_ok(U.bias_edge_case(dtype, rot, A, F)["want"], f"bias edge A={A} F={F}")
    cases = [("planted", U.planted_decode_case(dtype, rot))]
    if dtype != torch.float16:
        cases += [(f"S=4096 j={j}", U.lds_case(dtype, rot, j)) for j in U.LDS_J]
    for what, c in cases:
        _floor_ok(c["want"], what)
        assert len(c["weight"]) >= 1
        for (n, j), w in c["weight"].items():
            assert float(w.min()) >= 0.99, f"{what}: planted key {j} of sequence {n} has weight {float(w.min()):.4f}"
    assert len(cases[0][1]["weight"]) == 27
    c = U.store_read_case(dtype, rot, 160, 2, 10, 10, [120, 127, 144], 16, seed=59)
    for t in range(16):
        _floor_ok(c["want"][t], f"store-then-read step {t}")


@pytest.mark.parametrize("dtype,rot", MODES)
@pytest.mark.parametrize("kind", U.PLANT_KINDS)
@pytest.mark.parametrize("i,tile", [(i, t) for i, ts in U.PLANT_TILES.items() for t in ts])
def test_suffix_plants_carry_the_row_and_decoys_are_invisible(i, kind, tile, dtype, rot):
    c = U.t_case(dtype, rot, i, plant=(kind, tile))
    info = c["plant"]
    assert float(info["weight"].min()) >= 0.99, f"planted weight {float(info['weight'].min()):.4f}"
    assert len(info["decoys"]) == (3 if info["c"] + 1 < c["O"] else 2)
    plain = U.t_case(dtype, rot, i, plant=(kind, tile), decoys=False)
    assert torch.equal(c["want"][info["row"]], plain["want"][info["row"]])            # sample 0's rows come first
    assert not torch.equal(c["suf"].view(torch.uint8), plain["suf"].view(torch.uint8))
    assert bool(torch.isfinite(c["cache"][c["start"][0]].float()).all())              # cache row `start`: the decoy, not NaN
    _floor_ok(c["want"][c["valid"]], "planted suffix case")
    if tile == "chunk2":                                   # the planted own-option key and the own-option decoy: second chunk
        T, s_lo = c["T"], (32 // c["T"]) * c["T"]
        assert info["row"] == 63 and info["c"] * T + info["qj"] + 1 >= s_lo + 32
        if kind in ("own_qj", "own_qj_m1"):
            assert info["key_pos"] - int(c["start"][0]) + info["c"] * T >= s_lo + 32


@pytest.mark.parametrize("dtype,rot", MODES)
def test_suffix_cases_no_reference_row_is_tiny(dtype, rot):
    cases = [(f"T case {i}", U.t_case(dtype, rot, i)) for i in range(len(U.T_CASES))]
    cases.append(("start edges", U.start_edge_case(dtype, rot)))
    cases += [(f"frame window A={A} F={F}", U.frame_window_case(dtype, rot, A, F)) for A, F in U.AF_PAIRS]
    cases += [(f"append T={T} start={st}", U.append_case(dtype, rot, T, st)) for T in (1, 7, 16) for st in U.APPEND_STARTS]
    for what, c in cases:
        assert int(c["valid"].sum()) > 0
        _floor_ok(c["want"][c["valid"]], what)
        assert not bool(c["want"][~c["valid"]].any())                                  # padding rows: zeros
        cache = c["cache"][: c["N"] * c["S"]].view(c["N"], c["S"], -1).float()
        for n, st in enumerate(c["start"].tolist()):                                   # poison from start on, none in front of it
            assert bool(torch.isnan(cache[n, st:]).all()) and bool(torch.isfinite(cache[n, :st]).all())


def test_start_edge_case_is_what_it_says():
    c = U.start_edge_case(torch.float32, True)
    assert c["start"].tolist()[:8] == U.START_EDGES and c["length"].tolist() == [4] * 8 + [0]
    valid = c["valid"].view(c["N"], c["O"], c["T"])
    assert valid[7].sum() == 5 and not bool(valid[8].any()) and bool(valid[:7].all())  # start 127: cut to 1; len 0: nothing


def test_fp32_in_the_kernels_order_stays_inside_the_fp32_bound():
    """The CPU figure that a re-derived bound would rest on: the decode formula in fp32, in the kernel's order, against fp64."""
    c = U.sweep_case(torch.float32, True)
    N, S, H = c["N"], c["S"], c["H"]
    seqs = c["full"][: N * S].view(N, S, 3, H, U.DH).double()
    arows = c["full"][N * S:].view(c["A"], 3, H, U.DH).double()
    _, _, c64, s64 = U.tables(S)
    worst = 0.0
    for n in (0, 7, 15):
        p = int(c["pos"][n])
        qhat = U.rot_rows(c["qkv_row"][n].view(3, H, U.DH)[0].double(), p, c64, s64).float().double()
        o = U.decode_row_fp32(qhat, seqs[n, :, 1], seqs[n, :, 2], arows[:, 1], arows[:, 2], c["g1"].double(), c["g2"].double(),
                              int(c["vstart"][n]), c["F"], p)
        worst = max(worst, float(U.row_figures(o.reshape(1, -1), c["want"][n].reshape(1, -1)).max()))
    print(f"decode formula in fp32 on the CPU, kernel order, per row: {worst:.3e}")
    assert worst < U.BOUND[torch.float32]
