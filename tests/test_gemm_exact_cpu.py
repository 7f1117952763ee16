"""CPU half of the exact-product GEMM tests (tests/gemm_exact_util.py, tests/test_gemm_exact_gpu.py): that the REFERENCE stays
exact for every problem of the GPU table whatever the summation order, the split and the storage type; that the operand families
keep their coverage condition; and that check_exact sees the defects the GPU tests are there to catch. No GPU, no library."""
import pytest
import torch

from tests import gemm_exact_util as U
from tests.gemm_exact_util import SENT, check_exact, windowed

NAN = float("nan")
PROBLEMS = U.problems()
IDS = [f"{f}-{M}x{N}x{K}" for (f, M, N, K) in PROBLEMS]


@pytest.mark.parametrize("family,M,N,K", PROBLEMS, ids=IDS)
def test_reference_is_exact_in_every_order_split_and_type(family, M, N, K):
    """The fp64 product recomputed in fp32 with k permuted, whole and as 2, 4 and 8 pieces whose partial sums pass through the
    24-bit slab format, then rounded once to bf16 / fp16 (SA, SB; with the largest residual or tail value added too): every
    result is the fp64 product. If this fails for a shape, the shape or the family is wrong, not a kernel."""
    a, b = U.operands(family, M, N, K)
    ref = a @ b.T
    sparse = {"SA": a, "SB": b}.get(family)
    if sparse is not None:
        dense = b if family == "SA" else a
        assert int((sparse != 0).sum(dim=1).max()) <= U.NNZ and float(sparse.abs().max()) <= 1 and float(dense.abs().max()) == 1
        assert float(ref.abs().max()) <= U.NNZ             # every partial sum over any subset of k, this one included
    else:
        assert float(a.abs().max()) <= 2 and float(b.abs().max()) <= 2 and 4 * K < 1 << 24
    for pieces, got in U.emulate(a, b, seed=K + 7 * M + N).items():
        assert torch.equal(got.double(), ref), pieces
        if sparse is not None:
            for dt in (torch.bfloat16, torch.float16):
                assert torch.equal(got.to(dt).double(), ref), (pieces, dt)
                for r in (64.0, -64.0):                    # the residual's / the tail's range: |sum| <= 192
                    assert torch.equal((got + r).to(dt).double(), ref + r), (pieces, dt, r)


def test_round24_emulation_matches_the_slab_format():
    """Add 0x80 to the word, drop the low byte: 16 significant bits, ties away from zero; Inf / NaN keep their bits."""
    x = torch.tensor([1.0, -3.0, 65535.0, 65536.0, 65537.0, 131071.0, 131073.0, 192.0, float("inf"), NAN])
    r = U.round24(x)
    assert torch.equal(r[:4], x[:4]) and r[4] == 65538.0 and r[5] == 131072.0 and r[6] == 131072.0 and r[7] == 192.0
    assert r[8] == float("inf") and bool(torch.isnan(r[9]))


@pytest.mark.parametrize("family,M,N,K", [p for p in PROBLEMS if p[0] != "DN"], ids=[i for i in IDS if not i.startswith("DN")])
def test_coverage_condition(family, M, N, K):
    """Every aligned block of 16 rows x 8 k of the sparse operand holds a non-zero — by construction, so wherever 128 non-zeros
    per row can do it. B (SB) can at every shape of the table; A (SA) cannot in a ragged last block of too few rows for K
    (M = 1 at K = 2816, the 17th and the 33rd row of the few-rows shapes): there the gaps lie in that block alone."""
    a, b = U.operands(family, M, N, K)
    x = a if family == "SA" else b
    gaps, bad = U.coverage_gaps(x), U.infeasible_blocks(*x.shape)
    if family == "SB":
        assert bad == [] and gaps == []
    else:
        assert all(blk in bad for (blk, _) in gaps), gaps[:4]
        assert bad in ([], [(M - 1) // 16]) and (gaps == []) == (bad == [])
        assert U.infeasible_blocks(N, K) == []             # ... and the SB problem of the same shape is covered throughout


def test_every_case_of_the_table_has_its_problems_here():
    assert {(f, c.M, c.N, c.K) for c in U.CASES for f in c.families()} == set(PROBLEMS)
    for c in U.CASES:
        assert c.N % 8 == 0 and c.K % (32 if c.dtypes == U.ONLY32 else 64) == 0
        assert ("DN" in c.families()) == (c.out == "f32" or c.acc or c.m_split is not None or c.dtypes == U.ONLY32)
        assert c.M * c.N * c.K <= 2e10


# ----------------------------------------------------------------------------------------------------- the check sees defects
def _sample(n_blocks, n_chunks, want=100):
    """>= `want` (block, chunk) positions (all of them where there are fewer), the first and last of either dimension among them."""
    g = torch.Generator().manual_seed(n_blocks * 131 + n_chunks)
    pos = {(i, j) for i in (0, n_blocks - 1) for j in (0, n_chunks - 1)}
    if n_blocks * n_chunks <= want + 4:
        return sorted((i, j) for i in range(n_blocks) for j in range(n_chunks))
    while len(pos) < want + 4:
        pos.add((int(torch.randint(0, n_blocks, (1,), generator=g)), int(torch.randint(0, n_chunks, (1,), generator=g))))
    return sorted(pos)


def _rejects(got, want, dt):
    """check_exact on a window holding `got` where `want` belongs."""
    arena, view = windowed(got.to(dt), (1, 2), (16, 16), SENT)
    try:
        check_exact(arena, view, want.to(dt))
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("family,M,N,K", PROBLEMS, ids=IDS)
def test_check_sees_defects(family, M, N, K):
    """Applied to the reference: a dropped 16 x 8 chunk of A, of B, a doubled one (>= 100 positions per operand, the first and
    last of every dimension among them), a dropped K piece of a 256 x 256 tile, a tile's last k granule skipped, an output row
    written one row lower, a word written beside the window, an operand word changed: check_exact fails each time, and passes
    the clean reference. A chunk of the sparse operand that holds no non-zero is no defect to see; it occurs only in the blocks
    test_coverage_condition names, never in SB."""
    a, b = U.operands(family, M, N, K)
    ref = a @ b.T
    dt = torch.float32 if family == "DN" else torch.bfloat16
    arena, view = windowed(ref.to(dt), (2, 3), (16, 16), SENT)
    check_exact(arena, view, ref, SENT, [(a, a.clone()), (b, b.clone())])
    assert not _rejects(ref[:16], ref[:16], dt)
    bad_a = U.infeasible_blocks(M, K) if family == "SA" else []
    void = 0
    # chunks of A: the rows of the block change
    for (blk, ch) in _sample(-(-M // 16), K // 8):
        rows, ks = slice(16 * blk, min(M, 16 * blk + 16)), slice(8 * ch, 8 * ch + 8)
        delta = a[rows, ks] @ b[:, ks].T
        if family == "SA" and not bool(a[rows, ks].any()):
            assert blk in bad_a
            void += 1
            continue
        assert _rejects(ref[rows] - delta, ref[rows], dt), ("A dropped", blk, ch)
        assert _rejects(ref[rows] + delta, ref[rows], dt), ("A doubled", blk, ch)
    # chunks of B: the columns of the block change
    for (blk, ch) in _sample(-(-N // 16), K // 8):
        cols, ks = slice(16 * blk, min(N, 16 * blk + 16)), slice(8 * ch, 8 * ch + 8)
        delta = a[:, ks] @ b[cols, ks].T
        if family == "SA" and not bool(a[:, ks].any()):
            assert bad_a == list(range(-(-M // 16)))       # no row block of A can be covered: M < 16 at this K
            void += 1
            continue
        assert _rejects(ref[:, cols] - delta, ref[:, cols], dt), ("B dropped", blk, ch)
        assert _rejects(ref[:, cols] + delta, ref[:, cols], dt), ("B doubled", blk, ch)
    assert void == 0 or bad_a
    # a K piece of a 256 x 256 tile never added; the tile's last granule (4 stages of 64) skipped
    tm, tn = -(-M // 256), -(-N // 256)
    for (ti, tj) in {(0, 0), (tm - 1, tn - 1), (0, tn - 1), (tm - 1, 0)}:
        rows, cols = slice(256 * ti, min(M, 256 * ti + 256)), slice(256 * tj, min(N, 256 * tj + 256))
        ranges = [(K - ((K - 1) % 256 + 1), K)]
        for s in (2, 4, 8):
            if K // s >= 8:
                ranges += [(0, K // s // 8 * 8), ((s - 1) * (K // s) // 8 * 8, K)]
        for (k0, k1) in ranges:
            got = ref[rows].clone()
            got[:, cols] -= a[rows, k0:k1] @ b[cols, k0:k1].T
            assert _rejects(got, ref[rows], dt), ("K piece", ti, tj, k0, k1)
    # an output row written one row lower: inside the window, and its last row past the window's end
    for r in {0, M // 2, M - 2} & set(range(M - 1)):
        got = ref[r:r + 2].clone()
        got[1], got[0] = ref[r], NAN
        assert _rejects(got, ref[r:r + 2], dt), ("row", r)
    arena, view = windowed(ref.to(dt), (2, 3), (16, 16), SENT)
    view[M - 1] = NAN
    arena[2 + M, 16:16 + N] = ref[M - 1].to(dt)
    with pytest.raises(AssertionError):
        check_exact(arena, view, ref)
    # one word beside the window: above, below, left, right; and the same word rewritten with other bits
    for (r, c_) in ((1, 16), (2 + M, 16 + N - 1), (2, 15), (2 + M - 1, 16 + N)):
        arena, view = windowed(ref.to(dt), (2, 3), (16, 16), SENT)
        arena[r, c_] = ref[0, 0].to(dt) if float(ref[0, 0]) != SENT else 1.0
        with pytest.raises(AssertionError, match="around the window"):
            check_exact(arena, view, ref)
    # an operand word changed
    a2 = a.clone()
    a2[M - 1, K - 1] += 1
    with pytest.raises(AssertionError, match="operand"):
        check_exact(*windowed(ref.to(dt), (2, 3), (16, 16), SENT), ref, SENT, [(a2, a)])


def test_check_exact_compares_values_inside_and_bits_outside():
    """Inside the window: value equality (-0 equals +0, a NaN fails). Outside: bits (a sentinel rewritten as another NaN or a
    -0 in place of +0 fails)."""
    want = torch.tensor([[0.0, 1.0], [-2.0, 0.0]])
    arena, view = windowed(torch.tensor([[-0.0, 1.0], [-2.0, 0.0]]), (1, 1), (1, 1), 0.0)
    check_exact(arena, view, want, 0.0)
    view[0, 1] = NAN
    with pytest.raises(AssertionError, match="differ"):
        check_exact(arena, view, want, 0.0)
    arena, view = windowed(want.clone(), (1, 1), (1, 1), 0.0)
    arena[0, 0] = -0.0
    with pytest.raises(AssertionError, match="around"):
        check_exact(arena, view, want, 0.0)
    arena, view = windowed(want.clone(), (1, 1), (1, 1), NAN)
    check_exact(arena, view, want, NAN)
    U.bits(arena)[0, 0] ^= 1                               # another NaN payload
    with pytest.raises(AssertionError, match="around"):
        check_exact(arena, view, want, NAN)
