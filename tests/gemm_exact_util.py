"""Exact integer products for the GEMM routes (tests/test_gemm_exact_cpu.py, tests/test_gemm_exact_gpu.py). CPU only.

With small-integer operands every product and every partial sum of C = A · B^T is an integer that fp32 accumulators, the 24-bit
partial-tile slabs of the split-K exchange (16 significant bits) and every storage type hold exactly, so a correct kernel returns
the fp64 product word for word whatever its summation order, and any dropped, doubled or misplaced k chunk, tile edge, hand-off
piece or store is a mismatch. Nothing here carries a tolerance.

Operand families (built on the CPU from a seed, as fp64 tensors of integers):

  SA   A (M, K) in {-1, 0, +1} with <= 128 non-zeros per row, B (N, K) in {-1, +1} with about one entry in eight set to 0
  SB   the roles swapped: B sparse, A dense
  DN   A and B integers in [-2, 2]; only where the output (or the tail) is fp32: |sum| <= 4 K < 2^24

A residual and a prefilled fp32 tail hold integers in [-64, 64]. SA / SB: every partial sum over any subset of k is <= 128 in
magnitude, <= 192 with the residual or tail added: exact in bf16 (integers up to 256), fp16, fp32 and the slab format.

Coverage: every aligned block of 16 rows x 8 k of the sparse operand holds a non-zero, BY CONSTRUCTION: row j of a block covers
the k chunks c with c % 16 == j (a lane's 16-byte load is one such chunk of one row). A ragged last block of r < 16 rows staggers
modulo r; it can be covered only while ceil(K / 8 / r) <= 128 (`block_feasible`) — one row of 128 non-zeros cannot reach 512
chunks. Where it cannot (M = 1 at K = 2816, the lone 17th row at K = 4096, the 33rd at K = 11008), that block of A is left partly
covered in SA and the other family closes the gap: in SB the sparse operand is B, whose blocks are all coverable at every N used
here, and a dropped chunk of EITHER operand then changes an output (the sparse one has a non-zero in that chunk in every 16 of
its rows, and the dense one a non-zero at that very k in every 16 of its own: dense_operand). The CPU tests assert this, per case.
"""
import zlib

import torch

SENT = -7.25                     # around C, the residual and the tail: exact in every dtype (tests/test_rider_gpu.SENT)
NNZ = 128                        # non-zeros per row of a sparse operand


# ------------------------------------------------------------------------------------------------------------------ operands
def block_feasible(rows_in_block: int, K: int) -> bool:
    """Can a block of `rows_in_block` rows x K, NNZ non-zeros per row, hold a non-zero in every 8-wide k chunk?"""
    return -(-(K // 8) // rows_in_block) <= NNZ


def sparse_operand(rows: int, K: int, seed: int, nnz: int = NNZ) -> torch.Tensor:
    """(rows, K) fp64 in {-1, 0, +1}, <= nnz non-zeros per row. Row j of an aligned 16-row block (of r rows: 16, fewer in a ragged
    last block) holds one non-zero, at a random place and of random sign, in each k chunk c with c % r == j — nnz of them, evenly spaced,
    where there are more — and random further ones up to the budget."""
    assert K % 8 == 0
    g = torch.Generator().manual_seed(seed)
    nch = K // 8
    x = torch.zeros(rows, K, dtype=torch.float64)
    row = torch.arange(rows)
    r_blk = torch.clamp(rows - (row // 16) * 16, max=16)                  # rows of this row's block
    j = row % 16
    T = min(nnz, nch)
    t = torch.arange(T)
    n_own = (nch - j + r_blk - 1) // r_blk                                # chunks c with c % r == j: this row's to cover
    step = torch.where(n_own > T, n_own, torch.full_like(n_own, T))       # more than the budget: every (n_own / T)-th of them
    own = t[None, :] * step[:, None] // T
    c = j[:, None] + r_blk[:, None] * own                                 # (rows, T) chunk indices
    valid = own < n_own[:, None]
    pos = c * 8 + torch.randint(0, 8, (rows, T), generator=g)
    sign = (torch.randint(0, 2, (rows, T), generator=g) * 2 - 1).double()
    ri = row[:, None].expand(rows, T)
    x[ri[valid], pos[valid]] = sign[valid]
    # further non-zeros up to the budget (they never clear a mandatory one: only +-1 is written)
    n_mand = valid.sum(dim=1)
    E = min(nnz, K // 2)
    epos = torch.randint(0, K, (rows, E), generator=g)
    esign = (torch.randint(0, 2, (rows, E), generator=g) * 2 - 1).double()
    keep = torch.arange(E)[None, :] < (nnz - n_mand)[:, None]
    ri = row[:, None].expand(rows, E)
    x[ri[keep], epos[keep]] = esign[keep]
    assert int((x != 0).sum(dim=1).max()) <= nnz
    return x


def dense_operand(rows: int, K: int, seed: int) -> torch.Tensor:
    """(rows, K) fp64 in {-1, +1}, about one entry in eight 0 — but no k at which a whole aligned block of 16 rows (fewer in a
    ragged last block) is 0: wherever the sparse operand has its non-zero of a chunk, some row of every block of this one meets
    it. (A single row therefore holds no zero at all.)"""
    g = torch.Generator().manual_seed(seed)
    sign = (torch.randint(0, 2, (rows, K), generator=g) * 2 - 1).double()
    x = sign * (torch.randint(0, 8, (rows, K), generator=g) != 0)
    rb = -(-rows // 16)
    pad = torch.zeros(rb * 16, K, dtype=torch.bool)
    pad[:rows] = x != 0
    blk, k = (~pad.view(rb, 16, K).any(dim=1)).nonzero(as_tuple=True)
    row = 16 * blk + k % torch.clamp(rows - 16 * blk, max=16)
    x[row, k] = sign[row, k]
    return x


def small_ints(rows: int, cols: int, seed: int, bound: int) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-bound, bound + 1, (rows, cols), generator=g).double()


def seed_of(*key) -> int:
    return zlib.crc32(repr(key).encode()) % (1 << 30)


def operands(family: str, M: int, N: int, K: int):
    """-> (A (M, K), B (N, K)) fp64 integers of the family; the seed is a function of the arguments only."""
    sa, sb = seed_of(family, "a", M, N, K), seed_of(family, "b", M, N, K)
    if family == "SA":
        return sparse_operand(M, K, sa), dense_operand(N, K, sb)
    if family == "SB":
        return dense_operand(M, K, sa), sparse_operand(N, K, sb)
    assert family == "DN", family
    return small_ints(M, K, sa, 2), small_ints(N, K, sb, 2)


def residual_ints(rows: int, N: int, key) -> torch.Tensor:
    """A residual, or what an fp32 tail holds before the call: integers in [-64, 64]."""
    return small_ints(rows, N, seed_of("r", rows, N, key), 64)


def coverage_gaps(x: torch.Tensor):
    """[(16-row block, 8-wide k chunk)] of the aligned blocks of x (the last one clipped to the matrix) that hold no non-zero."""
    rows, K = x.shape
    rb, nch = -(-rows // 16), K // 8
    pad = torch.zeros(rb * 16, K, dtype=torch.bool)
    pad[:rows] = x != 0
    hit = pad.view(rb, 16, nch, 8).any(dim=3).any(dim=1)
    return [tuple(v) for v in (~hit).nonzero().tolist()]


def infeasible_blocks(rows: int, K: int):
    """Row blocks that NNZ non-zeros per row cannot cover (at K <= 16384 only ever a ragged last block)."""
    return [b for b in range(-(-rows // 16)) if not block_feasible(min(16, rows - 16 * b), K)]


# ------------------------------------------------------------------------------------------------------------------- windows
def windowed(t: torch.Tensor, pad_rows, pad_cols, fill: float):
    """Place t (2-D) as an interior window of a larger tensor of its dtype and device filled with `fill`. pad_rows / pad_cols:
    (before, after) counts. -> (arena, view); the view's row stride is the arena's width."""
    (r0, r1), (c0, c1) = pad_rows, pad_cols
    R, C = t.shape
    arena = torch.full((r0 + R + r1, c0 + C + c1), fill, dtype=t.dtype, device=t.device)
    view = arena[r0:r0 + R, c0:c0 + C]
    view.copy_(t)
    return arena, view


def locate(window: torch.Tensor, width: int):
    """(first row, first column, rows, columns) of a 2-D window in an arena `width` elements wide that starts at storage offset 0."""
    assert window.dim() == 2 and (window.stride(1) == 1 or window.shape[1] == 1) and window.stride(0) == width, \
        (window.shape, window.stride(), width)
    off = window.storage_offset()
    return off // width, off % width, window.shape[0], window.shape[1]


def bits(t: torch.Tensor) -> torch.Tensor:
    """The words of t as integers (bitwise comparison: NaN payloads and the sign of zero count)."""
    return t.contiguous().view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def check_exact(got_arena: torch.Tensor, window: torch.Tensor, want: torch.Tensor, fill: float = SENT, operands=()):
    """Raises AssertionError unless (1) the window of got_arena equals `want` under torch.equal — value equality: the sign of zero
    is not compared, a NaN fails; (2) every word of got_arena outside the window still holds the bits of `fill`; (3) each
    (now, original) pair of `operands` is bitwise equal. window: a view that lies in got_arena — or in an arena of the same
    geometry, such as the device tensor got_arena was copied from — where the output was to be written."""
    assert got_arena.dim() == 2 and got_arena.is_contiguous()
    r0, c0, R, C = locate(window, got_arena.shape[1])
    assert r0 + R <= got_arena.shape[0] and c0 + C <= got_arena.shape[1]
    assert tuple(want.shape) == (R, C), (tuple(want.shape), (R, C))
    got = got_arena[r0:r0 + R, c0:c0 + C]
    want = want.to(got.dtype)
    if not torch.equal(got, want):
        bad = ~(got == want)
        idx = bad.nonzero()
        m, n = (int(v) for v in idx[0])
        rows, cols = idx[:, 0], idx[:, 1]
        raise AssertionError(
            f"{int(bad.sum())} of {R * C} words differ, {int(torch.isnan(got.float()).sum())} NaN; first at ({m}, {n}): got "
            f"{float(got[m, n])}, want {float(want[m, n])}; rows {int(rows.min())}..{int(rows.max())}, columns "
            f"{int(cols.min())}..{int(cols.max())}")
    fb = bits(torch.full((1,), fill, dtype=got_arena.dtype))[0]
    around = bits(got_arena).clone()
    around[r0:r0 + R, c0:c0 + C] = fb
    if not bool((around == fb).all()):
        idx = (around != fb).nonzero()
        m, n = (int(v) for v in idx[0])
        raise AssertionError(f"{idx.shape[0]} words around the window changed; first at arena ({m}, {n}), window origin ({r0}, {c0}), "
                             f"window {R} x {C}: {float(got_arena[m, n])}")
    for i, (now, orig) in enumerate(operands):
        if not torch.equal(bits(now), bits(orig)):
            raise AssertionError(f"operand arena {i} changed")


# ------------------------------------------------------------------------------------------------- the arithmetic, emulated
def round24(x: torch.Tensor) -> torch.Tensor:
    """fp32 -> the 24-bit slab format and back (csrc/gemm_sk.hip round24 / pack24 / unpack24): add 0x80 to the word, drop its
    low byte; a word whose exponent is all ones keeps its bits."""
    u = x.contiguous().view(torch.int32)
    special = (u & 0x7F800000) == 0x7F800000
    r = torch.where(special, u, u + 0x80) & -256
    return r.view(torch.float32)


def emulate(a: torch.Tensor, b: torch.Tensor, seed: int = 0):
    """The product as a kernel may form it: fp32, k permuted, cut into 8 pieces whose partial sums are added in fp32 — whole, or
    as 2, 4 or 8 pieces each passed through round24 first. -> {pieces: fp32 (M, N)} for pieces in 1, 2, 4, 8."""
    K = a.shape[1]
    perm = torch.randperm(K, generator=torch.Generator().manual_seed(seed))
    af, bf = a[:, perm].float(), b[:, perm].float()
    cuts = [K * i // 8 for i in range(9)]
    p8 = [af[:, cuts[i]:cuts[i + 1]] @ bf[:, cuts[i]:cuts[i + 1]].T for i in range(8)]
    out = {}
    for s in (1, 2, 4, 8):
        g = 8 // s
        parts = []
        for i in range(s):
            p = p8[i * g]
            for q in p8[i * g + 1:(i + 1) * g]:
                p = p + q
            parts.append(p if s == 1 else round24(p))
        tot = parts[0]
        for p in parts[1:]:
            tot = tot + p
        out[s] = tot
    return out


# ------------------------------------------------------------------------------------------------------------ the route table
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
ALL, H16, ONLY32 = (F32, BF16, F16), (BF16, F16), (F32,)
WIDTHS = (11, 12, 13, 14, 16)


class Case:
    """One fvqa_gemm_nt call. route: the kernel meant to take it — "128" (gemm_nt_128), "skinny" (gemm_nt_skinny), "fewrows",
    "sk256" (gemm_sk_256), "4w" (gemm4w_k), "sk4" (gemm4w_sk_k); s: pieces per tile of the split round (1: whole tiles), full:
    rounds of whole tiles before it (both None where the route has no tile plan). out: "st" (the storage type) or "f32";
    m_split: rows from there on accumulate into a prefilled fp32 tail; acc: out=None, every row into the tail; nbt: forced 4-wave
    tile width; contig: run with contiguous operands too."""

    def __init__(self, cid, route, M, N, K, dtypes, *, variant=0, out="st", resid=False, m_split=None, acc=False, nbt=None,
                 s=None, full=None, contig=False):
        self.id, self.route, self.M, self.N, self.K, self.dtypes = cid, route, M, N, K, dtypes
        self.variant, self.out, self.resid, self.m_split, self.acc, self.nbt = variant, out, resid, m_split, acc, nbt
        self.s, self.full, self.contig = s, full, contig
        assert not (acc and (resid or m_split is not None or out != "st"))

    def families(self):
        """DN only where the output, or the tail, is fp32 (every dtype's output is, in the fp32 build)."""
        f32_words = self.out == "f32" or self.acc or self.m_split is not None or self.dtypes == ONLY32
        return ("SA", "SB", "DN") if f32_words else ("SA", "SB")

    def __repr__(self):
        return self.id


def _cases():
    cs = []
    # ---- gemm_nt_128, register-staged (variant 1) and DMA-staged (variant 2), all three builds. K of one stage (64 in 16 bits,
    # 32 in fp32) and of several; M and N no multiple of 128; one and several tiles; tail rows from inside a tile and from a tile edge
    for v in (1, 2):
        t = f"128v{v}"
        cs += [
            Case(f"{t}_77x200x128", "128", 77, 200, 128, ALL, variant=v, contig=v == 1),
            Case(f"{t}_77x200x128_f32out", "128", 77, 200, 128, H16, variant=v, out="f32"),
            Case(f"{t}_77x200x128_resid", "128", 77, 200, 128, ALL, variant=v, resid=True),
            Case(f"{t}_77x200x64", "128", 77, 200, 64, ALL, variant=v),                    # one stage in 16 bits
            Case(f"{t}_77x200x32", "128", 77, 200, 32, ONLY32, variant=v),                 # one stage in fp32
            Case(f"{t}_138x256x512", "128", 138, 256, 512, ALL, variant=v),
            Case(f"{t}_138x256x512_f32out", "128", 138, 256, 512, H16, variant=v, out="f32"),
            Case(f"{t}_138x256x512_resid", "128", 138, 256, 512, ALL, variant=v, resid=True, contig=v == 2),
            Case(f"{t}_74x200x128_tail64", "128", 74, 200, 128, ALL, variant=v, m_split=64),
            Case(f"{t}_138x256x512_tail128_resid", "128", 138, 256, 512, ALL, variant=v, m_split=128, resid=True),
            Case(f"{t}_266x256x192_tail256_f32out", "128", 266, 256, 192, H16, variant=v, m_split=256, out="f32"),
        ]
    # ---- gemm_nt_skinny, forced (variant 12) and picked (variant 0): M in {1, 3, 16}; N of an even strip count, an odd one and
    # ragged; K of 1, 4 and 11 times the 256 a wave pair takes per turn (a Latin square of the three)
    ks = {(1, 512): 256, (1, 528): 1024, (1, 1000): 2816, (3, 512): 1024, (3, 528): 2816, (3, 1000): 256,
          (16, 512): 2816, (16, 528): 256, (16, 1000): 1024}
    for (M, N), K in ks.items():
        t = f"skinny_{M}x{N}x{K}"
        cs += [
            Case(f"{t}_v12", "skinny", M, N, K, H16, variant=12, contig=(M, N) == (3, 528)),
            Case(f"{t}_v12_f32out", "skinny", M, N, K, H16, variant=12, out="f32"),
            Case(f"{t}_v12_resid", "skinny", M, N, K, H16, variant=12, resid=True),
            Case(f"{t}_v0_resid", "skinny", M, N, K, H16, resid=True),
            Case(f"{t}_v0_f32out", "skinny", M, N, K, H16, out="f32"),
            Case(f"{t}_acc", "skinny", M, N, K, H16, acc=True, contig=(M, N) == (16, 1000)),
        ]
    # ---- the few-rows kernels: 17, 33 and 64 rows (2, 3 and 4 row blocks) against N x K >= 2^24; N no multiple of 64
    for (M, N, K) in ((17, 4104, 4096), (64, 4096, 4096), (33, 2048, 11008)):
        t = f"fewrows_{M}x{N}x{K}"
        cs += [
            Case(t, "fewrows", M, N, K, H16, contig=M == 17),
            Case(f"{t}_f32out", "fewrows", M, N, K, H16, out="f32"),
            Case(f"{t}_resid", "fewrows", M, N, K, H16, resid=True),
        ]
    # ---- gemm_sk_256, fp32 build (variant 13, and variant 0 where the shape is the persistent family's). Plans on 256 CUs.
    for resid in (False, True):
        r = "_resid" if resid else ""
        cs += [
            Case(f"sk256_f32_one_tile{r}", "sk256", 256, 256, 64, ONLY32, variant=13, resid=resid, s=1, full=0),
            Case(f"sk256_f32_ragged{r}", "sk256", 200, 264, 128, ONLY32, variant=13, resid=resid, s=1, full=0,
                 contig=resid),                                                            # M < 256, N % 256 != 0: 2 tiles
            Case(f"sk256_f32_split2{r}", "sk256", 256, 1024, 512, ONLY32, resid=resid, s=2, full=0),
            Case(f"sk256_f32_split4{r}", "sk256", 520, 1000, 1024, ONLY32, resid=resid, s=4, full=0),     # ragged M and N
            Case(f"sk256_f32_split8_ragged_k{r}", "sk256", 300, 768, 2112, ONLY32, resid=resid, s=8, full=0),  # 66 stages: 17 granules
            Case(f"sk256_f32_mgroups{r}", "sk256", 2304, 256, 64, ONLY32, resid=resid, s=1, full=0),     # 9 m tiles: 2 groups of 5
            # 8 m tiles x 33 n tiles on 32 teams: a round of whole tiles, then one tile whole (K = 64) or split 2 (K = 512)
            Case(f"sk256_f32_two_rounds{r}", "sk256", 1800, 8440, 64, ONLY32, resid=resid, s=1, full=1),
        ]
    cs += [Case("sk256_f32_round_then_split2", "sk256", 1800, 8440, 512, ONLY32, resid=True, s=2, full=1)]
    # ---- gemm_sk_256 on 16-bit operands: a split of 8 (the 4-wave split-K kernel takes 2 and 4), fp32 output on split tile sets
    cs += [
        Case("sk256_h16_split8", "sk256", 256, 2048, 4096, H16, s=8, full=0, contig=True),
        Case("sk256_h16_split8_resid", "sk256", 256, 2048, 4096, H16, resid=True, s=8, full=0),
        Case("sk256_h16_split2_f32out", "sk256", 512, 1024, 1024, H16, out="f32", s=2, full=0),
        Case("sk256_h16_split4_f32out", "sk256", 1000, 4000, 4096, H16, out="f32", s=4, full=0),
    ]
    # ---- gemm4w_k at every tile width, ragged in M and N; K of 5 stages and of 17 (the second shape: 2 m groups x 13 n tiles,
    # too many tiles for the 8-wave plan to split, so that the whole-tile kernel keeps it)
    for (M, N, K) in ((1034, 3000, 320), (2058, 3080, 1088)):
        for nbt in WIDTHS:
            t = f"4w_w{nbt}_{M}x{N}x{K}"
            cs += [
                Case(t, "4w", M, N, K, H16, nbt=nbt, contig=(nbt, K) == (13, 320)),
                Case(f"{t}_resid", "4w", M, N, K, H16, nbt=nbt, resid=True),
                Case(f"{t}_f32out", "4w", M, N, K, H16, nbt=nbt, out="f32"),
            ]
    # ---- gemm4w_sk_k: 2 pieces, and 4 pieces on tile sets ragged in M and N
    for (M, N, K, s) in ((512, 1024, 1024, 2), (1000, 4000, 4096, 4), (520, 4088, 2048, 4)):
        cs += [
            Case(f"sk4_split{s}_{M}x{N}x{K}", "sk4", M, N, K, H16, s=s, full=0, contig=s == 2),
            Case(f"sk4_split{s}_{M}x{N}x{K}_resid", "sk4", M, N, K, H16, resid=True, s=s, full=0),
        ]
    return cs


CASES = _cases()
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)


def problems():
    """The distinct (family, M, N, K) of the table (operands and their fp64 product are a function of these alone)."""
    seen = {}
    for c in CASES:
        for f in c.families():
            seen.setdefault((f, c.M, c.N, c.K), c)
    return list(seen)
