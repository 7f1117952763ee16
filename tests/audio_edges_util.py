"""Inputs, fp64 references, launch routes and error figures for the audio front end (csrc/heads.hip: the two-source
projections, the audio cross-attention, the --train_audio backward kernels) at the edges of every kernel branch. Host code only:
tests/test_audio_edges_cpu.py checks it without a GPU, tests/test_audio_edges_gpu.py runs the kernels against it.

* `route_*` restate the host routing of heads.hip and the trip / tile counts of the kernels' loops in plain Python (as
  tests/flipped_util.py: wide_schedule does for the suffix pass). Every case of the tables below carries the route and the partial
  trip it was written for (`expect`): a later change of a threshold makes the case fail instead of testing something else.
* Inputs are seeded on the CPU in storage precision, every operand from a generator seed of its own (`Inputs` asserts that no
  two operands of a case share one), every activation row scaled by its own power of two 2^-(r % 7).
* References are fp64 torch; the cross-attention backward is written out by hand (P, dP, dot, dS) so that the magnitude of what
  cancels in dS = P o (dP - sum_t P dP) is at hand: dq and dk are held against `den_q` / `den_k`, not against their own size.
"""
import functools
import math
import zlib
from collections import namedtuple

import torch

NAN = float("nan")
PAD = 4                                   # columns of padding beside / between pitched operands (16 bytes: the kernels' alignment)
PROJ = 2e-6                               # tests/test_rowops_edges_gpu.py, tests/test_audio_gpu.py VP_F32: the exact-fp32 projections
PROJ_H16 = 5e-3                           # tests/test_audio_gpu.py VP_H16: a cast token row of a 16-bit build
COND_A = 1e-6                             # condition (a): torch's own fp32 product against fp64, per row (half of PROJ)
COND_B = 5e-6                             # condition (b): the fp32 restatement of the cross-attention against fp64
CA_FLOOR, CA_FACTOR = 2e-6, 4.0           # cross-attention bound = max(CA_FLOOR, CA_FACTOR x the fp32 restatement's figure)


# ------------------------------------------------------------------------------ inputs
def by_name(fn):
    """A problem is built once per case (names are unique) and shared by the tests that need it; nobody changes it."""
    made = {}

    @functools.wraps(fn)
    def get(case):
        if case.name not in made:
            made[case.name] = fn(case)
        return made[case.name]
    return get


# Cases whose first inputs missed condition (a) or (b) of tests/test_audio_edges_cpu.py when the fp32 side was torch's own matmul on
# the host they were written on (figures below; a property of the inputs and of that host, not of the kernels): they draw other
# inputs, the bounds stay. In the fixed summation order that the conditions are asserted in (tree_sum below) both draws pass.
RESEED = {"mfma2-concat-K64+320-R127-D24": 1,     # 1.02e-6 -> 7.9e-7 (127 rows of only 24 outputs: the worst row of many)
          "mfma2-concat-K64+320-R128-D24": 5,     # 1.09e-6 -> 7.9e-7
          "mfma2-sum-K64+320-R127-D24": 1,        # 1.01e-6 -> 8.2e-7
          "stream2-K768+1024-R129-D22": 1,        # 1.42e-6 -> 7.5e-7
          "ca-peaked-nq16-T2-dim2052": 1}         # dq 5.1e-6 -> 2.3e-6


class Inputs:
    """Seeded operands of ONE case: uniform in (-scale, scale), rounded to fp32. The generator seed is a hash of (case, operand
    name), never a function of the shape: two operands whose shapes happen to sum to the same number must not share a stream."""

    def __init__(self, case):
        self.case, self.seeds = f"{case}#{RESEED[case]}" if case in RESEED else str(case), {}

    def t(self, name, *shape, scale=1.0, rows=False):
        seed = zlib.crc32(f"{self.case}/{name}".encode())
        assert name not in self.seeds and seed not in self.seeds.values(), (self.case, name, "shares a generator seed")
        self.seeds[name] = seed
        g = torch.Generator().manual_seed(seed)
        x = (torch.rand(*shape, generator=g, dtype=torch.float64) * 2 - 1) * scale
        if rows:                                              # every row on its own scale: a small row cannot hide behind a large one
            x = x * row_scales(shape[0])[:, None]
        return x.float()


def row_scales(n):
    return 2.0 ** -(torch.arange(n) % 7).double()


def pitched(t, fill=NAN, left=PAD, right=PAD):
    """t as a column range of a wider buffer -> (buffer, first column). The other columns hold `fill` (NaN: nothing may read
    them), or a tensor of the buffer's shape (the base of an accumulated output)."""
    rows, cols = t.shape
    right += -(left + cols + right) % 4                       # the pitch stays a multiple of 16 bytes
    if torch.is_tensor(fill):
        buf = fill.clone()
        assert tuple(buf.shape) == (rows, left + cols + right)
    else:
        buf = torch.full((rows, left + cols + right), fill, dtype=t.dtype)
    buf[:, left:left + cols] = t
    return buf, left


def two_ranges(k0, k1):
    """Column layout of two ranges in one buffer: PAD | k0 | PAD | k1 | PAD -> (first column of each, width)."""
    return (PAD, 2 * PAD + k0), 3 * PAD + k0 + k1


def outside_unchanged(after, before, inside):
    """Bit patterns outside the boolean mask `inside` are the ones the buffer had before the call (NaNs included)."""
    it = {4: torch.int32, 2: torch.int16}[after.element_size()]
    a, b = after.detach().cpu().contiguous().view(it), before.detach().cpu().contiguous().view(it)
    return bool(torch.equal(a[~inside], b[~inside]))


def mask2d(shape, rows, c0, cols):
    m = torch.zeros(shape, dtype=torch.bool)
    m[:rows, c0:c0 + cols] = True
    return m


# ------------------------------------------------------------------------------ fp32 arithmetic in a fixed order
# The preconditions and the cross-attention bounds are figures of an fp32 evaluation against fp64. torch's matmul sums in an
# order that depends on the machine's BLAS, vector width and thread count (the same peaked case gave dq 2.3e-6 on one host and
# 1.2e-5 on another), so a figure taken from it would make a test pass on one machine and fail on the next. These sums use
# elementwise products and a pairwise tree of elementwise adds only: every step is one IEEE operation, the same bits everywhere.
def tree_sum(x):
    """Sum over the last dimension: zero-padded to a power of two, then halves added until one element is left."""
    n = x.shape[-1]
    m = 1 << max(0, (n - 1).bit_length())
    if m != n:
        x = torch.nn.functional.pad(x, (0, m - n))
    while x.shape[-1] > 1:
        h = x.shape[-1] // 2
        x = x[..., :h] + x[..., h:]
    return x[..., 0]


def nt(a, b):
    """a (M, K) b (N, K)^T -> (M, N) in the operands' dtype, every output one tree_sum of its K products."""
    M, K = a.shape
    N = b.shape[0]
    out = torch.empty(M, N, dtype=a.dtype)
    step = max(1, (1 << 22) // (M * K))
    for n0 in range(0, N, step):
        out[:, n0:n0 + step] = tree_sum(a[:, None, :] * b[None, n0:n0 + step, :])
    return out


# ------------------------------------------------------------------------------ routes (heads.hip restated)
def _ceil(a, b):
    return -(-a // b)


def route_fwd(R, Ks, D, bias, tokens):
    """proj_fwd_launch: mfma iff every K_s % 64 == 0 and R <= 128; HELD iff not mfma, one source, K <= 2048; OPT iff bias or no
    tokens. Then the loops: proj_fwd_mfma_k walks each wave's K_s / 4 columns in k-steps of 16, VU = 4 steps per trip, rows in
    <= 8 blocks of 16, one workgroup per 16 features; proj_fwd_k takes one wave per feature (4 per workgroup), 256 columns per
    lane trip."""
    mfma = all(k % 64 == 0 for k in Ks) and R <= 128
    held = (not mfma) and len(Ks) == 1 and Ks[0] <= 2048
    r = {"form": "mfma" if mfma else "held" if held else "stream", "nsrc": len(Ks), "opt": bool(bias) or not tokens}
    if mfma:
        steps = [k // 4 // 16 for k in Ks]
        r.update(steps=steps, trips=[_ceil(s, 4) for s in steps], partial=[s % 4 for s in steps], nrb=_ceil(R, 16),
                 row_clamp=R % 16 != 0, tiles=_ceil(D, 16), d_clamp=D % 16 != 0)
    else:
        r.update(blocks=_ceil(D, 4), d_return=D % 4 != 0, trips=[_ceil(k, 256) for k in Ks], ragged=[k % 256 != 0 for k in Ks])
    return r


def route_bwd(R, Ks, D, bias):
    """proj_bwd_launch: every K_s <= 1024 -> one <KMAX 16, DB 4, RT 8> launch with the sources on grid.y; else one <32, 2, 4>
    launch per source. A wave owns DB features (a workgroup 4 * DB), RT rows per trip; dbias rides on source 0 only."""
    narrow = all(k <= 1024 for k in Ks)
    db, rt = (4, 8) if narrow else (2, 4)
    return {"form": "narrow" if narrow else "wide", "launches": 1 if narrow else len(Ks), "grid_y": len(Ks) if narrow else 1,
            "db": db, "rt": rt, "blocks": _ceil(D, 4 * db), "d_partial": D % (4 * db) != 0, "d_clamp": D % db != 0,
            "row_trips": _ceil(R, rt), "row_rem": R % rt, "ragged": [k % 256 != 0 for k in Ks], "bias": bool(bias)}


def route_dx(rows, dim, k):
    """av_proj_dx_k: one workgroup per 16 columns x 16 rows, each wave dim / 4 of the reduction in steps of 16, VU = 8 per trip."""
    steps = dim // 4 // 16
    return {"steps": steps, "trips": _ceil(steps, 8), "partial": steps % 8, "col_tiles": _ceil(k, 16), "k_clamp": k % 16 != 0,
            "row_tiles": _ceil(rows, 16), "row_rem": rows % 16}


def route_ca(nq, T, dim):
    """av_cross_attn_fwd_k: a workgroup per query row, 1024 columns per thread trip. av_cross_attn_bwd_k: a workgroup per sample,
    queries in chunks of CA_QC = 16, columns in tiles of 1024 (each tile recomputes the scores)."""
    return {"chunks": _ceil(nq, 16), "last_chunk": nq % 16, "col_tiles": _ceil(dim, 1024), "col_rem": dim % 1024, "T": T}


def route_temporal(rows, F, D):
    return {"blocks": _ceil(F * D, 256), "ragged": (F * D) % 256 != 0, "samples": rows // F}


def holds(route, expect):
    """The subset `expect` of the route -> list of mismatches (empty: the case runs the branch it was written for)."""
    return [(k, route.get(k), v) for k, v in expect.items() if route.get(k) != v]


# ------------------------------------------------------------------------------ case tables
# forward projections. why: the branch of the gap table the case is there for; expect: what route_fwd must say (without bias, with
# tokens, unless the entry says otherwise). Bias and tokens are crossed in by FWD_MODES.
Fwd = namedtuple("Fwd", "name Ks layout R D xpitch expect why")
FWD_MODES = [(False, None), (True, None), (False, 1), (True, 3), (False, "R"), (True, "R")]      # (bias, F of the temporal table)
H16_MODES = [m for m in FWD_MODES if m[1] is not None]      # a 16-bit build differs only where tokens are written

MFMA2_KS = [(64, 320), (832, 192)]       # k-steps per wave (1, 5): a partial trip alone, a full trip + 1; (13, 3): 3 trips + 1, 3 of 4
MFMA2_R = [1, 16, 17, 127, 128]
MFMA2_D = [24, 520]


def _fwd_cases():
    out = []
    for ks in MFMA2_KS:
        for layout in ("concat", "sum"):
            for R in MFMA2_R:
                for D in MFMA2_D:
                    exp = {"form": "mfma", "nsrc": 2, "partial": [k // 64 % 4 for k in ks], "d_clamp": True, "nrb": _ceil(R, 16),
                           "row_clamp": R % 16 != 0}
                    out.append(Fwd(f"mfma2-{layout}-K{ks[0]}+{ks[1]}-R{R}-D{D}", ks, layout, R, D, False, exp,
                                   "VU = 4 partial trip, bn clamp with two sources / bias, nrb and ar clamp"))
    out.append(Fwd("mfma2-concat-K64+320-R17-D24-xpitch", (64, 320), "concat", 17, 24, True,
                   {"form": "mfma", "nsrc": 2, "partial": [1, 1], "d_clamp": True}, "source x with a row pitch"))
    for k in (64, 320):
        out.append(Fwd(f"mfma1-K{k}-R17-D520", (k,), "one", 17, 520, False,
                       {"form": "mfma", "nsrc": 1, "partial": [k // 64 % 4], "d_clamp": True, "row_clamp": True},
                       "NSRC = 1 with OPT (bias): partial trip"))
    out.append(Fwd("stream2-K100+36-R3-D22", (100, 36), "concat", 3, 22, True,
                   {"form": "stream", "nsrc": 2, "ragged": [True, True], "d_return": True}, "two sources, ragged K, d >= D return"))
    out.append(Fwd("stream2-K768+1024-R129-D22", (768, 1024), "sum", 129, 22, False,
                   {"form": "stream", "nsrc": 2, "ragged": [False, False], "trips": [3, 4], "d_return": True},
                   "two sources past 128 rows on the fallback"))
    out.append(Fwd("held-K100-R5-D22", (100,), "one", 5, 22, True,
                   {"form": "held", "ragged": [True], "d_return": True}, "HELD with bias, k < K0 mask"))
    out.append(Fwd("held-K2048-R129-D520", (2048,), "one", 129, 520, False,
                   {"form": "held", "trips": [8], "ragged": [False]}, "HELD at its last K"))
    out.append(Fwd("stream1-K2052-R3-D520", (2052,), "one", 3, 520, False,
                   {"form": "stream", "nsrc": 1, "trips": [9], "ragged": [True]}, "one source past HELD's 2048 columns"))
    return out


FWD_CASES = _fwd_cases()
AGREE = {"Ks": (832, 192), "D": 24, "rows": (128, 129)}      # the MFMA form and the wave form on the same 128 rows

# backward projections. entry: "proj" = av_proj_bwd (d_tok + d_qav, dtemporal (F, D)), "linear" = av_linear_bwd (g, dbias).
Bwd = namedtuple("Bwd", "name entry Ks R D F gpitch bias expect why")


def _bwd_cases():
    out = []
    for ks in [(100, 36), (768, 1024)]:
        for D in (21, 22, 24):
            for R in (1, 3, 7, 8, 9, 33):
                exp = {"form": "narrow", "grid_y": 2, "d_partial": True, "row_rem": R % 8, "row_trips": _ceil(R, 8),
                       "ragged": [k % 256 != 0 for k in ks]}
                for gp in (False, True):
                    out.append(Bwd(f"narrow-linear-K{ks[0]}+{ks[1]}-D{D}-R{R}-{'gp' if gp else 'gc'}-bias", "linear", ks, R, D,
                                   None, gp, True, exp, "BIAS with D % 16 != 0, two sources on grid.y, R against RT = 8, pitches"))
                out.append(Bwd(f"narrow-linear-K{ks[0]}+{ks[1]}-D{D}-R{R}-gp-nobias", "linear", ks, R, D, None, True, False, exp,
                               "BIAS = false at the same shapes"))
                F = 3 if R % 3 == 0 else R
                out.append(Bwd(f"narrow-proj-K{ks[0]}+{ks[1]}-D{D}-R{R}-F{F}", "proj", ks, R, D, F, False, False, exp,
                               "g0 + g1, dtemporal"))
    # 96 workgroups per source at D % 16 = 4. A dbias added by both rows of grid.y is a race of two read-modify-writes; it shows
    # where the second lands after the first and in the same L2 (the workgroups x and x + 96 share an XCD); with the 2 workgroups
    # per source of D <= 24, or with 97, the two coincide or sit on different XCDs and the sum comes out added once
    for R in (9, 33):
        out.append(Bwd(f"narrow-linear-K768+1024-D1524-R{R}-gp-bias", "linear", (768, 1024), R, 1524, None, True, True,
                       {"form": "narrow", "grid_y": 2, "d_partial": True, "blocks": 96}, "dbias once at a grid of many workgroups"))
    for R, F in ((3, 3), (12, 3)):                            # F * D = 63: one ragged block of temporal_bwd_k; one and four samples
        out.append(Bwd(f"temporal-K100+36-D21-R{R}-F{F}", "proj", (100, 36), R, 21, F, False, False,
                       {"form": "narrow"}, "temporal_bwd_k: F * D % 256 != 0, one sample / four samples"))
    for k in (1028, 2048):
        for R in (1, 3, 5, 33):
            exp = {"form": "wide", "launches": 1, "rt": 4, "db": 2, "row_rem": R % 4, "d_partial": True, "d_clamp": True,
                   "ragged": [k % 256 != 0]}
            out.append(Bwd(f"wide-linear-K{k}-D21-R{R}", "linear", (k,), R, 21, None, True, True, exp, "<32, 2, 4> at its K edges"))
            out.append(Bwd(f"wide-proj-K{k}-D21-R{R}", "proj", (k,), R, 21, R, False, False, exp, "<32, 2, 4> through av_proj_bwd"))
    out.append(Bwd("wide-linear-K1028+100-D21-R5", "linear", (1028, 100), 5, 21, None, True, True,
                   {"form": "wide", "launches": 2, "grid_y": 1}, "mixed widths: one launch each, dbias once"))
    return out


BWD_CASES = _bwd_cases()

Dx = namedtuple("Dx", "name rows dim k g1 expect")
DX_CASES = [Dx(f"dx-dim{dim}-k{k}-rows{rows}-{'g1' if g1 else 'g0'}", rows, dim, k, g1,
               {"partial": dim // 64 % 8, "k_clamp": True, "row_rem": rows % 16, "trips": _ceil(dim // 64, 8)})
            for dim in (64, 320, 576) for k in (20, 772) for rows in (1, 15, 17, 33) for g1 in (False, True)]

Ca = namedtuple("Ca", "name nq T dim mode expect")
CA_SHAPES = [(1, 1), (16, 2), (17, 16), (33, 3)]
CA_DIMS = [4, 68, 1028, 2052]
CA_MODES = ["broad", "peaked", "planted"]                     # q x 1; q x 30; one key of each sample carries >= 0.99 of every row
CA_B = 3
CA_BIG = [(17, 16, 68), (33, 3, 2052)]                        # forward only: scores beyond +-100 with a planted key
CA_CASES = [Ca(f"ca-{mode}-nq{nq}-T{T}-dim{dim}", nq, T, dim, mode,
               {"chunks": _ceil(nq, 16), "col_tiles": _ceil(dim, 1024), "col_rem": dim % 1024})
            for mode in CA_MODES for nq, T in CA_SHAPES for dim in CA_DIMS]

CA_BIG_CASES = [Ca(f"ca-big-nq{nq}-T{T}-dim{dim}", nq, T, dim, "big", {"col_tiles": _ceil(dim, 1024)}) for nq, T, dim in CA_BIG]

# the cells of the gap table -> predicate on (kind, case, route, mode)
CELLS = {
    "fwd mfma NSRC=2: partial VU trip": lambda k, c, r, m: k == "fwd" and r["form"] == "mfma" and r["nsrc"] == 2 and any(r["partial"]),
    "fwd mfma NSRC=2: full trip + partial": lambda k, c, r, m: k == "fwd" and r["form"] == "mfma" and r["nsrc"] == 2 and any(
        p and t > 1 for p, t in zip(r["partial"], r["trips"])),
    "fwd mfma NSRC=1 OPT: partial VU trip": lambda k, c, r, m: k == "fwd" and r["form"] == "mfma" and r["nsrc"] == 1 and r["opt"] and any(r["partial"]),
    "fwd mfma: D % 16 with bias": lambda k, c, r, m: k == "fwd" and r["form"] == "mfma" and r["d_clamp"] and m[0],
    "fwd mfma: D % 16 with two sources": lambda k, c, r, m: k == "fwd" and r["form"] == "mfma" and r["d_clamp"] and r["nsrc"] == 2,
    "fwd mfma: R = 1": lambda k, c, r, m: k == "fwd" and r["form"] == "mfma" and c.R == 1,
    "fwd mfma: R = 17": lambda k, c, r, m: k == "fwd" and r["form"] == "mfma" and c.R == 17,
    "fwd mfma: R = 127": lambda k, c, r, m: k == "fwd" and r["form"] == "mfma" and c.R == 127,
    "fwd mfma: pitched x": lambda k, c, r, m: k == "fwd" and r["form"] == "mfma" and c.xpitch,
    "fwd mfma: tokens with F = 1, 3, R": lambda k, c, r, m: k == "fwd" and r["form"] == "mfma" and m[1] == 3,
    "fwd stream: two sources, ragged K": lambda k, c, r, m: k == "fwd" and r["form"] == "stream" and r["nsrc"] == 2 and all(r["ragged"]),
    "fwd stream: two sources beyond 128 rows": lambda k, c, r, m: k == "fwd" and r["form"] == "stream" and r["nsrc"] == 2 and c.R > 128,
    "fwd stream: D % 4": lambda k, c, r, m: k == "fwd" and r["form"] == "stream" and r["d_return"],
    "fwd stream: one source past 2048": lambda k, c, r, m: k == "fwd" and r["form"] == "stream" and r["nsrc"] == 1,
    "fwd held: bias, ragged K": lambda k, c, r, m: k == "fwd" and r["form"] == "held" and m[0] and r["ragged"][0],
    "fwd held: K = 2048": lambda k, c, r, m: k == "fwd" and r["form"] == "held" and c.Ks == (2048,),
    "bwd: BIAS with D % (4 DB)": lambda k, c, r, m: k == "bwd" and r["bias"] and r["d_partial"],
    "bwd: BIAS with the d clamp": lambda k, c, r, m: k == "bwd" and r["bias"] and r["d_clamp"],
    "bwd: two sources on grid.y at D % 16": lambda k, c, r, m: k == "bwd" and r["grid_y"] == 2 and r["d_partial"],
    "bwd narrow: R < RT": lambda k, c, r, m: k == "bwd" and r["form"] == "narrow" and c.R < 8,
    "bwd narrow: R % RT = 1": lambda k, c, r, m: k == "bwd" and r["form"] == "narrow" and c.R > 8 and r["row_rem"] == 1,
    "bwd narrow: R % RT = RT - 1": lambda k, c, r, m: k == "bwd" and r["form"] == "narrow" and r["row_rem"] == 7,
    "bwd wide: R < RT": lambda k, c, r, m: k == "bwd" and r["form"] == "wide" and c.R < 4,
    "bwd wide: R % RT = 1": lambda k, c, r, m: k == "bwd" and r["form"] == "wide" and c.R > 4 and r["row_rem"] == 1,
    "bwd: K % 256 under pitched ldw and ldg": lambda k, c, r, m: k == "bwd" and any(r["ragged"]) and c.gpitch,
    "bwd: K = 1028": lambda k, c, r, m: k == "bwd" and c.Ks == (1028,),
    "bwd: K = 2048": lambda k, c, r, m: k == "bwd" and c.Ks == (2048,),
    "bwd: mixed widths, one launch each": lambda k, c, r, m: k == "bwd" and r["launches"] == 2,
    "temporal: F * D % 256, one sample": lambda k, c, r, m: k == "tmp" and r["ragged"] and r["samples"] == 1,
    "temporal: F * D % 256, four samples": lambda k, c, r, m: k == "tmp" and r["ragged"] and r["samples"] == 4,
    "dx: partial VU trip": lambda k, c, r, m: k == "dx" and r["partial"] and r["trips"] == 1,
    "dx: full trip + partial": lambda k, c, r, m: k == "dx" and r["partial"] and r["trips"] == 2,
    "dx: k % 16": lambda k, c, r, m: k == "dx" and r["k_clamp"],
    "dx: rows < 16": lambda k, c, r, m: k == "dx" and c.rows < 16,
    "dx: rows % 16 = 1": lambda k, c, r, m: k == "dx" and c.rows > 16 and r["row_rem"] == 1,
    "dx: g1": lambda k, c, r, m: k == "dx" and c.g1,
    "ca: dim > 1024": lambda k, c, r, m: k == "ca" and r["col_tiles"] > 1,
    "ca: dim % 1024 small": lambda k, c, r, m: k == "ca" and r["col_tiles"] > 1 and r["col_rem"] == 4,
    "ca: n_query > 16 (second chunk)": lambda k, c, r, m: k == "ca" and r["chunks"] == 2,
    "ca: three chunks, last of one query": lambda k, c, r, m: k == "ca" and r["chunks"] == 3 and r["last_chunk"] == 1,
    "ca: n_query > 16 at dim > 1024": lambda k, c, r, m: k == "ca" and r["chunks"] > 1 and r["col_tiles"] > 1,
    "ca: peaked": lambda k, c, r, m: k == "ca" and c.mode == "peaked",
    "ca: planted key": lambda k, c, r, m: k == "ca" and c.mode == "planted" and c.T > 1,
    "ca: scores beyond +-100 (forward)": lambda k, c, r, m: k == "ca" and c.mode == "big",
    "ca: one key": lambda k, c, r, m: k == "ca" and c.T == 1,
    "ca: sixteen keys": lambda k, c, r, m: k == "ca" and c.T == 16,
}


def coverage():
    """-> {cell: [case names]} over every case of every table (and every mode of the forward cases)."""
    hit = {cell: [] for cell in CELLS}

    def visit(kind, case, route, mode=None):
        for cell, pred in CELLS.items():
            if pred(kind, case, route, mode):
                hit[cell].append(case.name)

    for c in FWD_CASES:
        for m in FWD_MODES:
            visit("fwd", c, route_fwd(c.R, c.Ks, c.D, m[0], m[1] is not None), m)
    for c in BWD_CASES:
        visit("bwd", c, route_bwd(c.R, c.Ks, c.D, c.bias))
        if c.entry == "proj":
            visit("tmp", c, route_temporal(c.R, c.F, c.D))
    for c in DX_CASES:
        visit("dx", c, route_dx(c.rows, c.dim, c.k))
    for c in CA_CASES + CA_BIG_CASES:
        visit("ca", c, route_ca(c.nq, c.T, c.dim))
    return hit


# ------------------------------------------------------------------------------ figures
def row_err(got, ref, what="", quantum=0.0):
    from tests.test_rowops_edges_gpu import row_err as f     # the one definition of the per-row figure
    return f(got, ref, what, quantum)


def den_err(got, ref, den, what=""):
    """Worst row of max|got - ref| / den[row]: for a quantity whose formula cancels by design, den is the magnitude of what
    cancels. A row with den == 0 (one key: dS = 1 * (dP - dP)) must be exactly zero."""
    got, ref, den = got.detach().double().cpu(), ref.double(), den.double()
    assert got.shape == ref.shape and den.shape == ref.shape[:1], (what, got.shape, ref.shape, den.shape)
    zero = den == 0
    assert bool((got[zero] == 0).all()), f"{what}: a row with nothing to cancel is not exactly zero"
    if bool(zero.all()):
        return 0.0
    err = (got - ref).abs().amax(1)                           # (a NaN stays a NaN)
    return float((err[~zero] / den[~zero]).max())


# ------------------------------------------------------------------------------ projections: problems and references
@by_name
def fwd_problem(case):
    """-> dict of host tensors and fp64 references for one forward case. xs / ws: the fp32 sources; bias (D), temporal (R, D)
    (a table of F rows is its first F); ref (R, D) = sum_s x_s w_s^T in fp64, without bias."""
    inp = Inputs(case.name)
    ktot = sum(case.Ks)
    xs = [inp.t(f"x{s}", case.R, k, rows=True) for s, k in enumerate(case.Ks)]
    if case.layout == "concat":
        W = inp.t("W", case.D, ktot, scale=1 / math.sqrt(ktot))
        ws = [W[:, :case.Ks[0]], W[:, case.Ks[0]:]]
    else:
        ws = [inp.t(f"w{s}", case.D, k, scale=1 / math.sqrt(ktot)) for s, k in enumerate(case.Ks)]
    ref = sum(x.double() @ w.double().T for x, w in zip(xs, ws))
    return {"xs": xs, "ws": ws, "bias": inp.t("bias", case.D, scale=0.05) * float(row_scales(case.R).min()),
            "temporal": inp.t("temporal", case.R, case.D, scale=0.5), "ref": ref, "seeds": inp.seeds}


def fwd_refs(case, prob, bias, F):
    """-> (raw reference, token reference or None) of one mode."""
    raw = prob["ref"] + (prob["bias"].double()[None, :] if bias else 0.0)
    if F is None:
        return raw, None
    F = case.R if F == "R" else F
    idx = torch.arange(case.R) % F
    return raw, raw + prob["temporal"][:F].double()[idx]


def fwd_fp32(prob, bias, torch_own=False):
    """The same product in fp32: sources in order, each output a tree_sum (`nt`); torch_own: torch's matmul, for the record."""
    key = "torch32" if torch_own else "fp32"
    if key not in prob:
        prob[key] = sum((x @ w.T if torch_own else nt(x, w)) for x, w in zip(prob["xs"], prob["ws"]))
    return prob[key] + prob["bias"][None, :] if bias else prob[key]


@by_name
def bwd_problem(case):
    """-> host tensors and fp64 references of one backward case: g0 (and g1 for av_proj_bwd) (R, D), xs, the random bases the
    outputs accumulate onto and what they must hold afterwards."""
    inp = Inputs(case.name)
    R, D = case.R, case.D
    xs = [inp.t(f"x{s}", R, k, rows=True) for s, k in enumerate(case.Ks)]
    g0 = inp.t("g0", R, D, rows=True)
    g1 = inp.t("g1", R, D, rows=True) if case.entry == "proj" else None
    g = g0.double() + (g1.double() if g1 is not None else 0.0)
    p = {"xs": xs, "g0": g0, "g1": g1, "seeds": inp.seeds}
    if len(case.Ks) == 2:                                     # two column ranges of ONE gradient, random everywhere
        offs, width = two_ranges(*case.Ks)
    else:
        offs, width = (PAD,), 2 * PAD + case.Ks[0]
    p["dW_base"], p["dW_offs"] = inp.t("dW_base", D, width, scale=0.25), offs
    p["dW_ref"] = [p["dW_base"][:, o:o + k].double() + g.T @ x.double() for o, k, x in zip(offs, case.Ks, xs)]
    p["dW_fp32"] = [p["dW_base"][:, o:o + k] + nt(g.float().T.contiguous(), x.T.contiguous()) for o, k, x in zip(offs, case.Ks, xs)]
    if case.bias:
        p["dbias_base"] = inp.t("dbias_base", D + 4, scale=0.25)
        p["dbias_ref"] = p["dbias_base"][:D].double() + g0.double().sum(0)
    if case.entry == "proj":
        F = case.F
        p["dtemp_base"] = inp.t("dtemp_base", F + 1, D, scale=0.25)
        p["dtemp_ref"] = p["dtemp_base"][:F].double() + g0.double().view(R // F, F, D).sum(0)
    return p


@by_name
def dx_problem(case):
    inp = Inputs(case.name)
    g0 = inp.t("g0", case.rows, case.dim, rows=True)
    g1 = inp.t("g1", case.rows, case.dim, rows=True) if case.g1 else None
    w = inp.t("w", case.dim, case.k, scale=1 / math.sqrt(case.dim))
    g = g0.double() + (g1.double() if case.g1 else 0.0)
    return {"g0": g0, "g1": g1, "w": w, "ref": g @ w.double(), "fp32": nt(g.float(), w.T.contiguous()), "seeds": inp.seeds}


# ------------------------------------------------------------------------------ cross-attention
def ca_formula(q, k, v, dx, B, nq, T):
    """Forward and backward of x = softmax(q k^T / sqrt(dim)) v over the T keys of each of the B samples, written out (no
    autograd, every sum a tree_sum), in the dtype of its operands. -> dict with x, dq, dk, dv (flattened to rows), P, dP, dot."""
    dim = q.shape[1]
    scale = 1.0 / math.sqrt(dim)
    q3, k3, v3, d3 = q.view(B, nq, dim), k.view(B, T, dim), v.view(B, T, dim), dx.view(B, nq, dim)

    def rows_by_rows(a, b):                                   # (B, n, dim), (B, m, dim) -> (B, n, m): sum over dim
        return tree_sum(a[:, :, None, :] * b[:, None, :, :])

    def mix(w, b):                                            # (B, n, m), (B, m, dim) -> (B, n, dim): sum over m
        return tree_sum(w[:, :, None, :] * b.transpose(1, 2)[:, None, :, :])

    S = rows_by_rows(q3, k3) * scale
    E = torch.exp(S - S.amax(-1, keepdim=True))
    P = E / tree_sum(E)[..., None]
    x = mix(P, v3)
    dP = rows_by_rows(d3, v3)
    dot = tree_sum(P * dP)[..., None]
    dS = P * (dP - dot)
    return {"x": x.reshape(B * nq, dim), "dq": (mix(dS, k3) * scale).reshape(B * nq, dim),
            "dk": (mix(dS.transpose(1, 2), q3) * scale).reshape(B * T, dim), "dv": mix(P.transpose(1, 2), d3).reshape(B * T, dim),
            "P": P, "dP": dP, "dot": dot, "S": S, "scale": scale}


def ca_dens(f64, q, k, B, nq, T):
    """den_q[f] = scale sum_t P_ft (|dP_ft| + |dot_f|) max|k_t|, den_k[t] = scale sum_f P_ft (|dP_ft| + |dot_f|) max|q_f|."""
    dim = q.shape[1]
    mag = f64["P"] * (f64["dP"].abs() + f64["dot"].abs())                       # (B, nq, T)
    kmax = k.double().view(B, T, dim).abs().amax(-1)                            # (B, T)
    qmax = q.double().view(B, nq, dim).abs().amax(-1)                           # (B, nq)
    den_q = f64["scale"] * (mag * kmax[:, None, :]).sum(-1)
    den_k = f64["scale"] * (mag * qmax[:, :, None]).sum(1)
    return den_q.reshape(B * nq), den_k.reshape(B * T)


PLANT_GAP = 7.5                           # e^-7.5 x 15 other keys < 0.01


@by_name
def ca_problem(case):
    """-> host tensors, the fp64 reference, the denominators, the fp32 restatement's own figures and the bounds made of them.
    broad: q x 1; peaked: q x 30; planted: key t* = 0 (even samples) / T - 1 (odd samples) is beta u for a sign vector u and
    every query row is u + (its row scale) x noise / 4, so that q.k_t* >= 0.75 beta dim in every row: beta puts that score
    PLANT_GAP + 3 above zero, the other keys' scores are a few units at the most (the >= 0.99 is asserted on the fp64 P, not
    assumed). big: the same with 128 beta, scores in the hundreds and thousands (forward only: the other keys' P underflows,
    and a dv row made of underflowing weights has no digits to compare)."""
    B, nq, T, dim = CA_B, case.nq, case.T, case.dim
    inp = Inputs(case.name)
    q = inp.t("q", B * nq, dim)
    k = inp.t("k", B * T, dim, rows=True)
    v = inp.t("v", B * T, dim, rows=True)
    dx = inp.t("dx", B * nq, dim, rows=True)
    qs = row_scales(B * nq)[:, None]
    planted = None
    if case.mode in ("planted", "big"):
        u = torch.where(inp.t("u", dim) < 0, -1.0, 1.0).double()
        q = (q.double() / 4 * qs + u[None, :]).float()
        beta = float(2 ** math.ceil(math.log2((PLANT_GAP + 3) / (0.75 * math.sqrt(dim))))) * (128 if case.mode == "big" else 1)
        planted = [0 if n % 2 == 0 else T - 1 for n in range(B)]
        for n, t in enumerate(planted):
            k[n * T + t] = (beta * u).float()
    else:
        q = (q.double() * qs * (30.0 if case.mode == "peaked" else 1.0)).float()
    f64 = ca_formula(q.double(), k.double(), v.double(), dx.double(), B, nq, T)
    f32 = ca_formula(q, k, v, dx, B, nq, T)
    den_q, den_k = ca_dens(f64, q, k, B, nq, T)
    own = {"x": row_err(f32["x"], f64["x"], "fp32 x"), "dv": row_err(f32["dv"], f64["dv"], "fp32 dv"),
           "dq": den_err(f32["dq"], f64["dq"], den_q, "fp32 dq"), "dk": den_err(f32["dk"], f64["dk"], den_k, "fp32 dk")}
    bound = {n: max(CA_FLOOR, CA_FACTOR * e) for n, e in own.items()}
    return {"q": q, "k": k, "v": v, "dx": dx, "f64": f64, "den_q": den_q, "den_k": den_k, "own": own, "bound": bound,
            "planted": planted, "seeds": inp.seeds}
