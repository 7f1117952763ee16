"""Every route a projection call can take (csrc/gemm.hip fvqa_gemm_nt -> gemm_nt_128, gemm_nt_skinny, the few-rows kernels,
gemm_sk_256 whole or split, gemm4w_k at five widths, gemm4w_sk_k) held to the fp64 product WORD FOR WORD on exact integer
operands (tests/gemm_exact_util.py: families, windows, check_exact, the table of cases). No assertion here carries a tolerance —
except z of the (a, b)-storing SwiGLU forward, which keeps the bound of test_gemm_nt_swiglu_fwd_epilogue.

Operands are interior windows of NaN arenas (lda, ldb != K: the step hands these entries column-block views), the output a NaN
window of an arena of sentinels with the residual laid out alike, the fp32 tail rows of a flat sentinel arena: a word the kernel
never writes, a word written outside the output, a row or k chunk read from beside the operand all show. Each case names its
route; the host's own rules must predict it (no launch) and the launch record (_kinds_of) must name it again.
FVQA_GEMM4W, FVQA_GEMM4W_SK and FVQA_FEWROWS are read once per process: the rows they re-route run in child processes.
Run with -m gpu."""
import functools
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

from fvqa import _lib, ops  # noqa: E402
from oracle import ref_cpu  # noqa: E402
from tests import gemm_exact_util as U  # noqa: E402
from tests.gemm_exact_util import CASES, SENT, check_exact, windowed  # noqa: E402
from tests.test_kernels_gpu import DEV, DTYPES, _kinds_of, dev, rel, tol  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")
PARAMS = [pytest.param(c, d, id=f"{c.id}-{str(d)[6:]}") for c in CASES for d in c.dtypes if d in DTYPES]
SYNC_BYTES = 4096                                          # csrc/gemm_sk.hip: epoch flags ahead of the slabs


# ------------------------------------------------------------------------------------------------ the host's rules, restated
def _cus():
    return min(256, int(torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count))


def _off(name):
    return os.environ.get(name, "")[:1] == "0"


def _plan(M, N, K, dtype, n_cu):
    import ctypes as C
    plan = (C.c_int32 * 12)()
    code = _lib.F32 if dtype == torch.float32 else _lib.BF16           # (the host-only partition is the same in both 16-bit builds)
    assert _lib.load().fvqa_gemm_sk_describe(M, N, K, code, n_cu, C.cast(plan, C.c_void_p), -1, None, 0) == 0
    return dict(zip(("tm", "tn", "nw_tile", "gran", "gpt", "ts", "mgroups", "n_teams", "full", "rem", "s", "pstride"), plan))


def persistent_shape(M, N, K):                             # csrc/gemm.hip
    return N >= 256 and (M >= 192 or (M > 16 and N * K >= 1 << 24))


def fewrows_takes(M, N, K, dtype, out_f32, epi):           # csrc/gemm_fewrows.hip fvqa_fewrows_takes, epilogues none / residual
    if _off("FVQA_FEWROWS") or dtype == torch.float32 or M <= 16 or M > 64 or N < 256 or N % 8 or K % 32 or N * K < 1 << 24:
        return False
    if epi == 1 and out_f32:
        return False
    groups, T = -(-N // 64), K // 32                       # fr_planes: K ranges across workgroups
    ks = min(max(-(-768 // groups), 1), 16, max(T // 32, 1))
    steps = -(-T // (ks * 4))
    planes = -(-T // (steps * 4))
    return int(_lib.load().fvqa_gemm_sk_workspace()) - SYNC_BYTES >= planes * M * N * 4


def predict(c, dtype, n_cu):
    """(route, pieces per split tile or None, whole rounds or None) of a table row by the rules of the dispatch itself, in this
    process: fvqa_gemm_nt (csrc/gemm.hip), fvqa_gemm_sk_impl (gemm_sk.hip: fvqa_fewrows_takes, fvqa_gemm_sk_describe's plan,
    fvqa_gemm4w_choose, the 4-wave split-K condition) — with whatever kernel FVQA_GEMM4W / _SK / FVQA_FEWROWS rule out."""
    M, N, K = c.M, c.N, c.K
    h16, out_f32, epi = dtype != torch.float32, c.out == "f32", 1 if c.resid else 0
    tail = c.acc or c.m_split is not None
    assert N % 8 == 0                                      # (with the windows' pitch and offsets: all the persistent family asks)
    if c.variant == 13 or (c.variant == 0 and not tail and persistent_shape(M, N, K)):
        if fewrows_takes(M, N, K, dtype, out_f32, epi):
            return "fewrows", None, None
        p = _plan(M, N, K, dtype, n_cu)
        split = p["s"] if p["rem"] else 1
        if h16 and not (p["full"] == 0 and p["s"] > 1):
            with ops.gemm4w_width(c.nbt):
                if ops.gemm4w_choose(M, N, K, out_f32=out_f32, epilogue=epi, n_cu=n_cu):
                    return "4w", None, None
        if not _off("FVQA_GEMM4W") and not _off("FVQA_GEMM4W_SK") and h16 and not out_f32 and p["full"] == 0 and 2 <= p["s"] <= 4:
            return "sk4", split, p["full"]
        return "sk256", split, p["full"]
    assert c.variant in (0, 1, 2, 12)
    if h16 and M <= 16 and K % 256 == 0 and c.variant in (0, 12) and (c.acc or not tail):
        return "skinny", None, None
    return "128", None, None


def record_names(route, kinds, c, dtype, split):
    """The launch record against the route: bit 7 = the 4-wave kernels, bit 8 = few-rows, bit 4 = split-K, bit 5 = fp32 output,
    bit 6 = fp32 input. The 128 x 128 and the skinny kernel keep no record."""
    if route in ("128", "skinny"):
        assert kinds == [], kinds
        return
    assert len(kinds) == 1, kinds
    k = kinds[0]
    assert bool(k & 32) == (c.out == "f32" or dtype == torch.float32) and bool(k & 64) == (dtype == torch.float32), kinds
    if route == "fewrows":
        assert k & 256 and not k & 128, kinds
    elif route == "4w":
        assert k & 128 and not k & 16 and not k & 256, kinds
    elif route == "sk4":
        assert k & 128 and k & 16 and not k & 256, kinds
    else:
        assert route == "sk256" and not k & 128 and not k & 256 and bool(k & 16) == (split > 1), kinds


# ---------------------------------------------------------------------------------------------------------------- operands
@functools.lru_cache(maxsize=6)
def problem(family, M, N, K):
    """(A, B, fp64 product) of a family at a shape: built once, shared by every dtype and every row of the table at that shape."""
    a, b = U.operands(family, M, N, K)
    return a, b, a @ b.T


# Window offsets that keep what the entries demand: start and row pitch multiples of 16 bytes (operands: 32 elements left and right),
# C and the residual 16-byte aligned with ldc % 8 == 0 (the persistent family), the tail whole rows of a flat arena (the entry
# takes a contiguous tail). (rows above, below), (columns left, right): every window is interior, none ends its allocation.
PADS = dict(ab=((2, 3), (32, 32)), c=((2, 3), (16, 16)), tail=((2, 2), (0, 0)))


class Run:
    """One table row at one dtype, family and layout ("win": windows in poisoned arenas; "contig": contiguous tensors)."""

    def __init__(self, c, dtype, family, layout):
        _lib.load(dtype)                                   # before any gemm4w_width block: it forces every library loaded
        self.c, self.dt, self.family, self.layout = c, dtype, family, layout
        M, N, K = c.M, c.N, c.K
        a, b, ref = problem(family, M, N, K)
        self.odt = torch.float32 if c.out == "f32" else dtype
        win = layout == "win"
        p = PADS
        zero = ((0, 0), (0, 0))
        self.a_ar, self.a = windowed(a.to(dtype).to(DEV), *(p["ab"] if win else zero), NAN)
        self.b_ar, self.b = windowed(b.to(dtype).to(DEV), *(p["ab"] if win else zero), NAN)
        self.a0, self.b0 = self.a_ar.clone(), self.b_ar.clone()
        self.cpad = p["c"] if win else zero
        self.tpad = p["tail"] if win else zero
        rows_c = M if c.m_split is None else c.m_split
        self.rows_c = 0 if c.acc else rows_c
        want = ref[:rows_c]
        self.r_ar = self.r = self.r0 = None
        if c.resid:
            r = U.residual_ints(rows_c, N, c.id)
            want = want + r
            self.r_ar, self.r = windowed(r.to(dtype).to(DEV), *self.cpad, SENT)
            self.r0 = self.r_ar.clone()
        self.want_c = None if c.acc else want.to(self.odt)
        assert c.acc or torch.equal(self.want_c.double(), want)                      # the cast rounds nothing
        self.want_t = self.t_init = None
        if c.acc or c.m_split is not None:
            rows_t = M - (0 if c.acc else c.m_split)
            self.t_init = U.residual_ints(rows_t, N, (c.id, "tail")).float()
            self.want_t = (self.t_init.double() + ref[M - rows_t:]).float()
            assert torch.equal(self.want_t.double(), self.t_init.double() + ref[M - rows_t:])

    def targets(self):
        """Fresh output: (C arena, C window) — NaN inside, the sentinel around — and the same for the tail, prefilled."""
        c, N = self.c, self.c.N
        c_ar = c_v = t_ar = t_v = None
        if not c.acc:
            c_ar, c_v = windowed(torch.full((self.rows_c, N), NAN, dtype=self.odt, device=DEV), *self.cpad, SENT)
            assert self.r is None or self.r.stride(0) == c_v.stride(0)
        if self.t_init is not None:
            t_ar, t_v = windowed(self.t_init.to(DEV), *self.tpad, SENT)
            assert t_v.is_contiguous()
        return c_ar, c_v, t_ar, t_v

    def launch(self, c_v, t_v):
        c = self.c
        with ops.gemm4w_width(c.nbt):
            ops.gemm_nt(self.a, self.b, c_v, residual=self.r, tail=t_v, m_split=0 if c.acc else (c.m_split or 0),
                        variant=c.variant)

    def check(self, c_ar, c_v, t_ar, t_v):
        pairs = [(self.a_ar.cpu(), self.a0.cpu()), (self.b_ar.cpu(), self.b0.cpu())]
        if self.r_ar is not None:
            pairs.append((self.r_ar.cpu(), self.r0.cpu()))
        if c_ar is not None:
            check_exact(c_ar.cpu(), c_v, self.want_c, SENT, pairs)
            pairs = ()
        if t_ar is not None:
            check_exact(t_ar.cpu(), t_v, self.want_t, SENT, pairs)


def workspace_word():
    return int(ops.gemm_workspace(torch.device(DEV, torch.cuda.current_device()), 8)[:8].view(torch.int64)[0])


def run_case(c, dtype, route, split):
    """Every family of the row, windowed (and contiguous where the row says so): the launch record names `route`; check_exact;
    error word and the workspace's first word clear; a second launch into fresh targets gives equal bits."""
    for family in c.families():
        for layout in ("win", "contig") if c.contig else ("win",):
            what = (c.id, str(dtype), family, layout)
            run = Run(c, dtype, family, layout)
            first = run.targets()
            kinds = _kinds_of(lambda: run.launch(first[1], first[3]))
            record_names(route, kinds, c, dtype, split)
            try:
                run.check(*first)
            except AssertionError as e:
                raise AssertionError(f"{what}: {e}") from None
            assert ops.gemm_error() == 0 and workspace_word() == 0, what
            again = run.targets()
            run.launch(again[1], again[3])
            for x, y in ((first[0], again[0]), (first[2], again[2])):
                assert x is None or torch.equal(U.bits(x), U.bits(y)), what
            assert ops.gemm_error() == 0 and workspace_word() == 0, what


# --------------------------------------------------------------------------------------------------------------------- tests
@pytest.mark.parametrize("c,dtype", PARAMS)
def test_case_takes_the_route_it_names(c, dtype):
    """Host only (no launch): the dispatch's own rules put every row of the table on the kernel, the split and the number of
    whole rounds it names, so that a row cannot drift to another route while its id still names the old one."""
    route, split, full = predict(c, dtype, _cus())
    assert route == c.route, (route, split, full)
    if c.s is not None:
        assert (split, full) == (c.s, c.full), (split, full)


@pytest.mark.parametrize("c,dtype", PARAMS)
def test_product_is_exact_word_for_word(c, dtype):
    """Every row: the window equals the fp64 product (+ residual; the tail: + what it held), every word around it and every
    operand word is untouched, the launch record names the route, the error words are clear, a second launch gives equal bits."""
    route, split, full = predict(c, dtype, _cus())
    assert route == c.route and (c.s is None or (split, full) == (c.s, c.full)), (route, split, full)
    run_case(c, dtype, route, split)


def test_control_plain_matmul_of_the_same_operands_is_exact():
    """The assumption under every assertion here, measured apart from this project's kernels: torch.matmul on the device, in
    the storage type, returns the fp64 product of SA / SB operands exactly (and of DN in fp32)."""
    for family, dtype in (("SA", torch.bfloat16), ("SB", torch.float16), ("SB", torch.bfloat16), ("DN", torch.float32)):
        a, b, ref = problem(family, 520, 4088, 2048)
        got = torch.matmul(a.to(dtype).to(DEV), b.to(dtype).to(DEV).T)
        assert torch.equal(got.double().cpu(), ref), (family, dtype)


# -------------------------------------------------------------------------------------------------------- SwiGLU forward
BIAS_K = 64                                                # one more stage of K: x = 1 against W1 = 2 there, a += 128
SWIGLU = [
    # (id, dtypes, st, M, Hf, K, route, pieces, nbt): N = 2 Hf columns in the AB16 layout
    ("ab_sk256_f32", U.ONLY32, False, 300, 272, 256, "sk256", 1, None),         # the 8-wave kernel, fp32 build: ragged M and N
    ("ab_sk256_f32_mgroups", U.ONLY32, False, 2100, 144, 64, "sk256", 1, None),  # 9 m tiles in 2 groups
    ("ab_sk256_h16_ragged", U.H16, False, 1034, 1520, 320, "sk256", 1, None),   # 16-bit, whole tiles, ragged both ways
    ("ab_sk256_h16_split_k", U.H16, False, 1024, 144, 4096, "sk256", 8, None),  # a split-K tile set: 2 n tiles x 4 m tiles
    ("st_4w_w12", U.H16, True, 1034, 1520, 320 + BIAS_K, "4w", 1, 12),          # the 4-wave kernel at its even widths
    ("st_4w_w14", U.H16, True, 1034, 1520, 320 + BIAS_K, "4w", 1, 14),
    ("st_4w_w16", U.H16, True, 1034, 1520, 320 + BIAS_K, "4w", 1, 16),
    ("st_fewrows", U.H16, True, 33, 2048, 4096 + BIAS_K, "fewrows", 1, None),
    ("st_sk256_f32", U.ONLY32, True, 300, 272, 256 + BIAS_K, "sk256", 1, None),
]
SWIGLU_PARAMS = [pytest.param(*row, d, id=f"{row[0]}-{str(d)[6:]}") for row in SWIGLU for d in row[1] if d in DTYPES]


@functools.lru_cache(maxsize=4)
def swiglu_problem(family, st, M, Hf, K):
    """(x, w13, fp64 product in the AB16 layout). st: sparse rows of 64 non-zeros (|a|, |b| <= 64) and BIAS_K more k at which x
    is 1, the W1 rows 2 and the W3 rows 0, so that every a lies in [64, 192] and b in [-64, 64] whatever the order of summation."""
    if not st:
        return problem(family, M, 2 * Hf, K)
    K0 = K - BIAS_K
    sparse, dense = U.sparse_operand, U.dense_operand
    sx, sw = U.seed_of("swiglu", family, "x", M, Hf, K), U.seed_of("swiglu", family, "w", M, Hf, K)
    x0 = sparse(M, K0, sx, nnz=64) if family == "SA" else dense(M, K0, sx)
    w0 = dense(2 * Hf, K0, sw) if family == "SA" else sparse(2 * Hf, K0, sw, nnz=64)
    x = torch.cat([x0, torch.ones(M, BIAS_K, dtype=torch.float64)], dim=1)
    w1_rows = (torch.arange(2 * Hf) % 32 < 16).double()[:, None]                     # AB16: 16 rows of W1, 16 of W3, ...
    w = torch.cat([w0, 2 * w1_rows.expand(2 * Hf, BIAS_K)], dim=1)
    return x, w, x @ w.T


@pytest.mark.parametrize("cid,dtypes,st,M,Hf,K,route,pieces,nbt,dtype", SWIGLU_PARAMS)
def test_swiglu_forward_stores_the_exact_products(cid, dtypes, st, M, Hf, K, route, pieces, nbt, dtype):
    """ops.gemm_nt_swiglu_fwd(st=False): ab = x (W1 | W3)^T in the AB16 layout is a plain product, so on SA / SB operands it is
    the fp64 product word for word; z = silu(a) * b keeps the bound of test_gemm_nt_swiglu_fwd_epilogue. That epilogue lives in
    gemm_sk_256 alone (fvqa_gemm4w_choose refuses it): fp32 build, 16-bit whole tiles, a split-K tile set.

    The 4-wave kernel and the few-rows kernels carry the form that stores s = silu(a), t = b sigma(a) (1 + a (1 - sigma(a)))
    (st=True). With every a >= 64, exp(-a) < 2^-92 vanishes beside 1 in fp32, sigma(a) is 1 exactly, s = a and t = b: the stored
    words are again the plain product, and z = a b rounded once to the storage type — all three exact."""
    _lib.load(dtype)
    cus = _cus()
    p = _plan(M, 2 * Hf, K, dtype, cus)
    epi = 5 if st else 4                                   # FVQA_EPI_SWIGLU_FWD_ST / FVQA_EPI_SWIGLU_FWD (include/fvqa.h)
    with ops.gemm4w_width(nbt):
        takes4w = dtype != torch.float32 and not (p["full"] == 0 and p["s"] > 1) and ops.gemm4w_choose(M, 2 * Hf, K, epilogue=epi, n_cu=cus)
    few = st and dtype != torch.float32 and 16 < M <= 64 and 2 * Hf * K >= 1 << 24 and not _off("FVQA_FEWROWS")
    assert ("fewrows" if few else "4w" if takes4w else "sk256") == route and (route != "sk256" or (p["s"] if p["rem"] else 1) == pieces)
    for family in ("SA", "SB"):
        x, w13, ref = swiglu_problem(family, st, M, Hf, K)         # w13: its rows already interleaved in 16-blocks
        a_ref, b_ref = ops.unpack_ab16(ref)
        assert not st or (float(a_ref.min()) >= 64 and float(a_ref.max()) <= 192 and float(b_ref.abs().max()) <= 64)
        ab = torch.full((M + 2, 2 * Hf), SENT, dtype=dtype, device=DEV)
        z = torch.full((M + 2, Hf), SENT, dtype=dtype, device=DEV)
        ab[1:M + 1], z[1:M + 1] = NAN, NAN
        xd, wd = dev(x.to(dtype)), dev(w13.to(dtype))
        with ops.gemm4w_width(nbt):
            kinds = _kinds_of(lambda: ops.gemm_nt_swiglu_fwd(xd, wd, ab[1:M + 1], z[1:M + 1], st=st))
        assert len(kinds) == 1, kinds
        k = kinds[0]
        if route == "sk256":
            assert not k & 128 and not k & 256 and bool(k & 16) == (pieces > 1), kinds
        else:
            assert k & (128 if route == "4w" else 256) and not k & 16, kinds
        check_exact(ab.cpu(), ab[1:M + 1], ref.to(dtype), SENT, [(xd.cpu(), x.to(dtype)), (wd.cpu(), w13.to(dtype))])
        if st:
            check_exact(z.cpu(), z[1:M + 1], (a_ref * b_ref).to(dtype), SENT)
        else:
            zc = z.cpu()
            assert rel(zc[1:M + 1], ref_cpu.silu(a_ref) * b_ref) < tol(dtype, 5e-5, 2e-2), family
            assert bool((zc[0] == SENT).all()) and bool((zc[M + 1] == SENT).all())
        assert ops.gemm_error() == 0 and workspace_word() == 0


# ------------------------------------------------------------------------------------------------------- the switched builds
def _rows(pred):
    return [c for c in CASES if pred(c)]


SWITCHED = {
    # 16-bit whole-tile rows and split-2 / split-4 rows, all on gemm_sk_256 (24-bit slabs where the output is 16-bit)
    "FVQA_GEMM4W": _rows(lambda c: c.route == "sk4" or (c.route == "4w" and c.nbt == 16)),
    # the split rows on gemm_sk_256 while whole tiles stay on the 4-wave kernel
    "FVQA_GEMM4W_SK": _rows(lambda c: c.route == "sk4" or (c.route == "4w" and c.nbt == 13 and c.K == 320)),
    # the few-rows rows on the tile kernels
    "FVQA_FEWROWS": _rows(lambda c: c.route == "fewrows"),
}


def child_rows(switch):
    """In a child started with `switch`=0: the rows it re-routes, on the route the same host rules name with that kernel ruled
    out — which must be another kernel than the row's own wherever the switch bears on it."""
    assert _off(switch)
    n = 0
    for c in SWITCHED[switch]:
        for d in c.dtypes:
            route, split, full = predict(c, d, _cus())
            if switch == "FVQA_GEMM4W":
                assert route == "sk256", (c.id, route)
            elif switch == "FVQA_GEMM4W_SK":
                assert route == ("4w" if c.route == "4w" else "sk256") and (c.route == "4w" or split == c.s), (c.id, route, split)
            else:
                assert route in ("sk256", "4w", "sk4"), (c.id, route)
            run_case(c, d, route, split)
            print(f"{c.id}-{str(d)[6:]}: {route} split {split} full {full}")
            n += 1
    print(n, "rows")


@pytest.mark.parametrize("switch", sorted(SWITCHED))
def test_rows_behind_a_switch_are_exact_too(switch):
    """FVQA_GEMM4W=0, FVQA_GEMM4W_SK=0, FVQA_FEWROWS=0 (the A/B switches the project ships; each read once per process): a child
    process per setting runs the rows that setting re-routes through the same checks."""
    torch.cuda.synchronize()                               # (the persistent kernel wants the device to itself while it runs)
    env = dict(os.environ, FVQA_SYNTHETIC_TOKENIZER="1", **{switch: "0"},
               PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "flipped-vqa_amd"), os.environ.get("PYTHONPATH", "")]))
    code = f"import tests.test_gemm_exact_gpu as T\nT.child_rows({switch!r})\n"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (switch, r.returncode, (r.stdout + r.stderr)[-3000:])
    print(r.stdout[-3000:])
    assert f"{sum(len(c.dtypes) for c in SWITCHED[switch])} rows" in r.stdout
