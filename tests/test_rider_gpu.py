"""The GEMM riders (include/fvqa.h fvqa_sk_rider): a second product of <= 16 rows that runs on the compute units a projection
launch leaves idle, or as a launch of its own right after it. The step puts the adapter K/V rows of llama/model.py:98-100 there
(overwritten, storage dtype) and the adapter-query gradient rows (added to the fp32 gradient). Every route the rider can take is
pinned here against fp64 and against the stand-alone kernel, bit for bit (the header's promise: the same arithmetic wherever it
runs):

  dma    4-wave whole-tile kernel (gemm4w_k), light workgroups, operands by LDS-DMA (gemm_skinny.h skinny_strip2_dma_4w)
  reg    the same with register strips (skinny_strip2_4w: K2 % 512 != 0)
  sk4    4-wave split-K kernel (gemm4w_sk_k), rider workgroups appended to the grid (skinny_strip2_4w)
  sk256  8-wave persistent kernel (gemm_sk_256), rider workgroups appended to the grid (skinny_strip)
  own    a launch of its own after the main product (gemm_nt_skinny, or gemm_nt_128 for K2 % 256 != 0 and the fp32 build)

Each case names its route; the host's own partition and width functions must predict it, the launch record (_kinds_of) must
name the main kernel, and a kernel trace must show a rider kernel exactly when the rider ran on its own. FVQA_RIDER and
FVQA_RIDER_DMA are read once per process: the cross-route checks run in child processes. Run with -m gpu."""
import math
import os
import subprocess
import sys
import zlib

import pytest
import torch

pytestmark = pytest.mark.gpu

from fvqa import _lib, ops  # noqa: E402
from oracle import ref_cpu  # noqa: E402
from tests.test_kernels_gpu import DEV, DTYPES, _kinds_of, dev, rel, rnd  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H16 = [d for d in DTYPES if d != torch.float32]            # bf16 (libfvqa_hip.so), fp16 (libfvqa_hip_f16.so)
F32 = [torch.float32]
SENT = -7.25                                               # what the words around a rider's block hold (exact in every dtype)
EPI = {"none": 0, "residual": 1, "swiglu": 3, "swiglu_st": 6, "swiglu_fwd": 5, "rope": 7}
IN_LAUNCH = ("dma", "reg", "sk4", "sk256")
MAIN_KERNEL = {"4w": "gemm4w_k", "sk4": "gemm4w_sk_k", "sk256": "gemm_sk_256", "128": "gemm_nt_128"}
KERNELS = ("gemm4w_k", "gemm4w_sk_k", "gemm_sk_256", "gemm_nt_128", "gemm_nt_skinny")


class Case:
    """One rider call. entry: "rider" (ops.gemm_nt_rider, epilogue `epi`), "swiglu_fwd" (ops.gemm_nt_swiglu_fwd, st=True) or
    "rope" (ops.gemm_nt_rope). M, N, K: the main product as the C entry sees it (swiglu*: N = hidden, the output has 2N columns;
    rope: M = n_seq * S, N = 3 * D). route / main: where the rider runs and which kernel takes the main product. nbt: the
    4-wave tile width forced on both calls of a comparison (None where no 4-wave kernel is involved)."""

    def __init__(self, cid, entry, route, main, M, N, K, M2, N2, K2, *, epi="none", acc=False, nbt=None, dtypes=H16,
                 n_cu=None, rope=None):
        self.id, self.entry, self.route, self.main = cid, entry, route, main
        self.M, self.N, self.K, self.M2, self.N2, self.K2 = M, N, K, M2, N2, K2
        self.epi = {"swiglu_fwd": "swiglu_fwd", "rope": "rope"}.get(entry, epi)
        self.acc, self.nbt, self.dtypes, self.n_cu, self.rope = acc, nbt, dtypes, n_cu, rope
        self.seed = zlib.crc32(cid.encode()) % 100000

    def gemm_n(self):                                      # N of the GEMM the kernel runs
        return 2 * self.N if self.entry == "swiglu_fwd" else self.N

    def __repr__(self):
        return self.id


# Shapes were placed with fvqa_gemm_sk_describe / fvqa_gemm4w_choose on 256 CUs (test_case_routes_are_what_the_host_predicts
# re-derives every one). Rider rows M2 in {1, 10, 16}; N2 with an even strip count (% 32 == 0), an odd one (% 32 == 16) and
# ragged (% 16 != 0); K2 of one, two and eight DMA stages (512, 1024, 4096) and the step's backward 8192.
CASES = [
    # 4-wave kernel, LDS-DMA strips
    Case("dma_one_round_many_light", "rider", "dma", "4w", 1034, 3000, 320, 1, 1000, 512, nbt=16),            # 60 tiles, 196 light
    Case("dma_one_round_acc", "rider", "dma", "4w", 1034, 3000, 320, 16, 1040, 1024, acc=True, nbt=14),
    Case("dma_few_light_passes", "rider", "dma", "4w", 1024, 15360, 128, 10, 2064, 4096, epi="residual", acc=True,
         nbt=16),                                                                                               # 240 tiles: 16 light x 5 passes
    Case("dma_w2t_step_like", "rider", "dma", "4w", 1024, 11008, 128, 10, 4096, 8192, epi="swiglu_st", acc=True,
         nbt=12),                                                                                               # 232 tiles: 24 light x 6 passes
    Case("dma_multi_round", "rider", "dma", "4w", 1024, 19200, 64, 16, 8200, 1024, epi="swiglu_st", nbt=16),  # 300 tiles: 2 rounds, 212 light
    Case("dma_w13_multi_round", "swiglu_fwd", "dma", "4w", 1024, 11008, 128, 10, 8192, 4096, nbt=12),         # 460 tiles, 52 light
    Case("dma_rope", "rope", "dma", "4w", 600, 1536, 512, 10, 1024, 512, nbt=16, rope=(3, 200, 4)),
    # the 8-light boundary: 248 tiles of 256 columns ride, 249 do not
    Case("dma_8_light", "rider", "dma", "4w", 256, 248 * 256, 64, 10, 528, 512, nbt=16, n_cu=256),
    Case("own_7_light", "rider", "own", "4w", 256, 249 * 256, 64, 10, 528, 512, nbt=16, n_cu=256),
    # 4-wave kernel, register strips (K2 % 512 != 0)
    Case("reg_k768", "rider", "reg", "4w", 512, 4000, 256, 10, 1536, 768, epi="residual", acc=True, nbt=13),
    Case("reg_k1280_rope", "rope", "reg", "4w", 600, 1536, 512, 16, 1000, 1280, nbt=12, rope=(3, 200, 4)),
    Case("reg_k768_w13", "swiglu_fwd", "reg", "4w", 512, 1536, 256, 1, 2064, 768, nbt=16),
    # 4-wave split-K kernel: (512, 1024, 1024) = 8 tiles x 2 pieces, 240 idle CUs
    Case("sk4_split2", "rider", "sk4", "sk4", 512, 1024, 1024, 16, 4112, 1024, acc=True),
    Case("sk4_split2_residual", "rider", "sk4", "sk4", 512, 1024, 1024, 1, 1000, 512, epi="residual"),
    # 8-wave kernel: an epilogue the 4-wave kernels lack (SwiGLU' on (a, b)), and a split of 8
    Case("sk256_swiglu_bwd", "rider", "sk256", "sk256", 1024, 1536, 512, 10, 1992, 512, epi="swiglu", acc=True),
    Case("sk256_split8", "rider", "sk256", "sk256", 256, 2048, 4096, 1, 4096, 4096),
    # the idle boundary: 240 whole tiles leave 16 CUs and ride, 241 leave 15 and do not
    Case("sk256_16_idle", "rider", "sk256", "sk256", 256, 61440, 256, 10, 1040, 1024, epi="swiglu", n_cu=256),
    Case("own_15_idle", "rider", "own", "sk256", 256, 61696, 256, 10, 1040, 1024, epi="swiglu", n_cu=256),
    # own launches
    Case("own_no_light_qkv", "rope", "own", "4w", 1024, 12288, 512, 10, 8192, 512, nbt=12, rope=(8, 128, 32)),  # 256 tiles
    Case("own_few_rows", "rider", "own", "128", 100, 1024, 512, 10, 1040, 512, acc=True),
    Case("own_k320", "rider", "own", "4w", 512, 2048, 256, 10, 1000, 320, epi="residual", nbt=16),
    Case("own_k320_acc", "rider", "own", "4w", 512, 2048, 256, 16, 1000, 320, acc=True, nbt=16),
    Case("own_k320_w13", "swiglu_fwd", "own", "4w", 512, 1536, 256, 10, 1024, 320, nbt=16),
    Case("own_f32", "rider", "own", "sk256", 512, 1024, 256, 10, 1000, 512, acc=True, dtypes=F32),
    Case("own_f32_store", "rider", "own", "sk256", 512, 1024, 256, 16, 1040, 256, epi="residual", dtypes=F32),
    Case("own_f32_w13", "swiglu_fwd", "own", "sk256", 256, 768, 256, 10, 1024, 512, dtypes=F32),
]
BOUNDARY = {"dma_8_light": 8, "own_7_light": 7, "sk256_16_idle": 16, "own_15_idle": 15}     # light workgroups / idle CUs
BY_ID = {c.id: c for c in CASES}
PARAMS = [pytest.param(c, d, id=f"{c.id}-{str(d)[6:]}") for c in CASES for d in c.dtypes]


def _cus():
    return int(torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count)


def _plan(M, N, K, dtype, n_cu):
    import ctypes as C
    plan = (C.c_int32 * 12)()
    code = _lib.F32 if dtype == torch.float32 else _lib.BF16           # (the host-only partition is the same in both 16-bit builds)
    assert _lib.load().fvqa_gemm_sk_describe(M, N, K, code, n_cu, C.cast(plan, C.c_void_p), -1, None, 0) == 0
    return dict(zip(("tm", "tn", "nw_tile", "gran", "gpt", "ts", "mgroups", "n_teams", "full", "rem", "s", "pstride"), plan))


def predict(c, dtype, n_cu):
    """(route, main kernel, light workgroups or idle CUs) by the host functions the dispatch itself uses (csrc/gemm.hip
    fvqa_gemm_nt_rider, gemm_sk.hip fvqa_gemm_sk_impl, gemm4w.hip fvqa_gemm4w_impl), for this process's FVQA_RIDER_DMA."""
    M, N, K = c.M, c.gemm_n(), c.K
    epi, h16 = EPI[c.epi], dtype != torch.float32
    cus = min(n_cu, 256)
    fits = 1 <= c.M2 <= 16 and c.K2 % 256 == 0
    if c.entry == "rider" and not (M >= 192 and N >= 256) and epi not in (3, 6):
        assert N < 256 or not (M > 16 and N * K >= 1 << 24)          # fvqa_gemm_nt's 128 x 128 kernel, not the persistent one
        return "own", "128", 0
    if h16:
        p0 = _plan(M, N, K, dtype, cus)
        if not (p0["full"] == 0 and p0["s"] > 1):
            with ops.gemm4w_width(c.nbt):
                nbt = ops.gemm4w_choose(M, N, K, epilogue=epi, rider_nk=(c.N2, c.K2), n_cu=cus)
            if nbt:
                tiles = -(-M // 256) * -(-N // (16 * nbt))
                rounds = -(-tiles // cus)
                light = cus - (tiles - (rounds - 1) * cus)
                if fits and light >= 8:
                    dma = os.environ.get("FVQA_RIDER_DMA", "1")[:1] != "0" and (c.K2 // 8) % 64 == 0
                    return ("dma" if dma else "reg"), "4w", light
                return "own", "4w", light
    p = _plan(M, N, K, dtype, cus)
    idle = cus - p["n_teams"] * p["ts"]
    main = "sk4" if h16 and p["full"] == 0 and 2 <= p["s"] <= 4 and epi in (0, 1) else "sk256"
    if h16 and idle >= 16 and fits:
        return main, main, idle
    return "own", main, idle


def _need_cus(c):
    if c.n_cu is not None and _cus() != c.n_cu:
        pytest.skip(f"boundary case placed for {c.n_cu} CUs; this device has {_cus()}")


# ------------------------------------------------------------------------------------------------------------------ one call
class Run:
    """Operands of a case (seeded, CPU copies for the fp64 references) and the calls on them."""

    def __init__(self, c, dtype):
        _lib.load(dtype)                                   # before any gemm4w_width block: it forces every library loaded
        self.c, self.dt = c, dtype
        s, M, N, K, dt = c.seed, c.M, c.N, c.K, dtype
        if c.entry == "rider" and c.epi in ("none", "residual"):
            self.a, self.b = rnd(M, K, dtype=dt, seed=s), rnd(N, K, dtype=dt, scale=1 / math.sqrt(K), seed=s + 1)
            self.r = rnd(M, N, dtype=dt, seed=s + 2) if c.epi == "residual" else None
        elif c.entry == "rider":                           # dH W2^T with SwiGLU' (on (a, b), or on the saved (s, t))
            self.a, self.b = rnd(M, K, dtype=dt, seed=s), rnd(N, K, dtype=dt, scale=1 / math.sqrt(K), seed=s + 1)
            x, y = rnd(M, N, dtype=dt, scale=3, seed=s + 2).double(), rnd(M, N, dtype=dt, scale=3, seed=s + 3).double()
            if c.epi == "swiglu":
                self.ea, self.eb = x.to(dt), y.to(dt)
            else:
                sg = torch.sigmoid(x)
                self.ea, self.eb = (x * sg).to(dt), (y * sg * (1 + x * (1 - sg))).to(dt)        # (s, t)
            self.r = ops.pack_ab16(self.ea, self.eb)
        elif c.entry == "swiglu_fwd":
            self.a = rnd(M, K, dtype=dt, seed=s)
            self.w1 = rnd(N, K, dtype=dt, scale=2 / math.sqrt(K), seed=s + 1)
            self.w3 = rnd(N, K, dtype=dt, scale=2 / math.sqrt(K), seed=s + 2)
            self.b = ops.pack_ab16(self.w1.T.contiguous(), self.w3.T.contiguous()).T.contiguous()
        else:
            n_seq, S, H = c.rope
            assert n_seq * S == M and 3 * H * 128 == N
            self.a, self.b = rnd(M, K, dtype=dt, seed=s), rnd(N, K, dtype=dt, scale=1 / math.sqrt(K), seed=s + 1)
            self.cos, self.sin = ref_cpu.rope_tables(2 * S, 128, torch.float32)
            self.tables = (dev(self.cos), dev(self.sin))
        self.ad, self.bd = dev(self.a), dev(self.b)
        self.rd = dev(self.r) if getattr(self, "r", None) is not None else None
        # the rider's operands as the step lays them out: column blocks of wider matrices (lda, ldb != K2)
        M2, N2, K2 = c.M2, c.N2, c.K2
        wa, wb = rnd(M2, K2 + 64, dtype=dt, seed=s + 5), rnd(N2, K2 + 128, dtype=dt, scale=1 / math.sqrt(K2), seed=s + 6)
        self.ra, self.rb = wa[:, 32:32 + K2], wb[:, 64:64 + K2]
        self.rad, self.rbd = dev(wa)[:, 32:32 + K2], dev(wb)[:, 64:64 + K2]
        assert self.rad.stride(0) == K2 + 64 and self.rbd.stride(0) == K2 + 128
        self.base = rnd(M2, N2, seed=s + 7).float() if c.acc else None     # of the product's magnitude

    def rider_target(self):
        """-> (view the rider writes, the buffer around it). Storage-dtype rider: a block of a wider buffer (ldc = N2 + 48, rows
        above and below), NaN inside so that every word must be written, SENT around it. fp32 accumulate (ldc must be N2): rows
        of a flat buffer, SENT above and below, the non-zero base inside."""
        c = self.c
        M2, N2 = c.M2, c.N2
        if c.acc:
            buf = torch.full(((M2 + 4) * N2,), SENT, dtype=torch.float32, device=DEV)
            view = buf[2 * N2:(2 + M2) * N2].view(M2, N2)
            view.copy_(self.base)
        else:
            buf = torch.full((M2 + 3, N2 + 48), SENT, dtype=self.dt, device=DEV)
            view = buf[2:2 + M2, 16:16 + N2]
            view.fill_(float("nan"))
            assert view.stride(0) == N2 + 48
        return view, buf

    def main_buffers(self):
        c, M, N = self.c, self.c.M, self.c.N
        nan = float("nan")
        if c.entry == "swiglu_fwd":
            return [torch.full((M, 2 * N), nan, dtype=self.dt, device=DEV), torch.full((M, N), nan, dtype=self.dt, device=DEV)]
        cols = 2 * N if c.epi in ("swiglu", "swiglu_st") else N
        return [torch.full((M, cols), nan, dtype=self.dt, device=DEV)]

    def call(self, outs, target=None):
        """The entry of the case into `outs`; with target: the rider into it, else the same main call without a rider."""
        c = self.c
        rk = {} if target is None else dict(rider_a=self.rad, rider_b=self.rbd, rider_out=target)
        with ops.gemm4w_width(c.nbt):
            if c.entry == "swiglu_fwd":
                ops.gemm_nt_swiglu_fwd(self.ad, self.bd, outs[0], outs[1], st=True, **rk)
            elif c.entry == "rope":
                n_seq, S, H = c.rope
                ops.gemm_nt_rope(self.ad, self.bd, outs[0], self.tables, S, 128, H, **rk)
            elif target is not None:
                sw = dict(swiglu_ab=self.rd, swiglu_st=c.epi == "swiglu_st") if c.epi.startswith("swiglu") else {}
                ops.gemm_nt_rider(self.ad, self.bd, outs[0], residual=self.rd if c.epi == "residual" else None,
                                  accumulate=c.acc, **sw, **rk)
            elif c.epi.startswith("swiglu"):
                ops.gemm_nt_swiglu_bwd(self.ad, self.bd, self.rd, outs[0], st=c.epi == "swiglu_st")
            else:
                ops.gemm_nt(self.ad, self.bd, outs[0], residual=self.rd)

    def standalone(self, init=None):
        """The rider's product by the stand-alone kernel: fvqa_gemm_nt into a fresh buffer, or (accumulate) into the fp32 rows
        every row of which it adds to, starting from `init` (default: the base)."""
        if self.c.acc:
            t = (self.base.to(DEV) if init is None else init).clone().contiguous()
            ops.gemm_nt(self.rad, self.rbd, None, tail=t, m_split=0)
            return t
        o = torch.full((self.c.M2, self.c.N2), float("nan"), dtype=self.dt, device=DEV)
        ops.gemm_nt(self.rad, self.rbd, o)
        return o


def outputs(c, dtype):
    """Main outputs and rider block of one call with a rider (the cross-process comparisons): CPU tensors."""
    run = Run(c, dtype)
    outs, (view, _) = run.main_buffers(), run.rider_target()
    run.call(outs, view)
    torch.cuda.synchronize()
    return [o.cpu() for o in outs] + [view.cpu()]


def _trace(fn):
    """Names of the GEMM kernels fn() launches, in launch order (torch.profiler with device activity: kineto sees every kernel of
    the process, this library's included)."""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    evs = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    evs.sort(key=lambda e: e.time_range.start)
    names = []
    for e in evs:
        for k in KERNELS:
            if k in e.name:
                names.append(k)
    return names


def _main_refs(run):
    """(output index, selection, fp64 reference, bound) of the main outputs; bounds of tests/test_kernels_gpu.py per epilogue."""
    c, dt = run.c, run.dt
    f32 = dt == torch.float32
    lo = lambda v16, v32=5e-5: v32 if f32 else v16                     # noqa: E731
    if c.entry == "swiglu_fwd":
        a_, b_ = run.a.double() @ run.w1.double().T, run.a.double() @ run.w3.double().T
        sg = torch.sigmoid(a_)
        s_ref, t_ref = a_ * sg, b_ * sg * (1 + a_ * (1 - sg))
        return [(0, lambda o: ops.unpack_ab16(o)[0], s_ref, lo(1e-2)), (0, lambda o: ops.unpack_ab16(o)[1], t_ref, lo(1e-2)),
                (1, None, s_ref * b_, lo(2e-2))]
    p = run.a.double() @ run.b.double().T
    if c.entry == "rope":
        n_seq, S, H = c.rope
        D = H * 128
        raw = p.to(dt).double()                            # the epilogue rotates the rounded product
        qk = ref_cpu.rope_apply(raw[:, :2 * D].reshape(n_seq, S, 2 * H, 128), run.cos[:S].double(),
                                run.sin[:S].double()).reshape(c.M, 2 * D)
        return [(0, lambda o: o[:, :2 * D], qk, 1e-2), (0, lambda o: o[:, 2 * D:], raw[:, 2 * D:], 1e-2)]
    if c.epi == "swiglu":
        da, db = ref_cpu.swiglu_bwd(p, run.ea.double(), run.eb.double())
        return [(0, lambda o: ops.unpack_ab16(o)[0], da, lo(1e-2)), (0, lambda o: ops.unpack_ab16(o)[1], db, lo(1e-2))]
    if c.epi == "swiglu_st":
        return [(0, lambda o: ops.unpack_ab16(o)[0], p * run.eb.double(), lo(1e-2)),
                (0, lambda o: ops.unpack_ab16(o)[1], p * run.ea.double(), lo(1e-2))]
    return [(0, None, p + (run.r.double() if run.r is not None else 0), lo(1e-2))]


# --------------------------------------------------------------------------------------------------------------------- tests
@pytest.mark.parametrize("c,dtype", PARAMS)
def test_case_routes_are_what_the_host_predicts(c, dtype):
    """Host only (no launch): the partition and width functions the dispatch uses put every case on its intended route — the two
    boundaries on either side — so that a case cannot drift to another route while its id still names the old one."""
    _need_cus(c)
    route, main, spare = predict(c, dtype, _cus())
    assert (route, main) == (c.route, c.main), (route, main, spare)
    assert spare == BOUNDARY.get(c.id, spare), spare


@pytest.mark.parametrize("c,dtype", PARAMS)
def test_rider_against_fp64_and_the_standalone_kernel(c, dtype):
    """Every case: (1) main outputs against fp64 with their epilogue, every word written; (2) the rider's block against fp64
    (accumulate: base + product, then base + 2 product after a second call); (3) bitwise equal to the stand-alone kernel's
    product; (4) no word around the block moved; (5) the main outputs bitwise equal to the same call without a rider (a launch
    carrying a rider runs a full grid: the tiles go to other workgroups); (6) repeatable, error word clear. Route evidence: the
    launch record names the main kernel, and the trace shows a rider kernel after it exactly when the rider ran on its own."""
    _need_cus(c)
    assert predict(c, dtype, _cus())[:2] == (c.route, c.main)
    run = Run(c, dtype)
    own_kernel = "gemm_nt_skinny" if dtype != torch.float32 and c.K2 % 256 == 0 else "gemm_nt_128"
    outs, (view, buf) = run.main_buffers(), run.rider_target()
    names = []
    kinds = _kinds_of(lambda: names.extend(_trace(lambda: run.call(outs, view))))
    # route evidence
    main_k = MAIN_KERNEL[c.main]
    want = [main_k] + ([own_kernel] if c.route == "own" else [])
    assert names == want, (names, want)
    if c.main == "128":
        assert kinds == [], kinds                          # (the 128 x 128 kernel keeps no launch record)
    else:
        assert len(kinds) == 1, kinds
        k = kinds[0]
        assert {"4w": k & 128 and not k & 16, "sk4": k & 128 and k & 16, "sk256": not k & 128}[c.main], kinds
    # (1) main against fp64
    for o in outs:
        assert not torch.isnan(o).any()
    for i, (j, sel, ref, bound) in enumerate(_main_refs(run)):
        got = sel(outs[j]) if sel is not None else outs[j]
        assert rel(got, ref) < bound, (i, rel(got, ref))
    # (2) rider against fp64
    prod = run.ra.double() @ run.rb.double().T
    got = view.double().cpu()
    if c.acc:
        assert rel(got, run.base.double() + prod) < 2e-3
    else:
        assert not torch.isnan(got).any()
        assert rel(got, prod) < (5e-5 if dtype == torch.float32 else 1e-2)
    # (3) bitwise the stand-alone kernel
    first = view.clone()
    assert torch.equal(first, run.standalone())
    # (4) nothing around the block moved
    mask = torch.ones_like(buf, dtype=torch.bool)
    if c.acc:
        mask[2 * c.N2:(2 + c.M2) * c.N2] = False
    else:
        mask[2:2 + c.M2, 16:16 + c.N2] = False
    assert bool((buf[mask] == SENT).all())
    # (5) the main outputs bitwise equal to the call without a rider
    bare = run.main_buffers()
    run.call(bare)
    for o, b in zip(outs, bare):
        assert torch.equal(o, b)
    # (6) a second identical call: equal bits (accumulate: the stand-alone kernel's sum on the first result, and base + 2 product)
    outs2 = run.main_buffers()
    run.call(outs2, view)
    for o, o2 in zip(outs, outs2):
        assert torch.equal(o, o2)
    if c.acc:
        assert torch.equal(view, run.standalone(first))
        assert rel(view, run.base.double() + 2 * prod) < 2e-3
    else:
        assert torch.equal(view, first)
    assert bool((buf[mask] == SENT).all())
    assert ops.gemm_error() == 0


# ------------------------------------------------------------------------------------------------ the same bits on every route
def _env(**kv):
    return dict(os.environ, FVQA_SYNTHETIC_TOKENIZER="1", **kv,
                PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "flipped-vqa_amd"), os.environ.get("PYTHONPATH", "")]))


def _children(tmp_path, code, settings, timeout):
    """Start one child per setting, one after another; fail at once on a non-zero or negative return code (and start no more).
    -> {setting name: path of what it saved}."""
    torch.cuda.synchronize()                               # (the persistent kernel wants the device to itself while it runs)
    got = {}
    for name, env in settings:
        path = str(tmp_path / f"{name}.pt")
        r = subprocess.run([sys.executable, "-c", code.format(path=path)], cwd=ROOT, env=_env(**env), capture_output=True,
                           text=True, timeout=timeout)
        assert r.returncode == 0, (name, r.returncode, (r.stdout + r.stderr)[-3000:])
        print(f"[{name}]", r.stdout[-2000:])
        got[name] = path
    return got


def _in_launch_params():
    n_cu = _cus()
    return [(c, d) for c in CASES for d in c.dtypes if c.route in IN_LAUNCH and (c.n_cu is None or c.n_cu == n_cu)]


def child_kernel_outputs(path):
    res = {}
    for c, d in _in_launch_params():
        res[f"{c.id}-{d}"] = outputs(c, d)
        res[f"{c.id}-{d}-route"] = predict(c, d, _cus())[0]
    assert ops.gemm_error() == 0
    torch.save(res, path)
    print(len(res) // 2, "cases")


def test_in_launch_riders_equal_own_launch_and_register_strips(tmp_path):
    """The in-launch cases re-run in a child with FVQA_RIDER=0 (every rider a launch of its own: the stand-alone 512-thread
    kernel) and in one with FVQA_RIDER_DMA=0 (register strips where the DMA form ran), on the same seeded operands and the same
    forced tile widths: main outputs and rider blocks bitwise equal to this process's."""
    code = "import tests.test_rider_gpu as T\nT.child_kernel_outputs({path!r})\n"
    mine = {}
    for c, d in _in_launch_params():
        mine[f"{c.id}-{d}"] = outputs(c, d)
    got = _children(tmp_path, code, [("rider0", dict(FVQA_RIDER="0")), ("dma0", dict(FVQA_RIDER_DMA="0"))], 600)
    for name, path in got.items():
        theirs = torch.load(path)
        for key, want in mine.items():
            c = BY_ID[key.split("-")[0]]
            route = theirs[key + "-route"]
            if name == "dma0":
                assert route == ("reg" if c.route == "dma" else c.route), (key, route)
            for i, (a, b) in enumerate(zip(want, theirs[key])):
                assert torch.equal(a, b), (name, key, i, rel(a, b.double()))


# ------------------------------------------------------------------------------------------------------------------ step level
STEP_FORMS = [("vqa", torch.bfloat16), ("all", torch.bfloat16), ("vqa", torch.float16)]


def _step(form, dtype):
    """One training step of 7b_l2 at batch 8 with the product's tail-rows head: losses, every trainable's gradient, and the tile
    width the cost model picks for each launch of the step that carries a rider (it reads FVQA_RIDER_DMA)."""
    from fvqa import synth
    from tests.gpu_util import build_model, run_step
    cfg = synth.preset("7b_l2", batch_size=8, vaq=form == "all", qav=form == "all")
    batch = synth.make_batch(cfg, seed=0)
    model, _ = build_model(cfg, dtype)
    w = 1024.0 if dtype == torch.float16 else 1.0          # (as smoke(): the fp16 build steps under a loss scale)
    losses, grads, _, _ = run_step(model, batch, loss_weights=(w, w, w), lm_head="scored")
    eng = model._engine
    eng.check_gemm_error()
    B, S = batch["video"].shape[0], batch["text_id"]["vqa"].shape[-1]
    R, D, Hf = eng.arena(eng.n_streams * B, S).R, eng.D, eng.Hf
    n_cu = _cus()
    widths = {"w2t": ops.gemm4w_choose(R, Hf, D, epilogue=EPI["swiglu_st"] if ops.swiglu_st() else EPI["swiglu"],
                                       rider_nk=(D, 2 * D), n_cu=n_cu)}
    if ops.kv_rider_ahead(dtype):
        widths["w13"] = ops.gemm4w_choose(R, 2 * Hf, D, epilogue=EPI["swiglu_fwd"], rider_nk=(2 * D, D), n_cu=n_cu)
    else:
        widths["qkv"] = ops.gemm4w_choose(R, 3 * D, D, epilogue=EPI["rope"] if ops.rope_in_gemm(dtype) else 0,
                                          rider_nk=(2 * D, D), n_cu=n_cu)
    del model
    torch.cuda.empty_cache()
    return dict(losses=losses, grads=grads, widths=widths)


def child_step(path):
    torch.save({f"{f}-{d}": _step(f, d) for f, d in STEP_FORMS}, path)


def test_step_is_bitwise_whichever_way_the_riders_run(tmp_path):
    """7b_l2, batch 8, the product's tail-rows head, vqa only (C2's layer shapes) and vqa + vaq + qav (C3's), bf16, and fp16 on
    the first: a child with FVQA_RIDER=0 (riders as launches of their own; the width chooser sees the same rider, so only the
    rider's placement and the main grid change) gives bitwise-equal losses and gradients of every trainable, adapter_query
    included. A child with FVQA_RIDER_DMA=0 also changes the widths' cost model: bitwise where it picks the same widths (the
    widths it picks are printed either way; DMA against register strips at equal widths is pinned at kernel level above)."""
    mine = {f"{f}-{d}": _step(f, d) for f, d in STEP_FORMS}
    got = _children(tmp_path, "import tests.test_rider_gpu as T\nT.child_step({path!r})\n",
                    [("rider0", dict(FVQA_RIDER="0")), ("dma0", dict(FVQA_RIDER_DMA="0"))], 600)
    for name, path in got.items():
        theirs = torch.load(path)
        for key, want in mine.items():
            have = theirs[key]
            print(f"{name} {key}: widths {want['widths']} here, {have['widths']} there")
            if name == "rider0":
                assert have["widths"] == want["widths"], key
            elif have["widths"] != want["widths"]:
                continue                                   # another tile width: another main product, not this comparison
            assert have["losses"] == want["losses"], (name, key, have["losses"], want["losses"])
            assert sorted(have["grads"]) == sorted(want["grads"]) and any("adapter_query" in n for n in want["grads"])
            for n, g in want["grads"].items():
                assert torch.equal(g, have["grads"][n]), (name, key, n, float((g - have["grads"][n]).abs().max()))
