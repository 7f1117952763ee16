"""Tensor-level wrappers over the C ABI (include/fvqa.h): each function validates shapes, dtypes,
contiguity and device ON THE HOST before a kernel is launched (a mis-shaped operand must raise
here, never fault on the GPU), then passes raw device pointers + the current HIP stream.

PyTorch is only the owner of device memory and streams here; all arithmetic is in libfvqa_hip.so.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional

import torch

from . import _lib
from ._lib import BF16, EPI_NONE, EPI_RESIDUAL, EPI_SWIGLU_BWD, EPI_SWIGLU_BWD_ST, F16, F32

_DT = {torch.float32: F32, torch.bfloat16: BF16, torch.float16: F16}
_DTN = {torch.float32: "f32", torch.bfloat16: "bf16", torch.float16: "f16"}

def dt_code(dtype: torch.dtype) -> int:
    try:
        return _DT[dtype]
    except KeyError:
        raise TypeError(f"storage dtype must be float32, bfloat16 or float16, got {dtype}") from None


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _dev(*ts, rows_strided: bool = False):
    """rows_strided: 2-D views with unit inner stride are accepted (column blocks of wider matrices)."""
    dev = None
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise ValueError("fvqa ops need device tensors (no CPU fallback exists)")
        if rows_strided:
            if t.dim() != 2 or t.stride(1) != 1 or t.stride(0) < t.shape[1]:
                raise ValueError("fvqa GEMM operands must be 2-D with unit inner stride")
        elif not t.is_contiguous():
            raise ValueError("fvqa ops need contiguous tensors")
        dev = dev or t.device
        if t.device != dev:
            raise ValueError("tensors on different devices")


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _need(cond: bool, msg: str):
    if not cond:
        raise ValueError(msg)


def _rider(what: str, rider_a, rider_b, rider_out, accumulate: bool = False):
    """The small product a GEMM launch carries: rider_out (M2 <= 16, N2) = rider_a (M2, K2) @ rider_b (N2, K2)^T, unit inner
    strides -> the SkRider the library takes. The dtype rule is the caller's."""
    M2, K2 = rider_a.shape
    N2 = rider_b.shape[0]
    _need(rider_b.shape[1] == K2 and tuple(rider_out.shape) == (M2, N2) and M2 <= 16 and
          rider_a.stride(1) == rider_b.stride(1) == rider_out.stride(1) == 1, f"{what}: rider shapes")
    return _lib.SkRider(rider_a.data_ptr(), rider_b.data_ptr(), rider_out.data_ptr(), M2, N2, K2, rider_a.stride(0),
                        rider_b.stride(0), rider_out.stride(0), 1 if accumulate else 0)


# ------------------------------------------------------------------------------------ GEMM
_GEMM_WS = {}


def gemm_workspace(device=None, nbytes: int = 0) -> torch.Tensor:
    """THE persistent-GEMM workspace of (device, current stream): epoch flags + partial-tile slabs, shared by every GEMM
    launched on that stream (launches are stream-ordered, and include/fvqa.h allows one workspace per stream at a time:
    a second stream gets a workspace of its own). Its size does not depend on the problem (fvqa_gemm_sk_workspace), so
    the buffer — and the address of its error word — never moves once made."""
    device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    key = (device.index, torch.cuda.current_stream(device).cuda_stream)
    ws = _GEMM_WS.get(key)
    if ws is None:
        need = max(int(nbytes), int(_lib.load().fvqa_gemm_sk_workspace()))
        # zero-filled: the first 4 KiB are the epoch flags of the persistent GEMM (include/fvqa.h), which must
        # start at zero and are never reset afterwards
        ws = torch.zeros(need, dtype=torch.uint8, device=device)
        _GEMM_WS[key] = ws
    if ws.numel() < nbytes:
        raise RuntimeError("fvqa: GEMM workspace request exceeds fvqa_gemm_sk_workspace()")
    return ws


def gemm_error_word(device=None) -> Optional[torch.Tensor]:
    """8-byte view of the error word of the current stream's GEMM workspace (device memory; handed to
    grad_unscale_norm so that a timed-out split-K exchange skips the optimizer step like an overflow); None while no
    persistent GEMM has been launched on this stream."""
    device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    idx = device.index if device.index is not None else torch.cuda.current_device()
    ws = _GEMM_WS.get((idx, torch.cuda.current_stream(device).cuda_stream))
    return None if ws is None else ws[:8]


def gemm_error(ws: Optional[torch.Tensor] = None, device=None) -> int:
    """OR of the error words of the persistent-GEMM workspaces of `device` (include/fvqa.h: non-zero after a launch
    whose split-K exchange timed out), or the word of the given workspace. Device->host reads: not for the step path."""
    if ws is not None:
        return int(ws[:8].view(torch.int64)[0].item())
    idx = None
    if device is not None:
        device = torch.device(device)
        idx = device.index if device.index is not None else torch.cuda.current_device()
    bad = 0
    for (di, _), w in list(_GEMM_WS.items()):
        if idx is None or di == idx:
            bad |= int(w[:8].view(torch.int64)[0].item())
    return bad


class gemm4w_width:
    """`with ops.gemm4w_width(nbt):` — the whole-tile bf16 projections launched by THIS host thread inside the block use tiles of
    16 * nbt columns (nbt in 11, 12, 13, 14, 16) instead of the cost model's pick (include/fvqa.h fvqa_gemm4w_force); tests and
    the width sweep of tools/gemm4w_widths.py. nbt = 0 / None: the cost model."""

    def __init__(self, nbt: Optional[int]):
        self.nbt = int(nbt or 0)

    def __enter__(self):
        _lib.load()
        self.prev = {k: int(lib.fvqa_gemm4w_force(self.nbt)) for k, lib in _lib._LIBS.items()}   # (every loaded library)
        _need(all(v >= 0 for v in self.prev.values()), f"gemm4w_width: no tile width of {self.nbt} x 16 columns")
        return self

    def __exit__(self, *exc):
        for k, v in self.prev.items():
            _lib._LIBS[k].fvqa_gemm4w_force(v)
        return False


def gemm4w_choose(M: int, N: int, K: int, *, out_f32: bool = False, epilogue: int = EPI_NONE, rider_nk=None,
                  n_cu: int = 256) -> int:
    """Tile width (in 16-column blocks) the cost model picks for a bf16 projection on n_cu CUs; 0 = not the whole-tile kernel's
    problem. rider_nk: (N2, K2) of a <= 16-row rider product carried by the launch. Host only (no GPU touched)."""
    rd = None
    if rider_nk is not None:
        rd = _lib.SkRider(1, 1, 1, 10, int(rider_nk[0]), int(rider_nk[1]), int(rider_nk[1]), int(rider_nk[1]), int(rider_nk[0]), 0)
    return int(_lib.load().fvqa_gemm4w_choose(M, N, K, _lib.BF16, _lib.F32 if out_f32 else _lib.BF16, epilogue,
                                              C.addressof(rd) if rd is not None else None, n_cu))


def gemm_nt(a: torch.Tensor, b: torch.Tensor, out: torch.Tensor, *, residual: Optional[torch.Tensor] = None,
            tail: Optional[torch.Tensor] = None, m_split: int = 0, variant: int = 0, nbt: Optional[int] = None) -> torch.Tensor:
    """out[M,N] = a[M,K] @ b[N,K]^T (+ residual). Rows >= m_split go to `tail` (fp32) when given. nbt: force the whole-tile
    kernel's tile width for this call (gemm4w_width)."""
    if nbt:
        with gemm4w_width(nbt):
            return gemm_nt(a, b, out, residual=residual, tail=tail, m_split=m_split, variant=variant)
    _dev(a, b, out, residual, rows_strided=True)
    _dev(tail)
    _need(a.dim() == 2 and b.dim() == 2, "gemm_nt: 2-D operands")
    M, K = a.shape
    N, K2 = b.shape
    _need(K == K2, f"gemm_nt: K mismatch {K} vs {K2}")
    _need(a.dtype == b.dtype, "gemm_nt: a/b dtype mismatch")
    if out is None:                                  # every row accumulates into the fp32 tail
        _need(tail is not None and m_split == 0 and residual is None, "gemm_nt: out=None needs tail and m_split=0")
        _need(tail.dtype == torch.float32 and tuple(tail.shape) == (M, N), "gemm_nt: tail shape")
        out_dtype = a.dtype
    else:
        _need(out.dim() == 2 and out.dtype in (a.dtype, torch.float32), "gemm_nt: out dtype")
        out_dtype = out.dtype
        if tail is None:
            _need(tuple(out.shape) == (M, N), f"gemm_nt: out shape {tuple(out.shape)} != {(M, N)}")
            m_split = M
        else:
            _need(0 <= m_split <= M, "gemm_nt: m_split")
            _need(out.shape[0] >= m_split and out.shape[1] == N, "gemm_nt: out too small")
            _need(tail.dtype == torch.float32 and tuple(tail.shape) == (M - m_split, N), "gemm_nt: tail shape")
    epi = EPI_NONE
    if residual is not None:
        _need(residual.dtype == a.dtype and out_dtype == a.dtype, "gemm_nt: residual dtype")
        _need(residual.shape[1] == N and residual.shape[0] >= min(M, m_split), "gemm_nt: residual shape")
        epi = EPI_RESIDUAL
    lib = _lib.load(a.dtype)
    code = dt_code(a.dtype)
    if variant == 13:
        need = int(lib.fvqa_gemm_sk_workspace())
    elif variant == 0:
        need = int(lib.fvqa_gemm_workspace(M, N, K, code))
    else:
        need = 0
    ws = gemm_workspace(a.device, need) if need else None
    ldc = out.stride(0) if out is not None else N
    _need(residual is None or residual.stride(0) == ldc, "gemm_nt: residual and out must share their row stride")
    rc = lib.fvqa_gemm_nt(_ptr(a), _ptr(b), _ptr(out), _ptr(residual), _ptr(tail), M, N, K, a.stride(0), b.stride(0),
                          ldc, m_split,
                          code, dt_code(out_dtype), epi, variant, _ptr(ws), ws.numel() if ws is not None else 0,
                          _stream())
    _lib.check(rc, "fvqa_gemm_nt")
    return out


def gemm_nt_rider(a, b, out, *, rider_a, rider_b, rider_out, accumulate: bool = False, residual=None, swiglu_ab=None,
                  swiglu_st: bool = False):
    """out = a @ b^T (+ residual | SwiGLU' epilogue with swiglu_ab) and, on the CUs that launch leaves idle (or right
    after it), the small product rider_out (<= 16 rows) = rider_a @ rider_b^T (accumulate: fp32 rider_out += product).
    Operands may be column-block views of wider matrices (rows 16-byte aligned)."""
    for t in (a, b, out, residual, swiglu_ab, rider_a, rider_b, rider_out):
        if t is not None and (not t.is_cuda or t.dim() != 2 or t.stride(1) != 1):
            raise ValueError("gemm_nt_rider: 2-D device tensors with unit inner stride")
    M, K = a.shape
    N = b.shape[0]
    _need(b.shape[1] == K and a.dtype == b.dtype == rider_a.dtype == rider_b.dtype, "gemm_nt_rider: operands")
    epi, R, ldc = EPI_NONE, None, out.stride(0)
    if swiglu_ab is not None:
        _need(tuple(out.shape) == (M, 2 * N) and swiglu_ab.shape == out.shape and out.is_contiguous() and
              swiglu_ab.is_contiguous(), "gemm_nt_rider: SwiGLU' operands")
        epi, R = (EPI_SWIGLU_BWD_ST if swiglu_st else EPI_SWIGLU_BWD), swiglu_ab
    else:
        _need(tuple(out.shape) == (M, N), "gemm_nt_rider: out shape")
        if residual is not None:
            _need(residual.shape == out.shape and residual.stride(0) == ldc, "gemm_nt_rider: residual")
            epi, R = EPI_RESIDUAL, residual
    rd = _rider("gemm_nt_rider", rider_a, rider_b, rider_out, bool(accumulate))
    if accumulate:
        _need(rider_out.dtype == torch.float32 and rider_out.stride(0) == rider_out.shape[1],
              "gemm_nt_rider: an accumulated rider_out is contiguous fp32")
    else:
        _need(rider_out.dtype == a.dtype, "gemm_nt_rider: rider_out dtype")
    lib = _lib.load(a.dtype)
    ws = gemm_workspace(a.device, int(lib.fvqa_gemm_sk_workspace()))
    rc = lib.fvqa_gemm_nt_rider(_ptr(a), _ptr(b), _ptr(out), _ptr(R), M, N, K, a.stride(0), b.stride(0), ldc,
                                dt_code(a.dtype), dt_code(out.dtype), epi, C.addressof(rd), _ptr(ws), ws.numel(),
                                _stream())
    _lib.check(rc, "fvqa_gemm_nt_rider")
    return out


def gemm_timing_enable(on, stride: int = 1) -> None:
    """Measurement probe (include/fvqa.h fvqa_gemm_timing_enable): HIP events around every `stride`-th launch of
    the persistent GEMM kernel on its launch stream, under whichever schedule is running; the other launches are
    counted only (gemm_timing_read returns -2 us for them). Applies to every library loaded so far (the bf16 / fp32 one and,
    once an fp16 model exists, the fp16 one: each keeps its own record)."""
    _lib.load()
    for lib in _lib._LIBS.values():
        _lib.check(lib.fvqa_gemm_timing_enable(int(stride) if on else 0), "fvqa_gemm_timing_enable")


def gemm_timing_read():
    """-> list of (microseconds, flops, kind) per recorded launch (all loaded libraries, one after the other); clears the record."""
    out = []
    for lib in list(_lib._LIBS.values()):
        n = int(lib.fvqa_gemm_timing_read(0, None, None, None))
        if n <= 0:
            continue
        us, fl, kd = (C.c_float * n)(), (C.c_double * n)(), (C.c_int * n)()
        got = int(lib.fvqa_gemm_timing_read(n, C.cast(us, C.c_void_p), C.cast(fl, C.c_void_p), C.cast(kd, C.c_void_p)))
        out += [(float(us[i]), float(fl[i]), int(kd[i])) for i in range(min(n, got))]
    return out


def gemm_nt_swiglu_fwd(x: torch.Tensor, w13: torch.Tensor, ab: torch.Tensor, z: torch.Tensor, st: bool = False, *,
                       rider_a=None, rider_b=None, rider_out=None):
    """ab (M, 2*Hf) = x @ w13^T and z (M, Hf) = silu(a) * b in one launch; w13 / ab in the AB16 layout (pack_ab16).
    st=True (the training step): `ab` receives the backward's factors s = silu(a), t = dz/da in the a and b slots
    (FVQA_EPI_SWIGLU_FWD_ST), to be consumed by gemm_nt_swiglu_bwd(..., st=True). Optional rider (st=True only; <= 16 rows,
    rider_out = rider_a @ rider_b^T in the operands' dtype) as gemm_nt_rider."""
    _dev(x, w13, ab, z)
    _dev(rider_a, rider_b, rider_out, rows_strided=True)
    M, K = x.shape
    N = w13.shape[0]
    _need(w13.shape[1] == K and N % 32 == 0 and x.dtype == w13.dtype == ab.dtype == z.dtype, "gemm_nt_swiglu_fwd: operands")
    _need(ab.shape[-1] == N and ab.numel() >= M * N and z.shape[-1] == N // 2 and z.numel() >= M * N // 2,
          "gemm_nt_swiglu_fwd: ab / z shape")
    lib = _lib.load(x.dtype)
    ws = gemm_workspace(x.device, int(lib.fvqa_gemm_sk_workspace()))
    if rider_a is not None:
        _need(st, "gemm_nt_swiglu_fwd: a rider needs st=True")
        rd = _rider("gemm_nt_swiglu_fwd", rider_a, rider_b, rider_out)
        _need(rider_a.dtype == rider_b.dtype == rider_out.dtype == x.dtype, "gemm_nt_swiglu_fwd: rider dtype")
        rc = lib.fvqa_gemm_nt_swiglu_fwd_st_rider(_ptr(x), _ptr(w13), _ptr(ab), _ptr(z), M, N // 2, K, K, K, dt_code(x.dtype),
                                                  C.byref(rd), _ptr(ws), ws.numel(), _stream())
        _lib.check(rc, "fvqa_gemm_nt_swiglu_fwd_st_rider")
        return z
    fn = lib.fvqa_gemm_nt_swiglu_fwd_st if st else lib.fvqa_gemm_nt_swiglu_fwd
    rc = fn(_ptr(x), _ptr(w13), _ptr(ab), _ptr(z), M, N // 2, K, K, K, dt_code(x.dtype), _ptr(ws), ws.numel(), _stream())
    _lib.check(rc, "fvqa_gemm_nt_swiglu_fwd")
    return z


def pack_ab16(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """(.., H) a and b -> (.., 2H) in the AB16 layout of include/fvqa.h: 16 columns (rows, for weights passed as
    (H, K) matrices: use dim=0) of a, the matching 16 of b, and so on."""
    H = a.shape[-1]
    _need(a.shape == b.shape and H % 16 == 0, "pack_ab16: equal shapes, H % 16 == 0")
    lead = a.shape[:-1]
    return torch.stack([a.reshape(*lead, H // 16, 16), b.reshape(*lead, H // 16, 16)], dim=-2).reshape(*lead, 2 * H)


def unpack_ab16(ab: torch.Tensor):
    """inverse of pack_ab16 -> (a, b)"""
    H2 = ab.shape[-1]
    lead = ab.shape[:-1]
    v = ab.reshape(*lead, H2 // 32, 2, 16)
    return v[..., 0, :].reshape(*lead, H2 // 2), v[..., 1, :].reshape(*lead, H2 // 2)


def gemm_nt_swiglu_bwd(g: torch.Tensor, w2_t: torch.Tensor, ab: torch.Tensor, dab: torch.Tensor, st: bool = False):
    """dab (M, 2*Hf) = d/d(a,b)[silu(a)*b] with dz = g (M,D) @ w2_t (Hf,D)^T formed in the GEMM
    accumulators (the SwiGLU backward is the GEMM's epilogue; dz never reaches HBM). ab / dab: AB16 layout.
    st=True: `ab` holds (s, t) as left by gemm_nt_swiglu_fwd(..., st=True)."""
    _dev(g, w2_t, ab, dab)
    M, K = g.shape
    N = w2_t.shape[0]
    _need(w2_t.shape[1] == K and g.dtype == w2_t.dtype == ab.dtype == dab.dtype, "gemm_nt_swiglu_bwd: operands")
    _need(ab.numel() >= M * 2 * N and dab.numel() >= M * 2 * N and ab.shape[-1] == 2 * N and dab.shape[-1] == 2 * N,
          "gemm_nt_swiglu_bwd: ab/dab shape")
    lib = _lib.load(g.dtype)
    need = int(lib.fvqa_gemm_sk_workspace())                 # this epilogue lives in the persistent kernel
    ws = gemm_workspace(g.device, need)
    rc = lib.fvqa_gemm_nt(_ptr(g), _ptr(w2_t), _ptr(dab), _ptr(ab), None, M, N, K, K, K, 2 * N, M, dt_code(g.dtype),
                          dt_code(g.dtype), EPI_SWIGLU_BWD_ST if st else EPI_SWIGLU_BWD, 0, _ptr(ws),
                          ws.numel() if ws is not None else 0,
                          _stream())
    _lib.check(rc, "fvqa_gemm_nt(swiglu_bwd)")
    return dab


# ------------------------------------------------------------------------------------ row ops
def rmsnorm_fwd(x, w, y, rstd, eps: float, rows: Optional[int] = None):
    _dev(x, w, y, rstd)
    dim = x.shape[-1]
    rows = rows if rows is not None else x.numel() // dim
    _need(x.dtype == w.dtype == y.dtype, "rmsnorm_fwd: dtype")
    _need(w.numel() == dim and y.shape[-1] == dim, "rmsnorm_fwd: dim")
    _need(x.numel() >= rows * dim and y.numel() >= rows * dim, "rmsnorm_fwd: rows")
    _need(rstd is None or (rstd.dtype == torch.float32 and rstd.numel() >= rows), "rmsnorm_fwd: rstd")
    rc = _lib.load(x.dtype).fvqa_rmsnorm_fwd(_ptr(x), _ptr(w), _ptr(y), _ptr(rstd), rows, dim, float(eps),
                                      dt_code(x.dtype), _stream())
    _lib.check(rc, "fvqa_rmsnorm_fwd")
    return y


def rmsnorm_bwd(g, x, w, rstd, dx, resid=None, rows: Optional[int] = None):
    _dev(g, x, w, rstd, dx, resid)
    dim = x.shape[-1]
    rows = rows if rows is not None else x.numel() // dim
    _need(g.dtype == x.dtype == w.dtype == dx.dtype, "rmsnorm_bwd: dtype")
    _need(resid is None or resid.dtype == x.dtype, "rmsnorm_bwd: resid dtype")
    for t in (g, x, dx, resid):
        _need(t is None or (t.shape[-1] == dim and t.numel() >= rows * dim), "rmsnorm_bwd: shape")
    _need(rstd.dtype == torch.float32 and rstd.numel() >= rows and w.numel() == dim, "rmsnorm_bwd: rstd/w")
    rc = _lib.load(g.dtype).fvqa_rmsnorm_bwd(_ptr(g), _ptr(x), _ptr(w), _ptr(rstd), _ptr(resid), _ptr(dx), rows, dim,
                                      dt_code(x.dtype), _stream())
    _lib.check(rc, "fvqa_rmsnorm_bwd")
    return dx


def rmsnorm_dw_workspace(rows: int, dim: int, dtype=None) -> int:
    """Bytes of workspace fvqa_rmsnorm_dw needs for (rows, dim); 0: a shape it refuses."""
    return int(_lib.load(dtype).fvqa_rmsnorm_dw_workspace(int(rows), int(dim)))


def rmsnorm_dw(g, x, rstd, dw, ws, accumulate: bool = True, rows: Optional[int] = None):
    """dw (dim,) fp32 (+)= sum_r g[r] * round_to_storage(x[r] * rstd[r]): the gradient of an RMSNorm's weight (include/fvqa.h).
    ws: a uint8 device buffer of at least rmsnorm_dw_workspace(rows, dim) bytes."""
    _dev(g, x, rstd, dw, ws)
    dim = x.shape[-1]
    rows = rows if rows is not None else x.numel() // dim
    _need(g.dtype == x.dtype, "rmsnorm_dw: dtype")
    for t in (g, x):
        _need(t.shape[-1] == dim and t.numel() >= rows * dim, "rmsnorm_dw: shape")
    _need(rstd.dtype == torch.float32 and rstd.numel() >= rows, "rmsnorm_dw: rstd")
    _need(dw.dtype == torch.float32 and dw.numel() == dim, "rmsnorm_dw: dw")
    lib = _lib.load(g.dtype)
    need = int(lib.fvqa_rmsnorm_dw_workspace(rows, dim))
    _need(ws.dtype == torch.uint8 and (need == 0 or ws.numel() >= need), "rmsnorm_dw: workspace")
    rc = lib.fvqa_rmsnorm_dw(_ptr(g), _ptr(x), _ptr(rstd), _ptr(dw), _ptr(ws), ws.numel(), rows, dim, int(bool(accumulate)),
                             dt_code(x.dtype), _stream())
    _lib.check(rc, "fvqa_rmsnorm_dw")
    return dw


def rope_qk(qkv, cos_t, sin_t, n_seq: int, seq_len: int, n_heads: int, head_dim: int, inverse: bool = False):
    _dev(qkv, cos_t, sin_t)
    dim = n_heads * head_dim
    _need(qkv.shape[-1] == 3 * dim and qkv.numel() >= n_seq * seq_len * 3 * dim, "rope_qk: qkv shape")
    _need(cos_t.dtype == sin_t.dtype == torch.float32, "rope_qk: table dtype")
    _need(cos_t.shape[-1] == head_dim // 2 and cos_t.shape[0] >= seq_len and sin_t.shape == cos_t.shape,
          "rope_qk: table shape")
    rc = _lib.load(qkv.dtype).fvqa_rope_qk(_ptr(qkv), _ptr(cos_t), _ptr(sin_t), n_seq, seq_len, n_heads, head_dim,
                                  int(inverse), dt_code(qkv.dtype), _stream())
    _lib.check(rc, "fvqa_rope_qk")
    return qkv


def swiglu_fwd(ab, z, rows: int, hidden: int):
    _dev(ab, z)
    _need(ab.dtype == z.dtype, "swiglu_fwd: dtype")
    _need(ab.numel() >= rows * 2 * hidden and z.numel() >= rows * hidden, "swiglu_fwd: shape")
    rc = _lib.load(ab.dtype).fvqa_swiglu_fwd(_ptr(ab), _ptr(z), rows, hidden, dt_code(ab.dtype), _stream())
    _lib.check(rc, "fvqa_swiglu_fwd")
    return z


def swiglu_bwd(dz, ab, dab, rows: int, hidden: int):
    _dev(dz, ab, dab)
    _need(dz.dtype == ab.dtype == dab.dtype, "swiglu_bwd: dtype")
    _need(ab.numel() >= rows * 2 * hidden and dab.numel() >= rows * 2 * hidden and dz.numel() >= rows * hidden,
          "swiglu_bwd: shape")
    rc = _lib.load(ab.dtype).fvqa_swiglu_bwd(_ptr(dz), _ptr(ab), _ptr(dab), rows, hidden, dt_code(ab.dtype), _stream())
    _lib.check(rc, "fvqa_swiglu_bwd")
    return dab


def row_segs(maps, offs, stream_rows: int):
    """fvqa_row_segs (include/fvqa.h) of up to three streams: maps[k] the int32 device map of stream k (gather: compact -> dense row
    within the stream; scatter: dense row -> compact row within the segment, -1 none), offs the segment offsets (len(maps) + 1)."""
    n = len(maps)
    _need(1 <= n <= 3 and len(offs) == n + 1 and offs[0] == 0, "row_segs: 1..3 segments starting at 0")
    sg = _lib.RowSegs()
    sg.n, sg.stream_rows = n, int(stream_rows)
    for k in range(4):
        sg.off[k] = int(offs[min(k, n)])
    for k, m in enumerate(maps):
        _dev(m)
        _need(m.dtype == torch.int32 and m.dim() == 1 and m.is_contiguous(), "row_segs: int32 maps")
        sg.map[k] = m.data_ptr()
    sg._keep = list(maps)
    return sg


def gather_rows(src, dst, segs):
    """dst (M, dim) compact <- rows of src ((n * stream_rows), dim) dense, by segs (row_segs of idx maps)."""
    _dev(src, dst)
    _need(src.dim() == 2 and dst.dim() == 2 and src.dtype == dst.dtype and src.shape[1] == dst.shape[1], "gather_rows: shape")
    _need(src.shape[0] >= segs.n * segs.stream_rows and dst.shape[0] >= segs.off[segs.n], "gather_rows: rows")
    rc = _lib.load(src.dtype).fvqa_gather_rows(_ptr(src), _ptr(dst), C.addressof(segs), src.shape[1], dt_code(src.dtype), _stream())
    _lib.check(rc, "fvqa_gather_rows")
    return dst


def scatter_rows(src, dst, segs):
    """dst ((n * stream_rows), dim) dense <- rows of src (M, dim) compact by segs (row_segs of inv maps), zeros where the map is < 0."""
    _dev(src, dst)
    _need(src.dim() == 2 and dst.dim() == 2 and src.dtype == dst.dtype and src.shape[1] == dst.shape[1], "scatter_rows: shape")
    _need(dst.shape[0] >= segs.n * segs.stream_rows and src.shape[0] >= segs.off[segs.n], "scatter_rows: rows")
    rc = _lib.load(src.dtype).fvqa_scatter_rows(_ptr(src), _ptr(dst), C.addressof(segs), src.shape[1], dt_code(src.dtype), _stream())
    _lib.check(rc, "fvqa_scatter_rows")
    return dst


def cast_rows(src, dst_rows):
    """dst_rows (n, dim) storage dtype <- src (n, dim) fp32."""
    _dev(src, dst_rows)
    _need(src.dtype == torch.float32 and src.shape == dst_rows.shape and src.dim() == 2, "cast_rows: shape")
    rc = _lib.load(dst_rows.dtype).fvqa_cast_rows(_ptr(src), _ptr(dst_rows), src.shape[0], src.shape[1],
                                    dt_code(dst_rows.dtype), _stream())
    _lib.check(rc, "fvqa_cast_rows")
    return dst_rows


# ------------------------------------------------------------------------------------ attention
def _attn_shapes(qkv, n_seq, S, H, Dh, A):
    D = H * Dh
    _need(qkv.dim() == 2 and tuple(qkv.shape) == (n_seq * S + A, 3 * D),
          f"attention: qkv must be ({n_seq * S + A}, {3 * D}), got {tuple(qkv.shape)}")
    _need(Dh == 128 and 1 <= A <= 16, "attention: head_dim must be 128 and adapter_len <= 16")
    return D


def kv_rider_ahead(dtype: torch.dtype) -> bool:
    """True when the step computes the adapter K/V rows of layer i+1 as the rider of layer i's W1|W3 launch (layer 0's as a
    launch of its own before the walk) instead of beside layer i+1's QKV projection (csrc/schedule.hip)."""
    return bool(_lib.load(dtype).fvqa_kv_rider_ahead(dt_code(dtype)))


def swiglu_st() -> bool:
    """True unless FVQA_SWIGLU_AB=1: the W1|W3 launch saves the SwiGLU backward's factors (s, t) instead of (a, b)."""
    return bool(_lib.load().fvqa_swiglu_st())


def rope_in_gemm(dtype: torch.dtype) -> bool:
    """True when the step rotates q, k in the QKV projection's epilogue (gemm_nt_rope): the arena's qkv rows hold ROTATED
    q, k, attn_fwd runs without tables and the backward is attn_bwd(..., prerotated=True)."""
    return bool(_lib.load(dtype).fvqa_rope_in_gemm(dt_code(dtype)))


def gemm_nt_rope(a, b, out, rope, seq_len, head_dim, n_heads, *, rider_a=None, rider_b=None, rider_out=None):
    """out (M, 3*D) = a @ b.T with RoPE applied to the q | k columns [0, 2*D) in the epilogue (bf16; position = row % seq_len);
    optional rider (<= 16 rows) as gemm_nt_rider."""
    _dev(a, b, out, rider_a, rider_b, rider_out, rows_strided=True)
    _need(a.dtype == b.dtype == out.dtype and a.dtype in (torch.bfloat16, torch.float16), "gemm_nt_rope: 16-bit storage")
    for t in (a, b, out):
        _need(t.dim() == 2 and t.stride(1) == 1, "gemm_nt_rope: 2-D tensors with unit inner stride")
    M, K = a.shape
    N = b.shape[0]
    D = n_heads * head_dim
    _need(b.shape[1] == K and tuple(out.shape) == (M, N) and N >= 2 * D and M % seq_len == 0, "gemm_nt_rope: shapes")
    cos_t, sin_t = _rope_tables(rope, seq_len, head_dim, "gemm_nt_rope")
    _need(cos_t is not None, "gemm_nt_rope: rope tables")
    rp = _lib.SkRope(cos_t.data_ptr(), sin_t.data_ptr(), seq_len, head_dim, 2 * D)
    rd = None
    if rider_a is not None:
        rd = _rider("gemm_nt_rope", rider_a, rider_b, rider_out)
        _need(rider_out.dtype == a.dtype, "gemm_nt_rope: rider dtype")
    ws = gemm_workspace(a.device)
    rc = _lib.load(a.dtype).fvqa_gemm_nt_rope(_ptr(a), _ptr(b), _ptr(out), M, N, K, a.stride(0), b.stride(0), out.stride(0),
                                       C.byref(rp), C.byref(rd) if rd is not None else None, _ptr(ws), ws.numel(),
                                       _stream())
    _lib.check(rc, "fvqa_gemm_nt_rope")
    return out


def attn_rope_fused(dtype: torch.dtype) -> bool:
    """True when attn_fwd / attn_bwd of this dtype rotate q,k themselves (rope=(cos, sin) argument)."""
    return bool(_lib.load(dtype).fvqa_attn_rope_fused(dt_code(dtype)))


def _rope_tables(rope, S, Dh, what):
    if rope is None:
        return None, None
    cos_t, sin_t = rope
    _dev(cos_t, sin_t)
    _need(cos_t.dtype == sin_t.dtype == torch.float32 and cos_t.shape == sin_t.shape and
          cos_t.shape[-1] == Dh // 2 and cos_t.shape[0] >= S and cos_t.is_contiguous() and sin_t.is_contiguous(),
          f"{what}: rope tables")
    return cos_t, sin_t


def attn_fwd(qkv, o, lse_a, lse_t, gate1, gate2, vstart, n_seq, S, H, Dh, A, F, rope=None):
    """rope=(cos_t, sin_t): qkv holds the raw projections and RoPE is applied inside (attn_rope_fused)."""
    _dev(qkv, o, lse_a, lse_t, gate1, gate2, vstart)
    cos_t, sin_t = _rope_tables(rope, S, Dh, "attn_fwd")
    D = _attn_shapes(qkv, n_seq, S, H, Dh, A)
    _need(o.dtype == qkv.dtype and tuple(o.shape) == (n_seq * S, D), "attn_fwd: o shape")
    for t in (lse_a, lse_t):
        _need(t.dtype == torch.float32 and t.numel() == n_seq * H * S, "attn_fwd: lse shape")
    for t in (gate1, gate2):
        _need(t.dtype == torch.float32 and t.numel() == H, "attn_fwd: gate shape")
    _need(vstart.dtype == torch.int32 and vstart.numel() == n_seq, "attn_fwd: vstart")
    rc = _lib.load(qkv.dtype).fvqa_attn_fwd(_ptr(qkv), _ptr(o), _ptr(lse_a), _ptr(lse_t), _ptr(gate1), _ptr(gate2),
                                   _ptr(vstart), _ptr(cos_t), _ptr(sin_t), n_seq, S, H, Dh, A, F,
                                   dt_code(qkv.dtype), _stream())
    _lib.check(rc, "fvqa_attn_fwd")
    return o


def _attn_decode(what, qkv_row, qkv_cache, o_row, gate1, gate2, vstart, pos, rope, n_seq, S, H, Dh, A, F, cache_rotated, mass=None):
    """attn_decode and attn_decode_mass (mass given): the same operands and checks but for the summary."""
    _dev(qkv_row, qkv_cache, o_row, gate1, gate2, vstart, pos, mass)
    cos_t, sin_t = _rope_tables(rope, S, Dh, what)
    D = _attn_shapes(qkv_cache, n_seq, S, H, Dh, A)
    _need(cos_t is not None, f"{what}: rope tables")
    _need(qkv_row.dtype == qkv_cache.dtype == o_row.dtype, f"{what}: dtype")
    _need(tuple(qkv_row.shape) == (n_seq, 3 * D) and tuple(o_row.shape) == (n_seq, D), f"{what}: row shapes")
    _need(pos.dtype == torch.int64 and pos.numel() == n_seq, f"{what}: pos")
    _need(vstart.dtype == torch.int32 and vstart.numel() == n_seq, f"{what}: vstart")
    for t in (gate1, gate2):
        _need(t.dtype == torch.float32 and t.numel() == H, f"{what}: gate shape")
    extra = ()
    if mass is not None:
        _need(F >= 0 and mass.dtype == torch.float32 and tuple(mass.shape) == (n_seq, H, F + 2),
              f"{what}: mass must be fp32 (n_seq, H, F + 2)")
        extra = (_ptr(mass),)
    rc = getattr(_lib.load(qkv_cache.dtype), "fvqa_" + what)(
        _ptr(qkv_row), _ptr(qkv_cache), _ptr(o_row), _ptr(gate1), _ptr(gate2), _ptr(vstart), _ptr(pos), _ptr(cos_t),
        _ptr(sin_t), *extra, n_seq, S, H, Dh, A, F, 1 if cache_rotated else 0, dt_code(qkv_row.dtype), _stream())
    _lib.check(rc, "fvqa_" + what)
    return o_row


def attn_decode(qkv_row, qkv_cache, o_row, gate1, gate2, vstart, pos, rope, n_seq, S, H, Dh, A, F, cache_rotated: bool):
    """One new token per sequence (generation path): attention of the new row over the cached keys / values + the
    adapter prefix; the new token's k, v are stored into cache row n*S + pos[n]. qkv_row holds RAW projections."""
    return _attn_decode("attn_decode", qkv_row, qkv_cache, o_row, gate1, gate2, vstart, pos, rope, n_seq, S, H, Dh, A, F,
                        cache_rotated)


def attn_decode_mass(qkv_row, qkv_cache, o_row, mass, gate1, gate2, vstart, pos, rope, n_seq, S, H, Dh, A, F,
                     cache_rotated: bool):
    """attn_decode — the same o_row and cache stores, bit for bit — that also writes each row's frame-attention summary into
    mass (n_seq, H, F + 2) fp32: the text softmax's weight on each frame key, in front of the window and behind it
    (include/fvqa.h fvqa_attn_decode_mass)."""
    return _attn_decode("attn_decode_mass", qkv_row, qkv_cache, o_row, gate1, gate2, vstart, pos, rope, n_seq, S, H, Dh, A, F,
                        cache_rotated, mass=mass)


def attn_row_mass(qkv, seq, pos, mass, gate2, vstart, rope, n_seq, S, H, Dh, A, F, cache_rotated: bool):
    """The summary of attn_decode_mass for R rows that already sit in a layer's arena buffer qkv (n_seq*S + A, 3*D), q and k in
    the cache's convention: row r is the query at position pos[r] of sequence seq[r] (int32, R each). Writes mass (R, H, F + 2)
    fp32 and nothing else (include/fvqa.h fvqa_attn_row_mass)."""
    _dev(qkv, seq, pos, mass, gate2, vstart)
    cos_t, sin_t = _rope_tables(rope, S, Dh, "attn_row_mass")
    _attn_shapes(qkv, n_seq, S, H, Dh, A)
    _need(cos_t is not None, "attn_row_mass: rope tables")
    R = seq.numel()
    _need(seq.dtype == pos.dtype == torch.int32 and 1 <= R <= 65535 and pos.numel() == R,
          "attn_row_mass: seq and pos are int32, 1..65535 rows each")
    _need(vstart.dtype == torch.int32 and vstart.numel() == n_seq, "attn_row_mass: vstart")
    _need(gate2.dtype == torch.float32 and gate2.numel() == H, "attn_row_mass: gate shape")
    _need(F >= 0 and mass.dtype == torch.float32 and tuple(mass.shape) == (R, H, F + 2),
          "attn_row_mass: mass must be fp32 (R, H, F + 2)")
    rc = _lib.load(qkv.dtype).fvqa_attn_row_mass(_ptr(qkv), _ptr(seq), _ptr(pos), _ptr(gate2), _ptr(vstart), _ptr(cos_t),
                                                 _ptr(sin_t), _ptr(mass), R, n_seq, S, H, Dh, A, F, 1 if cache_rotated else 0,
                                                 dt_code(qkv.dtype), _stream())
    _lib.check(rc, "fvqa_attn_row_mass")
    return mass


SUFFIX_MAX = 16          # suffix rows per option fvqa_attn_suffix takes (csrc/score.hip TMAX)
SUFFIX_MASS_FEATS = 64   # max_feats fvqa_attn_suffix_mass takes (csrc/score.hip MFMAX: the accumulators' LDS rows)
SUFFIX_WIDE_MAX = 64     # suffix rows per option fvqa_attn_suffix_wide takes (csrc/score.hip TWIDE)


def _attn_suffix(what, qkv_suf, qkv_cache, o_suf, gate1, gate2, vstart, start, length, rope, n_seq, n_options, T, S, H, Dh, A, F,
                 cache_rotated, mass=None, t_max=SUFFIX_MAX):
    """attn_suffix (n_options >= 1 continuations per sequence, the cache only read), attn_suffix_mass (the same with the summary:
    mass given), attn_suffix_wide (up to t_max = SUFFIX_WIDE_MAX rows) and attn_suffix_append (n_options None: one, whose rows
    join the cache): the same operands but for the options and the summary."""
    _dev(qkv_suf, qkv_cache, o_suf, gate1, gate2, vstart, start, length, mass)
    cos_t, sin_t = _rope_tables(rope, S, Dh, what)
    D = _attn_shapes(qkv_cache, n_seq, S, H, Dh, A)
    R = n_seq * (n_options or 1) * T
    _need(cos_t is not None, f"{what}: rope tables")
    _need(qkv_suf.dtype == qkv_cache.dtype == o_suf.dtype, f"{what}: dtype")
    _need(1 <= T <= t_max and (n_options is None or n_options >= 1), f"{what}: 1 <= {'rows per sequence' if n_options is None else 'suffix rows'} <= {t_max}")
    _need(tuple(qkv_suf.shape) == (R, 3 * D) and tuple(o_suf.shape) == (R, D), f"{what}: row shapes")
    for t in (vstart, start, length):
        _need(t.dtype == torch.int32 and t.numel() == n_seq, f"{what}: vstart / start / len are int32 (n_seq)")
    for t in (gate1, gate2):
        _need(t.dtype == torch.float32 and t.numel() == H, f"{what}: gate shape")
    extra = ()
    if mass is not None:
        _need(0 <= F <= SUFFIX_MASS_FEATS and mass.dtype == torch.float32 and mass.is_contiguous()
              and tuple(mass.shape) == (R, H, F + 2), f"{what}: mass must be fp32 (rows, H, F + 2), F <= {SUFFIX_MASS_FEATS}")
        extra = (_ptr(mass),)
    rc = getattr(_lib.load(qkv_cache.dtype), "fvqa_" + what)(
        _ptr(qkv_suf), _ptr(qkv_cache), _ptr(o_suf), _ptr(gate1), _ptr(gate2), _ptr(vstart), _ptr(start), _ptr(length),
        _ptr(cos_t), _ptr(sin_t), n_seq, *(() if n_options is None else (n_options,)), T, S, H, Dh, A, F,
        1 if cache_rotated else 0, dt_code(qkv_suf.dtype), _stream(), *extra)
    _lib.check(rc, "fvqa_" + what)
    return o_suf


def attn_suffix(qkv_suf, qkv_cache, o_suf, gate1, gate2, vstart, start, length, rope, n_seq, n_options, T, S, H, Dh, A, F,
                cache_rotated: bool):
    """The option-scoring path's attention at the suffix rows (include/fvqa.h fvqa_attn_suffix): qkv_suf (n_seq*n_options*T,
    3*D) RAW projections of suffix row j of option c of sample n at position start[n] + j; qkv_cache the layer's prefill buffer
    (read only). Writes o_suf (n_seq*n_options*T, D); rows j >= length[n] are padding (zeros)."""
    return _attn_suffix("attn_suffix", qkv_suf, qkv_cache, o_suf, gate1, gate2, vstart, start, length, rope, n_seq,
                        int(n_options), T, S, H, Dh, A, F, cache_rotated)


def attn_suffix_mass(qkv_suf, qkv_cache, o_suf, mass, gate1, gate2, vstart, start, length, rope, n_seq, n_options, T, S, H, Dh, A,
                     F, cache_rotated: bool):
    """attn_suffix — the same o_suf, bit for bit — that also writes each suffix row's frame-attention summary into mass
    (n_seq*n_options*T, H, F + 2) fp32: the text softmax's weight on each frame key, in front of the window and behind it; zeros
    at the rows j >= length[n] (include/fvqa.h fvqa_attn_suffix_mass). F <= SUFFIX_MASS_FEATS."""
    _need(mass is not None, "attn_suffix_mass: mass is required")
    return _attn_suffix("attn_suffix_mass", qkv_suf, qkv_cache, o_suf, gate1, gate2, vstart, start, length, rope, n_seq,
                        int(n_options), T, S, H, Dh, A, F, cache_rotated, mass=mass)


def attn_suffix_append(qkv_suf, qkv_cache, o_suf, gate1, gate2, vstart, start, length, rope, n_seq, T, S, H, Dh, A, F,
                       cache_rotated: bool):
    """attn_suffix for ONE continuation per sequence whose rows join the cache (include/fvqa.h fvqa_attn_suffix_append; the
    draft-and-verify pass of generate(lookahead=T)): qkv_suf (n_seq*T, 3*D) RAW projections of row j of sequence n at position
    start[n] + j. Writes o_suf (n_seq*T, D) as attn_suffix does, and the k (in the cache's convention) and v of the rows
    j < length[n] into cache row n*S + start[n] + j — the bits attn_decode stores for the same raw row and position."""
    return _attn_suffix("attn_suffix_append", qkv_suf, qkv_cache, o_suf, gate1, gate2, vstart, start, length, rope, n_seq, None,
                        T, S, H, Dh, A, F, cache_rotated)


def attn_suffix_wide(qkv_suf, qkv_cache, o_suf, gate1, gate2, vstart, start, length, rope, n_seq, n_options, T, S, H, Dh, A, F,
                     cache_rotated: bool):
    """attn_suffix for 1 <= T <= SUFFIX_WIDE_MAX suffix rows per option (include/fvqa.h fvqa_attn_suffix_wide): the same operands
    and semantics; the frame window [vstart, vstart + F) may lie inside the suffix (vstart < 0: none)."""
    return _attn_suffix("attn_suffix_wide", qkv_suf, qkv_cache, o_suf, gate1, gate2, vstart, start, length, rope, n_seq,
                        int(n_options), T, S, H, Dh, A, F, cache_rotated, t_max=SUFFIX_WIDE_MAX)


def option_pick(rowloss, row_map, n_rows: int, n_seq: int, n_options: int, S: int):
    """The per-option reduction (include/fvqa.h fvqa_option_pick): rowloss fp32 compact per-row losses, row_map int32 (entry of
    (n_seq, n_options, S-1) each of the first n_rows rows belongs to, < 0 none) ->
    (individual_losses (n_seq, n_options, S-1) fp32, sum, count int64, mean (n_seq, n_options), prediction (n_seq,) int64)."""
    _dev(rowloss, row_map)
    _need(rowloss.dtype == torch.float32 and row_map.dtype == torch.int32, "option_pick: fp32 losses, int32 map")
    _need(0 <= n_rows <= min(rowloss.numel(), row_map.numel()), "option_pick: rows")
    _need(1 <= n_options <= 64 and S >= 2 and n_seq >= 1, "option_pick: 1..64 options")
    dev = rowloss.device
    il = torch.empty(n_seq, n_options, S - 1, dtype=torch.float32, device=dev)
    s = torch.empty(n_seq, n_options, dtype=torch.float32, device=dev)
    cnt = torch.empty(n_seq, n_options, dtype=torch.int64, device=dev)
    mean = torch.empty(n_seq, n_options, dtype=torch.float32, device=dev)
    pred = torch.empty(n_seq, dtype=torch.int64, device=dev)
    rc = _lib.load().fvqa_option_pick(_ptr(rowloss), _ptr(row_map), n_rows, _ptr(il), _ptr(s), _ptr(cnt), _ptr(mean),
                                      _ptr(pred), n_seq, n_options, S, _stream())
    _lib.check(rc, "fvqa_option_pick")
    return il, s, cnt, mean, pred


_I32, _I64, _F32 = torch.int32, torch.int64, torch.float32
_DTYPE_NAME = {_I32: "int32", _I64: "int64", _F32: "fp32"}


def _lead(t) -> int:
    """Rows of a 2-D operand; -1, which no check accepts, of anything else."""
    return t.shape[0] if t.dim() == 2 else -1


def _of(dtype, numel, **tensors):
    """Rows of _token_step's table: the named operands are `dtype` tensors of `numel` elements."""
    return [(name, t, dtype, numel) for name, t in tensors.items()]


def _table(what, table):
    """The check of _of's rows: each named operand has its dtype and element count."""
    for name, t, dtype, numel in table:
        _need(t.dtype == dtype and t.numel() == numel, f"{what}: {name} is {_DTYPE_NAME.get(dtype, dtype)}, {numel} elements")


def suffix_embed(ids, slot, emb, vf_tok, length, x, n_seq: int, n_options: int, T: int, F: int):
    """The suffix rows' inputs (include/fvqa.h fvqa_suffix_embed): x (n_seq*n_options*T, D) <- emb[ids[r]], or the bits of
    vf_tok[n, slot[r]] where slot[r] >= 0 (slot int32 (rows) or None; vf_tok (n_seq, F, D) of x's dtype), or zeros at the rows
    j >= length[n]. ids (rows) int64 inside the table: checked on the host copy by the caller."""
    _dev(ids, slot, emb, vf_tok, length, x)
    R = n_seq * n_options * T
    _need(n_seq >= 1 and n_options >= 1 and T >= 1 and R <= 0x7fffffff, "suffix_embed: rows")
    _need(emb.dim() == 2 and x.dtype == emb.dtype and tuple(x.shape) == (R, emb.shape[1]), "suffix_embed: x (rows, D) of emb's dtype")
    D = emb.shape[1]
    _need(D * emb.element_size() % 16 == 0, "suffix_embed: rows of a multiple of 16 bytes")
    _table("suffix_embed", _of(_I64, R, ids=ids) + _of(_I32, n_seq, length=length) +
           (_of(_I32, R, slot=slot) + _of(emb.dtype, n_seq * F * D, vf_tok=vf_tok) if slot is not None else []))
    _need(slot is None or F >= 1, "suffix_embed: frame rows need max_feats >= 1")
    rc = _lib.load(emb.dtype).fvqa_suffix_embed(_ptr(ids), _ptr(slot), _ptr(emb), _ptr(vf_tok if slot is not None else None),
                                                _ptr(length), _ptr(x), n_seq, n_options, T, D, emb.shape[0], F,
                                                dt_code(emb.dtype), _stream())
    _lib.check(rc, "fvqa_suffix_embed")
    return x


TREE_DEPTH_MAX = 31          # depth of a row fvqa_attn_suffix_tree takes (include/fvqa.h FVQA_TREE_DEPTH_MAX)
TREE_ROWS_MAX = 4096         # rows (and members) per sample (FVQA_TREE_ROWS_MAX)
TREE_TOTAL_ROWS_MAX = 65536  # n_seq * rows of one pass (FVQA_TREE_TOTAL_ROWS_MAX)
TREE_TILE = 32               # rows per tile (csrc/score.hip QT)
TREE_TOP_MAX = 8             # members fvqa_trie_score ranks (csrc/tree.hip TOPMAX)


def attn_suffix_tree(qkv_suf, qkv_cache, o_suf, gate1, gate2, vstart, start, n_rows, depth, end, tile_anc, rope, n_seq, R, S, H,
                     Dh, A, F, cache_rotated: bool):
    """The tree-masked suffix attention (include/fvqa.h fvqa_attn_suffix_tree): qkv_suf (n_seq*R, 3*D) RAW projections of row r of
    sample n at position start[n] + depth[n, r]; a row sees the cache rows [0, start[n]), its ancestors-or-self among the rows and
    the adapter keys. n_rows (n_seq), depth / end (n_seq*R), tile_anc (n_seq * ceil(R / 32) * 32): int32, fvqa.vocab.plan_vocab's.
    Writes o_suf (n_seq*R, D); rows r >= n_rows[n] are padding (zeros). The shapes, dtypes and alignment are checked here; the
    VALUES of the plan's arrays are the planner's (the kernel clamps what it reads)."""
    what = "attn_suffix_tree"
    _need(all(torch.is_tensor(t) for t in (qkv_suf, qkv_cache, o_suf, gate1, gate2, vstart, start, n_rows, depth, end, tile_anc)),
          f"{what}: tensors")
    _need(int(n_seq) >= 1 and 1 <= int(R) <= TREE_ROWS_MAX and n_seq * R <= TREE_TOTAL_ROWS_MAX,
          f"{what}: 1 <= rows per sample <= {TREE_ROWS_MAX}, n_seq * rows <= {TREE_TOTAL_ROWS_MAX}")
    _need(qkv_cache.dim() == 2 and qkv_suf.dim() == 2 and o_suf.dim() == 2, f"{what}: 2-D rows")
    D = H * Dh
    _need(Dh == 128 and 0 <= A <= 16 and F >= 0 and 1 <= S <= 4096, f"{what}: head_dim 128, adapter_len <= 16, seq_len <= 4096")
    _need(qkv_suf.dtype == qkv_cache.dtype == o_suf.dtype, f"{what}: dtype")
    _need(tuple(qkv_cache.shape) == (n_seq * S + A, 3 * D), f"{what}: qkv_cache is (n_seq * S + A, 3 * D)")
    _need(tuple(qkv_suf.shape) == (n_seq * R, 3 * D) and tuple(o_suf.shape) == (n_seq * R, D), f"{what}: row shapes")
    tiles = (R + TREE_TILE - 1) // TREE_TILE
    _table(what, _of(_I32, n_seq, vstart=vstart, start=start, n_rows=n_rows) + _of(_I32, n_seq * R, depth=depth, end=end) +
           _of(_I32, n_seq * tiles * TREE_TILE, tile_anc=tile_anc) + _of(_F32, H, gate1=gate1, gate2=gate2))
    for name, t in (("qkv_suf", qkv_suf), ("qkv_cache", qkv_cache), ("o_suf", o_suf)):
        _need(t.data_ptr() % 16 == 0, f"{what}: {name} on a 16-byte boundary")
    _dev(qkv_suf, qkv_cache, o_suf, gate1, gate2, vstart, start, n_rows, depth, end, tile_anc)
    cos_t, sin_t = _rope_tables(rope, S, Dh, what)
    _need(cos_t is not None, f"{what}: rope tables")
    rc = _lib.load(qkv_cache.dtype).fvqa_attn_suffix_tree(
        _ptr(qkv_suf), _ptr(qkv_cache), _ptr(o_suf), _ptr(gate1), _ptr(gate2), _ptr(vstart), _ptr(start), _ptr(n_rows),
        _ptr(depth), _ptr(end), _ptr(tile_anc), _ptr(cos_t), _ptr(sin_t), n_seq, R, S, H, Dh, A, F, 1 if cache_rotated else 0,
        dt_code(qkv_suf.dtype), _stream())
    _lib.check(rc, "fvqa_attn_suffix_tree")
    return o_suf


def trie_score(tables: dict, edge_lp, n_seq: int, R: int, V: int, *, logits=None, lse=None, row0: int = 0, n_block_rows: int = 0,
               reduce: bool = False, n_columns: int = 0, top: int = 1, by_mean: bool = True):
    """The reduction of the tree pass (include/fvqa.h fvqa_trie_score). tables: the int32 device arrays of a plan — edge_parent,
    edge_token (n_seq, E), n_edges (n_seq,), member_path (n_seq, MU, 32), member_len, member_index (n_seq, MU), n_members
    (n_seq,); edge_lp (n_seq, E) fp32, in and out. logits (>= n_block_rows, V) fp32 with lse: the block of head rows [row0, row0 +
    n_block_rows) fills its edges. reduce: -> dict(logprob_sum, count (int64), mean, log_posterior (n_seq, n_columns), ranking
    (n_seq, top) int64, prediction (n_seq,) int64); None otherwise."""
    what = "trie_score"
    ep, et, ne = tables["edge_parent"], tables["edge_token"], tables["n_edges"]
    mp, ml, mi, nm = tables["member_path"], tables["member_len"], tables["member_index"], tables["n_members"]
    _need(ep.dim() == 2 and ep.shape[0] == n_seq and ep.shape[1] >= 1, f"{what}: edge_parent is (n_seq, E)")
    E = int(ep.shape[1])
    _need(mp.dim() == 3 and mp.shape[0] == n_seq and mp.shape[2] == TREE_DEPTH_MAX + 1 and 1 <= mp.shape[1] <= TREE_ROWS_MAX,
          f"{what}: member_path is (n_seq, members <= {TREE_ROWS_MAX}, {TREE_DEPTH_MAX + 1})")
    MU = int(mp.shape[1])
    _table(what, _of(_I32, n_seq * E, edge_parent=ep, edge_token=et) + _of(_I32, n_seq, n_edges=ne, n_members=nm) +
           _of(_I32, n_seq * MU, member_len=ml, member_index=mi) + _of(_F32, n_seq * E, edge_lp=edge_lp))
    _need(1 <= R <= TREE_ROWS_MAX and n_seq * R <= TREE_TOTAL_ROWS_MAX and V >= 1, f"{what}: rows")
    _need((logits is None) == (lse is None) and (logits is not None or reduce), f"{what}: logits come with lse; nothing to do")
    if logits is not None:
        _need(logits.dtype == torch.float32 and lse.dtype == torch.float32 and n_block_rows >= 1 and row0 >= 0
              and row0 + n_block_rows <= n_seq * R and logits.numel() >= n_block_rows * V and lse.numel() >= n_block_rows,
              f"{what}: logits (n_block_rows, V) fp32 and lse of a block inside the pass's rows")
    _need(not reduce or (1 <= top <= TREE_TOP_MAX and n_columns >= 1), f"{what}: 1 <= top <= {TREE_TOP_MAX}, columns >= 1")
    _dev(logits, lse, ep, et, ne, edge_lp, mp, ml, mi, nm)
    out, ptrs = None, (None,) * 6
    if reduce:
        dev = edge_lp.device
        f = lambda *s, dtype=torch.float32: torch.empty(*s, dtype=dtype, device=dev)  # noqa: E731
        out = dict(logprob_sum=f(n_seq, n_columns), count=f(n_seq, n_columns, dtype=torch.int64), mean=f(n_seq, n_columns),
                   log_posterior=f(n_seq, n_columns), ranking=f(n_seq, top, dtype=torch.int64),
                   prediction=f(n_seq, dtype=torch.int64))
        ptrs = tuple(_ptr(out[k]) for k in ("logprob_sum", "count", "mean", "log_posterior", "ranking", "prediction"))
    rc = _lib.load().fvqa_trie_score(_ptr(logits), _ptr(lse), int(row0), int(n_block_rows), _ptr(ep), _ptr(et), _ptr(ne),
                                     _ptr(edge_lp), _ptr(mp), _ptr(ml), _ptr(mi), _ptr(nm), *ptrs, n_seq, R, E, MU,
                                     max(int(n_columns), 1), V, int(top), 1 if by_mean else 0, 1 if reduce else 0, _stream())
    _lib.check(rc, "fvqa_trie_score")
    return out


FLIPPED_TASKS = ("vqa", "vaq", "qav")


def flipped_pick(mean: dict, count: dict, weights, answer=None):
    """The pick over the tasks' per-option means (include/fvqa.h fvqa_flipped_pick). mean / count: {task: (B, O) fp32 / int64} for
    the requested tasks of FLIPPED_TASKS; weights: three floats (vqa, vaq, qav); answer (B,) int64 or None ->
    (total (B, O) fp32, prediction (B,) int64, prediction_t (3, B) int64, gold_loss (B, 3) fp32 or None)."""
    _need(len(mean) >= 1 and set(mean) == set(count) and set(mean) <= set(FLIPPED_TASKS), "flipped_pick: tasks of vqa, vaq, qav")
    _need(len(weights) == 3, "flipped_pick: three weights")
    first = next(iter(mean.values()))
    _need(first.dim() == 2, "flipped_pick: means are (B, O)")
    B, O = first.shape
    _need(1 <= B <= 65535 and 1 <= O <= 64, "flipped_pick: 1..64 options")
    _dev(*mean.values(), *count.values(), answer)
    table = []
    for t in mean:
        table += _of(_F32, B * O, **{"mean_" + t: mean[t]}) + _of(_I64, B * O, **{"count_" + t: count[t]})
    if answer is not None:
        table += _of(_I64, B, answer=answer)
    _table("flipped_pick", table)
    dev = first.device
    total = torch.empty(B, O, dtype=_F32, device=dev)
    pred = torch.empty(B, dtype=_I64, device=dev)
    pred_t = torch.empty(3, B, dtype=_I64, device=dev)
    gold = None if answer is None else torch.empty(B, 3, dtype=_F32, device=dev)
    rc = _lib.load().fvqa_flipped_pick(*[_ptr(mean.get(t)) for t in FLIPPED_TASKS], *[_ptr(count.get(t)) for t in FLIPPED_TASKS],
                                       *[float(w) for w in weights], _ptr(answer), _ptr(total), _ptr(pred), _ptr(pred_t),
                                       _ptr(gold), B, O, _stream())
    _lib.check(rc, "fvqa_flipped_pick")
    return total, pred, pred_t, gold


def _token_step(what, logits, n_logits, emb, x_next, ids, n_ids, table, *, pos64=None, n_pos64=0, ids_name="ids",
                temperature=0.0, u=None, u_shape=(), u_longer=False, top_k=0, repetition_penalty=1.0):
    """The operand checks of the token-step family (decode_next*, spec_step, trie_jump_step, beam_step*), under the entry's name
    `what`: logits (n_logits, V) fp32, emb of V rows and x_next's dtype, x_next (n_logits, D), ids of n_ids rows, int64; `table` rows
    (name, tensor, dtype, numel) for the entry's other operands; pos64 None or (n_pos64,) int64; the sampling keywords: under
    temperature > 0, u fp32 of u_shape (one dimension: that many elements, more with u_longer), top_k >= 0 and
    repetition_penalty >= 1. -> (V, D, S). Nothing is launched here."""
    _need(logits.dim() == 2 and logits.dtype == _F32 and logits.shape[0] == n_logits, f"{what}: logits ({n_logits}, V) fp32")
    V = logits.shape[1]
    _need(emb.dim() == 2 and emb.shape[0] == V and x_next.dtype == emb.dtype, f"{what}: emb (V, D) and x_next of one dtype")
    D = emb.shape[1]
    _need(tuple(x_next.shape) == (n_logits, D), f"{what}: x_next ({n_logits}, D), a row per row of logits")
    _need(ids.dim() == 2 and ids.shape[0] == n_ids and ids.dtype == _I64, f"{what}: {ids_name} (B, S) int64, B = {n_ids} rows")
    _table(what, table)
    _need(pos64 is None or (pos64.dtype == _I64 and pos64.numel() == n_pos64), f"{what}: pos64 ({n_pos64},) int64")
    if temperature != 0:
        _need(u is not None and u.dtype == _F32 and
              (tuple(u.shape) == u_shape if len(u_shape) > 1 else u.numel() == u_shape[0] or (u_longer and u.numel() > u_shape[0])),
              f"{what}: sampling needs u {u_shape} fp32")
    _need(int(top_k) == top_k and top_k >= 0 and repetition_penalty >= 1, f"{what}: top_k >= 0, repetition_penalty >= 1")
    return V, D, ids.shape[1]


def _trie_args(what: str, node, trie):
    """(node, trie) -> the five trie arguments of an entry (node_first, edge_token, edge_child, n_nodes, n_edges); without a trie
    (and without node: the two come together) three None and two 0. `trie`: a compiled constraint (fvqa.constrain.TokenTrie
    .to(device), or any object with node_first, edge_token, edge_child int32 tensors)."""
    _need((trie is None) == (node is None), f"{what}: node and trie come together")
    if trie is None:
        return None, None, None, 0, 0
    nf, et, ec = trie.node_first, trie.edge_token, trie.edge_child
    for t in (nf, et, ec):
        _need(torch.is_tensor(t) and t.dtype == _I32 and t.dim() == 1 and t.is_contiguous(),
              f"{what}: node_first, edge_token, edge_child are contiguous int32 vectors")
    _need(nf.numel() >= 2 and et.numel() == ec.numel(), f"{what}: node_first (n_nodes + 1,), edge_token / edge_child (n_edges,)")
    return nf, et, ec, nf.numel() - 1, et.numel()


def decode_next(logits, emb, ids, pos, done, x_next, token, n_kept, n_active, *, u=None, pos64=None, temperature: float = 0.0,
                top_p: float = 1.0, eos_id: int = 2, stop_at_eos: bool = True):
    """The token step of the generation API (include/fvqa.h fvqa_decode_next): logits (B, V) fp32 -> the picked token written
    into ids (B, S) int64 at pos + 1, pos (B,) int32 advanced, done (B,) int32 raised on EOS / at the end of the sequence,
    x_next (B, D) = emb[token], token / n_kept (B,) int32, n_active (1,) int32 = rows still running, pos64 (B,) int64 = pos
    after the step (what attn_decode reads). u (B,) fp32 in [0, 1) is needed when temperature > 0."""
    _dev(logits, emb, ids, pos, done, x_next, token, n_kept, n_active, u, pos64)
    B = _lead(logits)
    V, D, S = _token_step("decode_next", logits, B, emb, x_next, ids, B,
                          _of(_I32, B, pos=pos, done=done, token=token, n_kept=n_kept) + _of(_I32, 1, n_active=n_active),
                          pos64=pos64, n_pos64=B, temperature=temperature, u=u, u_shape=(B,))
    rc = _lib.load(emb.dtype).fvqa_decode_next(_ptr(logits), _ptr(u), _ptr(emb), float(temperature), float(top_p), int(eos_id),
                                               1 if stop_at_eos else 0, _ptr(ids), _ptr(pos), _ptr(done), _ptr(x_next),
                                               _ptr(token), _ptr(n_kept), _ptr(n_active), _ptr(pos64), B, V, D, S,
                                               dt_code(emb.dtype), _stream())
    _lib.check(rc, "fvqa_decode_next")
    return token


def _ex_table(B, pos, done, gen_start, token, n_kept, logprob, n_active, counter):
    """The operands decode_next_ex, _trie and _stream share, one per row or one per launch."""
    return (_of(_I32, B, pos=pos, done=done, gen_start=gen_start, token=token, n_kept=n_kept) + _of(_F32, B, logprob=logprob) +
            _of(_I32, 1, n_active=n_active, counter=counter))


def decode_next_ex(logits, emb, ids, pos, done, gen_start, x_next, token, n_kept, logprob, n_active, counter, *, u=None,
                   pos64=None, temperature: float = 0.0, top_p: float = 1.0, top_k: int = 0, repetition_penalty: float = 1.0,
                   eos_id: int = 2, stop_at_eos: bool = True):
    """decode_next with top-k, a repetition penalty and the token's log-probability (include/fvqa.h fvqa_decode_next_ex states
    the rule). On top of decode_next's operands: gen_start (B,) int32 — the ids at positions gen_start .. pos of a row are the
    tokens the penalty applies to —, logprob (B,) fp32 out (log_softmax of the RAW logits at the token; 0 where none was
    picked), counter: one int32 word the caller zeroed once (the library keeps no ticket for this entry)."""
    _dev(logits, emb, ids, pos, done, gen_start, x_next, token, n_kept, logprob, n_active, counter, u, pos64)
    B = _lead(logits)
    V, D, S = _token_step("decode_next_ex", logits, B, emb, x_next, ids, B,
                          _ex_table(B, pos, done, gen_start, token, n_kept, logprob, n_active, counter), pos64=pos64, n_pos64=B,
                          temperature=temperature, u=u, u_shape=(B,), top_k=top_k, repetition_penalty=repetition_penalty)
    rc = _lib.load(emb.dtype).fvqa_decode_next_ex(_ptr(logits), _ptr(u), _ptr(emb), float(temperature), float(top_p), int(top_k),
                                                  float(repetition_penalty), int(eos_id), 1 if stop_at_eos else 0, _ptr(ids),
                                                  _ptr(pos), _ptr(done), _ptr(gen_start), _ptr(x_next), _ptr(token),
                                                  _ptr(n_kept), _ptr(logprob), _ptr(n_active), _ptr(counter), _ptr(pos64), B, V,
                                                  D, S, dt_code(emb.dtype), _stream())
    _lib.check(rc, "fvqa_decode_next_ex")
    return token


def decode_next_rules(logits, emb, ids, pos, done, gen_start, x_next, token, n_kept, logprob, n_active, counter, *, u=None,
                      pos64=None, temperature: float = 0.0, top_p: float = 1.0, top_k: int = 0, repetition_penalty: float = 1.0,
                      eos_id: int = 2, stop_at_eos: bool = True, min_p: float = 0.0, no_repeat_ngram: int = 0,
                      min_new_tokens: int = 0):
    """decode_next_ex with three more pick rules (include/fvqa.h fvqa_decode_next_rules states them): min_p in [0, 1) — a token
    is also kept only if its probability is at least min_p times the largest —, no_repeat_ngram n >= 0 — the tokens that would
    repeat an n-gram of the generated ids are banned —, min_new_tokens m >= 0 — the EOS is banned while fewer than m tokens are
    generated (needs stop_at_eos). A banned token takes no part in the pick. All three at 0: decode_next_ex's results."""
    _dev(logits, emb, ids, pos, done, gen_start, x_next, token, n_kept, logprob, n_active, counter, u, pos64)
    B = _lead(logits)
    V, D, S = _token_step("decode_next_rules", logits, B, emb, x_next, ids, B,
                          _ex_table(B, pos, done, gen_start, token, n_kept, logprob, n_active, counter), pos64=pos64, n_pos64=B,
                          temperature=temperature, u=u, u_shape=(B,), top_k=top_k, repetition_penalty=repetition_penalty)
    _need(0 <= min_p < 1, "decode_next_rules: 0 <= min_p < 1")
    _need(int(no_repeat_ngram) == no_repeat_ngram and no_repeat_ngram >= 0, "decode_next_rules: no_repeat_ngram >= 0")
    _need(int(min_new_tokens) == min_new_tokens and min_new_tokens >= 0, "decode_next_rules: min_new_tokens >= 0")
    _need(min_new_tokens == 0 or stop_at_eos, "decode_next_rules: min_new_tokens holds the EOS back: it needs stop_at_eos")
    rc = _lib.load(emb.dtype).fvqa_decode_next_rules(_ptr(logits), _ptr(u), _ptr(emb), float(temperature), float(top_p),
                                                     int(top_k), float(repetition_penalty), int(eos_id), 1 if stop_at_eos else 0,
                                                     _ptr(ids), _ptr(pos), _ptr(done), _ptr(gen_start), _ptr(x_next), _ptr(token),
                                                     _ptr(n_kept), _ptr(logprob), _ptr(n_active), _ptr(counter), _ptr(pos64), B, V,
                                                     D, S, dt_code(emb.dtype), _stream(), float(min_p), int(no_repeat_ngram),
                                                     int(min_new_tokens))
    _lib.check(rc, "fvqa_decode_next_rules")
    return token


VOTE_SAMPLES_MAX = 64    # the most samples per prompt fvqa_sample_vote takes (csrc/vote.hip)


def sample_vote(tokens, score):
    """A vote over the samples of each prompt (include/fvqa.h fvqa_sample_vote): tokens (B, n, steps) int32, -1 padded, score
    (B, n) fp32 -> {"group", "votes" (B, n) int32, "winner", "n_groups" (B,) int32, "share" (B,) fp32}. Samples with equal token
    rows form a group; the largest group wins, ties by the larger score of its first sample, then by the lower index."""
    _dev(tokens, score)
    _need(tokens.dim() == 3 and tokens.dtype == _I32 and tokens.is_contiguous(), "sample_vote: tokens (B, n, steps) int32")
    B, n, steps = tokens.shape
    _need(B >= 1 and 1 <= n <= VOTE_SAMPLES_MAX and steps >= 1, f"sample_vote: 1 <= n <= {VOTE_SAMPLES_MAX}, steps >= 1")
    _need(tuple(score.shape) == (B, n) and score.dtype == _F32 and score.is_contiguous(), "sample_vote: score (B, n) fp32")
    i32 = dict(dtype=_I32, device=tokens.device)
    out = {"group": torch.empty(B, n, **i32), "votes": torch.empty(B, n, **i32), "winner": torch.empty(B, **i32),
           "n_groups": torch.empty(B, **i32), "share": torch.empty(B, dtype=_F32, device=tokens.device)}
    rc = _lib.load().fvqa_sample_vote(_ptr(tokens), _ptr(score), _ptr(out["group"]), _ptr(out["votes"]), _ptr(out["winner"]),
                                      _ptr(out["n_groups"]), _ptr(out["share"]), B, n, steps, _stream())
    _lib.check(rc, "fvqa_sample_vote")
    return out


LOOKUP_NGRAM_MAX = 4     # the longest n-gram fvqa_spec_step's prompt lookup matches (csrc/spec.hip GMAX)


def _pass_rows(what: str, w):
    """w (B, T) int32, the tokens a pass of up to T rows per sequence was fed -> (B, T)."""
    _need(w.dim() == 2 and w.dtype == _I32, f"{what}: w (B, T) int32")
    B, T = w.shape
    _need(1 <= T <= SUFFIX_MAX and 1 <= B <= 65535 and B * T <= 65535, f"{what}: 1 <= T <= {SUFFIX_MAX}, B * T <= 65535")
    return B, T


def _sample_operands(what, u, gen_start, n_kept, n_slots, B, max_new_tokens, temperature, top_p, top_k, repetition_penalty):
    """The operands the sampled draft-and-verify steps add: u (max_new_tokens, B) fp32, gen_start (B,) int32, n_kept of n_slots
    int32, and fvqa_decode_next_ex's parameters with temperature > 0."""
    _need(temperature > 0, f"{what}: temperature > 0 (temperature == 0 is the entry without _sample)")
    _need(0 < top_p <= 1, f"{what}: 0 < top_p <= 1")
    _need(int(top_k) == top_k and top_k >= 0 and repetition_penalty >= 1, f"{what}: top_k >= 0, repetition_penalty >= 1")
    _need(u is not None and u.dtype == _F32 and tuple(u.shape) == (int(max_new_tokens), B),
          f"{what}: u (max_new_tokens, B) = ({int(max_new_tokens)}, {B}) fp32")
    _table(what, _of(_I32, B, gen_start=gen_start) + _of(_I32, n_slots, n_kept=n_kept))


def _spec_step(what, sampling, logits, emb, ids, pos, done, n_generated, w, length, start, x_next, token, logprob, n_committed,
               n_drafted, n_active, counter, max_new_tokens, draft_tokens, lookup_ngram, pos64, eos_id, stop_at_eos):
    """spec_step (sampling None) and spec_step_sample (sampling = (u, gen_start, n_kept, temperature, top_p, top_k,
    repetition_penalty)) under the entry's name `what`: one set of operand checks, then fvqa_<what>."""
    sampled = sampling is not None
    u, gen_start, n_kept, temperature, top_p, top_k, repetition_penalty = sampling if sampled else (None,) * 7

    def only(*operands):                 # what the sampled entry has in these places on top of the plain one's
        return operands if sampled else ()
    _dev(logits, emb, ids, pos, done, n_generated, *only(gen_start), w, length, start, x_next, token, *only(n_kept), logprob,
         n_committed, n_drafted, n_active, counter, draft_tokens, pos64, *only(u))
    B, T = _pass_rows(what, w)
    V, D, S = _token_step(what, logits, B * T, emb, x_next, ids, B,
                          _of(_I32, B, pos=pos, done=done, n_generated=n_generated, len=length, start=start,
                              n_committed=n_committed, n_drafted=n_drafted) + _of(_I32, 1, n_active=n_active, counter=counter) +
                          _of(_I32, B * T, token=token) + _of(_F32, B * T, logprob=logprob), pos64=pos64, n_pos64=B)
    _need(int(max_new_tokens) == max_new_tokens and max_new_tokens >= 1, f"{what}: max_new_tokens >= 1")
    if sampled:
        _sample_operands(what, u, gen_start, n_kept, B * T, B, max_new_tokens, temperature, top_p, top_k, repetition_penalty)
    if draft_tokens is None:
        _need(int(lookup_ngram) == lookup_ngram and 1 <= lookup_ngram <= LOOKUP_NGRAM_MAX,
              f"{what}: 1 <= lookup_ngram <= {LOOKUP_NGRAM_MAX}")
    else:
        _need(draft_tokens.dtype == _I32 and tuple(draft_tokens.shape) == (B, int(max_new_tokens)),
              f"{what}: draft_tokens (B, max_new_tokens) int32")
    params = (float(temperature), float(top_p), int(top_k), float(repetition_penalty)) if sampled else ()
    rc = getattr(_lib.load(emb.dtype), "fvqa_" + what)(
        _ptr(logits), *map(_ptr, only(u)), _ptr(emb), _ptr(draft_tokens), int(lookup_ngram),
        *params, int(eos_id), 1 if stop_at_eos else 0, int(max_new_tokens), _ptr(ids), _ptr(pos), _ptr(done), _ptr(n_generated),
        *map(_ptr, only(gen_start)), _ptr(w), _ptr(length), _ptr(start), _ptr(x_next), _ptr(token), *map(_ptr, only(n_kept)),
        _ptr(logprob), _ptr(n_committed), _ptr(n_drafted), _ptr(n_active), _ptr(counter), _ptr(pos64), B, T, V, D, S,
        dt_code(emb.dtype), _stream())
    _lib.check(rc, "fvqa_" + what)
    return token


def spec_step(logits, emb, ids, pos, done, n_generated, w, length, start, x_next, token, logprob, n_committed, n_drafted,
              n_active, counter, *, max_new_tokens: int, draft_tokens=None, lookup_ngram: int = 2, pos64=None, eos_id: int = 2,
              stop_at_eos: bool = True):
    """The token step of draft-and-verify greedy decoding (include/fvqa.h fvqa_spec_step states the rule). logits (B*T, V) fp32:
    row n*T + j was computed at position pos[n] + j on the token w[n, j] (j = 0: the last committed token, ids[n, pos[n]]).
    In/out: ids (B, S) int64, pos / done / n_generated / length (B,) int32, w (B, T) int32. Out: start (B,) int32, x_next (B*T, D),
    token (B, T) int32 (-1 padded), logprob (B, T) fp32 (0 padded), n_committed / n_drafted (B,) int32, n_active (1,) int32,
    pos64 (B,) int64 or None. counter: one int32 word the caller zeroed once. draft_tokens (B, max_new_tokens) int32: the drafts
    are read from it at each row's n_generated; None: prompt lookup with n-grams of up to lookup_ngram tokens."""
    return _spec_step("spec_step", None, logits, emb, ids, pos, done, n_generated, w, length, start, x_next, token, logprob,
                      n_committed, n_drafted, n_active, counter, max_new_tokens, draft_tokens, lookup_ngram, pos64, eos_id,
                      stop_at_eos)


def spec_step_sample(logits, emb, ids, pos, done, n_generated, gen_start, w, length, start, x_next, token, n_kept, logprob,
                     n_committed, n_drafted, n_active, counter, *, u, max_new_tokens: int, temperature: float, top_p: float = 1.0,
                     top_k: int = 0, repetition_penalty: float = 1.0, draft_tokens=None, lookup_ngram: int = 2, pos64=None,
                     eos_id: int = 2, stop_at_eos: bool = True):
    """spec_step under sampling (include/fvqa.h fvqa_spec_step_sample states the rule): every row of a step is picked by
    decode_next_ex's rule with the draw of its token index, u[n_generated + i, n], and a draft is accepted iff it equals the
    token sampled in front of it. On top of spec_step's operands: u (max_new_tokens, B) fp32 — the plain loop's draws —,
    gen_start (B,) int32, n_kept (B, T) int32 out (0 padded), temperature > 0, top_p, top_k, repetition_penalty."""
    return _spec_step("spec_step_sample", (u, gen_start, n_kept, temperature, top_p, top_k, repetition_penalty), logits, emb,
                      ids, pos, done, n_generated, w, length, start, x_next, token, logprob, n_committed, n_drafted, n_active,
                      counter, max_new_tokens, draft_tokens, lookup_ngram, pos64, eos_id, stop_at_eos)


def trie_jump_step(logits, emb, ids, pos, done, n_generated, node, w, length, start, x_next, token, logprob_pick, logprob_fed,
                   n_committed, n_active, counter, trie, *, max_new_tokens: int, chain_eos: bool = True,
                   want_logprobs: bool = False, pos64=None, eos_id: int = 2):
    """The token step of jump-forward constrained greedy decoding (include/fvqa.h fvqa_trie_jump_step states the rule). logits
    (B*T, V) fp32: row n*T + j was computed on the token w[n, j]; the pick is made on row length[n] - 1. In/out: ids (B, S) int64,
    pos / done / n_generated / node / length (B,) int32, w (B, T) int32. Out: start (B,) int32, x_next (B*T, D), token (B, T) int32
    (-1 padded), logprob_pick (B,) and logprob_fed (B, T) fp32, n_committed (B,) int32, n_active (1,) int32, pos64 (B,) int64 or
    None. counter: one int32 word the caller zeroed once. `trie`: a fvqa.constrain.TokenTrie on the device; None (with node None):
    every row is unconstrained."""
    nf, et, ec, n_nodes, n_edges = _trie_args("trie_jump_step", node, trie)
    _dev(logits, emb, ids, pos, done, n_generated, node, w, length, start, x_next, token, logprob_pick, logprob_fed, n_committed,
         n_active, counter, pos64, nf, et, ec)
    B, T = _pass_rows("trie_jump_step", w)
    V, D, S = _token_step("trie_jump_step", logits, B * T, emb, x_next, ids, B,
                          _of(_I32, B, pos=pos, done=done, n_generated=n_generated, len=length, start=start,
                              n_committed=n_committed, **({} if node is None else {"node": node})) +
                          _of(_I32, 1, n_active=n_active, counter=counter) + _of(_I32, B * T, token=token) +
                          _of(_F32, B, logprob_pick=logprob_pick) + _of(_F32, B * T, logprob_fed=logprob_fed),
                          pos64=pos64, n_pos64=B)
    _need(int(max_new_tokens) == max_new_tokens and max_new_tokens >= 1, "trie_jump_step: max_new_tokens >= 1")
    rc = _lib.load(emb.dtype).fvqa_trie_jump_step(_ptr(logits), _ptr(emb), _ptr(nf), _ptr(et), _ptr(ec), n_nodes, n_edges,
                                                  int(eos_id), int(max_new_tokens), 1 if chain_eos else 0,
                                                  1 if want_logprobs else 0, _ptr(ids), _ptr(pos), _ptr(done), _ptr(n_generated),
                                                  _ptr(node), _ptr(w), _ptr(length), _ptr(start), _ptr(pos64), _ptr(x_next),
                                                  _ptr(token), _ptr(logprob_pick), _ptr(logprob_fed), _ptr(n_committed),
                                                  _ptr(n_active), _ptr(counter), B, T, V, D, S, dt_code(emb.dtype), _stream())
    _lib.check(rc, "fvqa_trie_jump_step")
    return token


TREE_SPEC_ROWS_MAX = 64      # rows of a sequence per pass fvqa_tree_spec_step takes (csrc/treespec.hip RMAX)
TREE_SPEC_WALK = 32          # tokens one step commits at the most: columns of token / logprob / path (csrc/treespec.hip WALK)


def _tree_spec_step(what, sampling, logits, emb, plan, ids, pos, done, n_generated, node, length, start, x_next, depth, end,
                    tile_anc, path, n_path, start_old, token, logprob, n_committed, n_drafted, n_active, n_on_trie, counter,
                    max_new_tokens, pos64, eos_id, stop_at_eos):
    """tree_spec_step (sampling None) and tree_spec_step_sample (sampling = (u, gen_start, n_kept, temperature, top_p, top_k,
    repetition_penalty)) under the entry's name `what`: one set of operand checks, then fvqa_<what>."""
    sampled = sampling is not None
    u, gen_start, n_kept, temperature, top_p, top_k, repetition_penalty = sampling if sampled else (None,) * 7

    def only(*operands):                 # what the sampled entry has in these places on top of the plain one's
        return operands if sampled else ()
    names = ("n_plan", "token", "depth", "end", "parent")
    _need(isinstance(plan, dict) and all(torch.is_tensor(plan.get(k)) for k in names), f"{what}: plan holds {names}")
    pn, pt, pd, pe, pp = (plan[k] for k in names)
    _dev(logits, emb, pn, pt, pd, pe, pp, ids, pos, done, n_generated, node, length, start, x_next, depth, end, tile_anc, path,
         n_path, start_old, token, logprob, n_committed, n_drafted, n_active, n_on_trie, counter, pos64,
         *only(u, gen_start, n_kept))
    B = pos.numel()
    _need(B >= 1 and logits.dim() == 2 and logits.shape[0] % B == 0 and x_next.dim() == 2 and x_next.shape[0] % B == 0,
          f"{what}: logits (B*R_in, V) and x_next (B*R_out, D) for the B of pos")
    R_in, R_out = logits.shape[0] // B, x_next.shape[0] // B
    _need(1 <= R_in <= TREE_SPEC_ROWS_MAX and 1 <= R_out <= TREE_SPEC_ROWS_MAX and B * max(R_in, R_out) <= 65535,
          f"{what}: 1 <= rows per sequence <= {TREE_SPEC_ROWS_MAX}, B * rows <= 65535")
    _need(pt.dim() in (1, 2) and pt.shape[-1] >= 1 and (pt.dim() == 1 or pt.shape[0] == B),
          f"{what}: plan tables are (P,) — shared — or (B, P)")
    P, per = int(pt.shape[-1]), pt.dim() == 2
    tiles = (R_out + TREE_TILE - 1) // TREE_TILE
    W = TREE_SPEC_WALK
    # (_token_step's checks with x_next at the rows of the NEXT pass: R_out need not be R_in)
    _need(logits.dtype == _F32, f"{what}: logits ({B * R_in}, V) fp32")
    V = logits.shape[1]
    _need(emb.dim() == 2 and emb.shape[0] == V and x_next.dtype == emb.dtype and x_next.shape[1] == emb.shape[1],
          f"{what}: emb (V, D) and x_next ({B * R_out}, D) of one dtype")
    D = emb.shape[1]
    _need(ids.dim() == 2 and ids.shape[0] == B and ids.dtype == _I64, f"{what}: ids (B, S) int64, B = {B} rows")
    S = ids.shape[1]
    _table(what, _of(_I32, B if per else 1, n_plan=pn) +
           _of(_I32, (B if per else 1) * P, plan_token=pt, plan_depth=pd, plan_end=pe, plan_parent=pp) +
           _of(_I32, B, pos=pos, done=done, n_generated=n_generated, node=node, len=length, start=start, n_path=n_path,
               start_old=start_old, n_committed=n_committed, n_drafted=n_drafted) +
           _of(_I32, 1, n_active=n_active, n_on_trie=n_on_trie) + _of(_I32, 2, counter=counter) +
           _of(_I32, B * R_out, depth=depth, end=end) + _of(_I32, B * tiles * TREE_TILE, tile_anc=tile_anc) +
           _of(_I32, B * W, token=token, path=path) + _of(_F32, B * W, logprob=logprob))
    _need(pos64 is None or (pos64.dtype == _I64 and pos64.numel() == B), f"{what}: pos64 ({B},) int64")
    _need(int(max_new_tokens) == max_new_tokens and max_new_tokens >= 1, f"{what}: max_new_tokens >= 1")
    if sampled:
        _sample_operands(what, u, gen_start, n_kept, B * W, B, max_new_tokens, temperature, top_p, top_k, repetition_penalty)
    params = (float(temperature), float(top_p), int(top_k), float(repetition_penalty)) if sampled else ()
    rc = getattr(_lib.load(emb.dtype), "fvqa_" + what)(
        _ptr(logits), *map(_ptr, only(u)), _ptr(emb), _ptr(pn), _ptr(pt), _ptr(pd), _ptr(pe), _ptr(pp), P, P if per else 0,
        *params, int(eos_id), 1 if stop_at_eos else 0, int(max_new_tokens), _ptr(ids), _ptr(pos), _ptr(done), _ptr(n_generated),
        *map(_ptr, only(gen_start)), _ptr(node), _ptr(length), _ptr(start), _ptr(x_next), _ptr(depth), _ptr(end), _ptr(tile_anc),
        _ptr(path), _ptr(n_path), _ptr(start_old), _ptr(token), *map(_ptr, only(n_kept)), _ptr(logprob), _ptr(n_committed),
        _ptr(n_drafted), _ptr(n_active), _ptr(n_on_trie), _ptr(counter), _ptr(pos64), B, R_in, R_out, V, D, S,
        dt_code(emb.dtype), _stream())
    _lib.check(rc, "fvqa_" + what)
    return token


def tree_spec_step(logits, emb, plan, ids, pos, done, n_generated, node, length, start, x_next, depth, end, tile_anc, path,
                   n_path, start_old, token, logprob, n_committed, n_drafted, n_active, n_on_trie, counter, *,
                   max_new_tokens: int, pos64=None, eos_id: int = 2, stop_at_eos: bool = True):
    """The token step of tree-shaped draft verification (include/fvqa.h fvqa_tree_spec_step states the rule). logits (B*R_in, V)
    fp32: row n*R_in + j is local row j of the pass the step verifies. plan: dict of int32 device tensors — n_plan (1,) with
    token, depth, end, parent (P,): ONE plan shared by every sequence; or n_plan (B,) with (B, P) tables: a plan per sequence.
    In/out: ids (B, S) int64, pos / done / n_generated / node / length (B,) int32. Out: start (B,) int32, x_next (B*R_out, D) —
    R_out, the rows per sequence of the NEXT pass, is read off x_next —, depth / end (B*R_out) and tile_anc (B * ceil(R_out / 32)
    * 32) int32: the next pass's operands of attn_suffix_tree (with `length` as its n_rows); path (B, 32), n_path, start_old (B,)
    int32 for kv_tree_commit; token (B, 32) int32 (-1 padded), logprob (B, 32) fp32 (0 padded), n_committed / n_drafted (B,) int32,
    n_active / n_on_trie (1,) int32, pos64 (B,) int64 or None. counter: TWO int32 words the caller zeroed once."""
    return _tree_spec_step("tree_spec_step", None, logits, emb, plan, ids, pos, done, n_generated, node, length, start, x_next,
                           depth, end, tile_anc, path, n_path, start_old, token, logprob, n_committed, n_drafted, n_active,
                           n_on_trie, counter, max_new_tokens, pos64, eos_id, stop_at_eos)


def tree_spec_step_sample(logits, emb, plan, ids, pos, done, n_generated, gen_start, node, length, start, x_next, depth, end,
                          tile_anc, path, n_path, start_old, token, n_kept, logprob, n_committed, n_drafted, n_active, n_on_trie,
                          counter, *, u, max_new_tokens: int, temperature: float, top_p: float = 1.0, top_k: int = 0,
                          repetition_penalty: float = 1.0, pos64=None, eos_id: int = 2, stop_at_eos: bool = True):
    """tree_spec_step under sampling (include/fvqa.h fvqa_tree_spec_step_sample states the rule): every commit of a step is
    picked by decode_next_ex's rule with the draw of its token index, u[n_generated + i, n], and the walk moves to the child
    under the sampled token. On top of tree_spec_step's operands: u (max_new_tokens, B) fp32, gen_start (B,) int32, n_kept
    (B, 32) int32 out (0 padded), temperature > 0, top_p, top_k, repetition_penalty."""
    return _tree_spec_step("tree_spec_step_sample", (u, gen_start, n_kept, temperature, top_p, top_k, repetition_penalty), logits,
                           emb, plan, ids, pos, done, n_generated, node, length, start, x_next, depth, end, tile_anc, path, n_path,
                           start_old, token, logprob, n_committed, n_drafted, n_active, n_on_trie, counter, max_new_tokens, pos64,
                           eos_id, stop_at_eos)


def kv_tree_commit(qkv_cache, qkv_rows, path, n_path, start_old, rope, *, n_seq: int, S: int, H: int, Dh: int, A: int,
                   cache_rotated: bool):
    """The cache append of the accepted path (include/fvqa.h fvqa_kv_tree_commit): qkv_cache (L, n_seq*S + A, 3*D), qkv_rows
    (L, n_seq*R, 3*D) the RAW rows every layer of the tree pass kept; path (n_seq, 32), n_path, start_old (n_seq,) int32 as
    tree_spec_step wrote them. One launch over all layers: the k (in the cache's convention) and v of row path[n, i] go to cache
    row n*S + start_old[n] + i for i < n_path[n]; nothing else is written."""
    what = "kv_tree_commit"
    _dev(qkv_cache, qkv_rows, path, n_path, start_old)
    D = H * Dh
    _need(qkv_cache.dim() == 3 and qkv_rows.dim() == 3 and qkv_cache.dtype == qkv_rows.dtype
          and qkv_cache.shape[0] == qkv_rows.shape[0] and qkv_cache.shape[2] == qkv_rows.shape[2] == 3 * D,
          f"{what}: qkv_cache (L, n_seq*S + A, 3*D) and qkv_rows (L, n_seq*R, 3*D) of one dtype")
    L = qkv_cache.shape[0]
    _need(Dh == 128 and n_seq >= 1 and qkv_cache.shape[1] == n_seq * S + A and qkv_rows.shape[1] % n_seq == 0 and A >= 0,
          f"{what}: head_dim 128, cache rows = n_seq*S + A, rows a multiple of n_seq")
    R = qkv_rows.shape[1] // n_seq
    _need(1 <= R <= TREE_SPEC_ROWS_MAX and n_seq <= 65535 and L <= 65535, f"{what}: 1 <= rows per sequence <= {TREE_SPEC_ROWS_MAX}")
    _table(what, _of(_I32, n_seq * TREE_SPEC_WALK, path=path) + _of(_I32, n_seq, n_path=n_path, start_old=start_old))
    cos_t, sin_t = _rope_tables(rope, S, Dh, what)
    _need(cos_t is not None or not cache_rotated, f"{what}: a rotated cache needs the rope tables")
    rc = _lib.load(qkv_cache.dtype).fvqa_kv_tree_commit(_ptr(qkv_cache), _ptr(qkv_rows), _ptr(path), _ptr(n_path),
                                                        _ptr(start_old), _ptr(cos_t), _ptr(sin_t), n_seq, R, S, H, Dh, A, L,
                                                        1 if cache_rotated else 0, dt_code(qkv_cache.dtype), _stream())
    _lib.check(rc, "fvqa_kv_tree_commit")
    return qkv_cache


def decode_next_trie(logits, emb, ids, pos, done, gen_start, x_next, token, n_kept, logprob, n_active, counter, node, trie, *,
                     u=None, pos64=None, temperature: float = 0.0, top_p: float = 1.0, top_k: int = 0,
                     repetition_penalty: float = 1.0, eos_id: int = 2, stop_at_eos: bool = True):
    """decode_next_ex under a trie of allowed answers (include/fvqa.h fvqa_decode_next_trie states the rule). On top of
    decode_next_ex's operands: node (B,) int32, in and out — the trie node of each row, -1: unconstrained —, and `trie`, a
    fvqa.constrain.TokenTrie on the device (node_first / edge_token / edge_child int32)."""
    nf, et, ec, n_nodes, n_edges = _trie_args("decode_next_trie", node, trie)
    _dev(logits, emb, ids, pos, done, gen_start, x_next, token, n_kept, logprob, n_active, counter, u, pos64, node, nf, et, ec)
    B = _lead(logits)
    V, D, S = _token_step("decode_next_trie", logits, B, emb, x_next, ids, B,
                          _ex_table(B, pos, done, gen_start, token, n_kept, logprob, n_active, counter) + _of(_I32, B, node=node),
                          pos64=pos64, n_pos64=B, temperature=temperature, u=u, u_shape=(B,), top_k=top_k,
                          repetition_penalty=repetition_penalty)
    rc = _lib.load(emb.dtype).fvqa_decode_next_trie(_ptr(logits), _ptr(u), _ptr(emb), float(temperature), float(top_p),
                                                    int(top_k), float(repetition_penalty), int(eos_id), 1 if stop_at_eos else 0,
                                                    _ptr(ids), _ptr(pos), _ptr(done), _ptr(gen_start), _ptr(x_next), _ptr(token),
                                                    _ptr(n_kept), _ptr(logprob), _ptr(n_active), _ptr(counter), _ptr(pos64),
                                                    _ptr(node), _ptr(nf), _ptr(et), _ptr(ec), n_nodes, n_edges, B, V, D, S,
                                                    dt_code(emb.dtype), _stream())
    _lib.check(rc, "fvqa_decode_next_trie")
    return token


def decode_next_pair(logits, emb, ids, pos, done, gen_start, x_next, token, n_kept, n_plausible, logprob, n_active, counter, *,
                     alpha: float, beta: float, node=None, trie=None, u=None, pos64=None, temperature: float = 0.0,
                     top_p: float = 1.0, top_k: int = 0, repetition_penalty: float = 1.0, eos_id: int = 2,
                     stop_at_eos: bool = True):
    """The token step of contrastive decoding (include/fvqa.h fvqa_decode_next_pair states the rule): decode_next_ex — with
    `node` and `trie`, decode_next_trie — on B PAIRS of rows. logits (2B, V), ids (2B, S), pos / done / pos64 (2B,) and x_next
    (2B, D) hold the B positive rows followed by their B twins; gen_start, token, n_kept, n_plausible, node (B,) int32, logprob
    and u (B,) fp32 are per pair (gen_start and u may be longer: their first B entries are read). n_active counts pairs."""
    nf, et, ec, n_nodes, n_edges = _trie_args("decode_next_pair", node, trie)
    _dev(logits, emb, ids, pos, done, gen_start, x_next, token, n_kept, n_plausible, logprob, n_active, counter, u, pos64, node,
         nf, et, ec)
    B2 = _lead(logits)
    _need(B2 > 0 and B2 % 2 == 0, "decode_next_pair: logits (2B, V) fp32")
    B = B2 // 2
    V, D, S = _token_step("decode_next_pair", logits, B2, emb, x_next, ids, B2,
                          _of(_I32, B2, pos=pos, done=done) + _of(_F32, B, logprob=logprob) +
                          _of(_I32, B, token=token, n_kept=n_kept, n_plausible=n_plausible, **({} if node is None else {"node": node})) +
                          _of(_I32, 1, n_active=n_active, counter=counter), pos64=pos64, n_pos64=B2,
                          temperature=temperature, u=u, u_shape=(B,), u_longer=True, top_k=top_k,
                          repetition_penalty=repetition_penalty)
    _need(gen_start.dtype == _I32 and gen_start.numel() >= B, "decode_next_pair: gen_start (B,) int32")
    _need(alpha >= 0 and 0 <= beta <= 1, "decode_next_pair: alpha >= 0, 0 <= beta <= 1")
    rc = _lib.load(emb.dtype).fvqa_decode_next_pair(_ptr(logits), _ptr(u), _ptr(emb), float(temperature), float(top_p),
                                                    int(top_k), float(repetition_penalty), float(alpha), float(beta),
                                                    int(eos_id), 1 if stop_at_eos else 0, _ptr(ids), _ptr(pos), _ptr(done),
                                                    _ptr(gen_start), _ptr(x_next), _ptr(token), _ptr(n_kept), _ptr(n_plausible),
                                                    _ptr(logprob), _ptr(n_active), _ptr(counter), _ptr(pos64), _ptr(node),
                                                    _ptr(nf), _ptr(et), _ptr(ec), n_nodes, n_edges, B, V, D, S,
                                                    dt_code(emb.dtype), _stream())
    _lib.check(rc, "fvqa_decode_next_pair")
    return token


def decode_next_stream(logits, emb, ids, pos, done, gen_start, x_next, token, n_kept, logprob, n_active, counter, req, budget,
                       out_tokens, out_n_generated, *, out_logprob=None, node=None, trie=None, u=None, pos64=None,
                       temperature: float = 0.0, top_p: float = 1.0, top_k: int = 0, repetition_penalty: float = 1.0,
                       eos_id: int = 2, stop_at_eos: bool = True):
    """The token step of in-flight batching (include/fvqa.h fvqa_decode_next_stream states the rule): decode_next_ex — with `node`
    and `trie`, decode_next_trie — on B slots that hold requests. On top of their operands: req (B,) int32 — the request in each
    slot, -1: none —, budget (N,) int32, out_tokens (N, W) int32, out_n_generated (N,) int32, out_logprob (N, W) fp32 or None;
    u is (W, N) fp32: a slot at token index i of request r reads u[i, r]."""
    nf, et, ec, n_nodes, n_edges = _trie_args("decode_next_stream", node, trie)
    _dev(logits, emb, ids, pos, done, gen_start, x_next, token, n_kept, logprob, n_active, counter, req, budget, out_tokens,
         out_n_generated, out_logprob, u, pos64, node, nf, et, ec)
    _need(out_tokens.dim() == 2 and out_tokens.dtype == _I32 and out_tokens.shape[0] >= 1 and out_tokens.shape[1] >= 1,
          "decode_next_stream: out_tokens (N, W) int32")
    N, W = out_tokens.shape
    B = _lead(logits)
    V, D, S = _token_step("decode_next_stream", logits, B, emb, x_next, ids, B,
                          _ex_table(B, pos, done, gen_start, token, n_kept, logprob, n_active, counter) +
                          _of(_I32, B, req=req, **({} if node is None else {"node": node})) +
                          _of(_I32, N, budget=budget, out_n_generated=out_n_generated), pos64=pos64, n_pos64=B,
                          temperature=temperature, u=u, u_shape=(W, N), top_k=top_k, repetition_penalty=repetition_penalty)
    _need(out_logprob is None or (out_logprob.dtype == _F32 and tuple(out_logprob.shape) == (N, W)),
          "decode_next_stream: out_logprob (N, W) fp32")
    rc = _lib.load(emb.dtype).fvqa_decode_next_stream(
        _ptr(logits), _ptr(u), _ptr(emb), float(temperature), float(top_p), int(top_k), float(repetition_penalty), int(eos_id),
        1 if stop_at_eos else 0, _ptr(ids), _ptr(pos), _ptr(done), _ptr(gen_start), _ptr(x_next), _ptr(token), _ptr(n_kept),
        _ptr(logprob), _ptr(n_active), _ptr(counter), _ptr(pos64), _ptr(node), _ptr(nf), _ptr(et), _ptr(ec), n_nodes, n_edges,
        _ptr(req), _ptr(budget), N, W, _ptr(out_tokens), _ptr(out_logprob), _ptr(out_n_generated), B, V, D, S,
        dt_code(emb.dtype), _stream())
    _lib.check(rc, "fvqa_decode_next_stream")
    return token


def slot_seat(slot, src, request, prompt_ids, prefix, vstart_src, logits_src, ids, pos, pos64, done, gen_start, vstart, req, lg,
              err, *, root=None, node=None):
    """Prefilled prompts take freed slots (include/fvqa.h fvqa_slot_seat). slot, src, request: three host lists of one length —
    entry j seats row src[j] of the prefill (prompt_ids (M, S) int64, prefix (M,) int64, vstart_src (M,) int32, logits_src
    (M, S, V) fp32, root (M,) int32 or None) in slot slot[j] for request request[j]. In/out per slot: ids (n, S) int64, pos / done /
    gen_start / vstart / req / node (n,) int32, pos64 (n,) int64, lg (n, V) fp32; err (1,) int32: bit 0 is raised when the device
    refused an entry (a slot or source row outside the arrays, a slot that holds a running request). Duplicate slots and duplicate
    requests are refused here."""
    slot, src, request = [int(x) for x in slot], [int(x) for x in src], [int(x) for x in request]
    _need(len(slot) == len(src) == len(request) >= 1, "slot_seat: slot, src, request of one length >= 1")
    _need(len(set(slot)) == len(slot), "slot_seat: a slot is named twice")
    _need(len(set(request)) == len(request), "slot_seat: a request is named twice")
    _need((root is None) == (node is None), "slot_seat: root and node come together")
    _dev(prompt_ids, prefix, vstart_src, logits_src, root, ids, pos, pos64, done, gen_start, vstart, req, node, lg, err)
    _need(ids.dim() == 2 and ids.dtype == torch.int64, "slot_seat: ids (n_slots, S) int64")
    n_slots, S = ids.shape
    _need(prompt_ids.dim() == 2 and prompt_ids.dtype == torch.int64 and prompt_ids.shape[1] == S,
          "slot_seat: prompt_ids (M, S) int64")
    M = prompt_ids.shape[0]
    _need(lg.dim() == 2 and lg.dtype == torch.float32 and lg.shape[0] == n_slots, "slot_seat: lg (n_slots, V) fp32")
    V = lg.shape[1]
    _need(logits_src.dtype == torch.float32 and logits_src.numel() == M * S * V, "slot_seat: logits_src (M, S, V) fp32")
    _need(prefix.dtype == torch.int64 and prefix.numel() == M, "slot_seat: prefix (M,) int64")
    for t, n in ((vstart_src, M), (pos, n_slots), (done, n_slots), (gen_start, n_slots), (vstart, n_slots), (req, n_slots),
                 (err, 1)) + (() if root is None else ((root, M), (node, n_slots))):
        _need(t.dtype == torch.int32 and t.numel() == n, "slot_seat: vstart_src / root (M,), pos / done / gen_start / vstart / req / "
                                                         "node (n_slots,), err (1,) int32")
    _need(pos64.dtype == torch.int64 and pos64.numel() == n_slots, "slot_seat: pos64 (n_slots,) int64")
    _need(len(slot) <= n_slots <= 65535, "slot_seat: at most n_slots <= 65535 entries")
    tri = torch.tensor([slot, src, request], dtype=torch.int32).to(ids.device, non_blocking=True)
    rc = _lib.load().fvqa_slot_seat(_ptr(tri[0]), _ptr(tri[1]), _ptr(tri[2]), len(slot), _ptr(prompt_ids), _ptr(prefix),
                                    _ptr(vstart_src), _ptr(logits_src), _ptr(root), M, _ptr(ids), _ptr(pos), _ptr(pos64),
                                    _ptr(done), _ptr(gen_start), _ptr(vstart), _ptr(req), _ptr(node), _ptr(lg), _ptr(err), n_slots,
                                    S, V, _stream())
    _lib.check(rc, "fvqa_slot_seat")
    return tri


BEAMS_MAX = 8            # slots per sample fvqa_beam_step takes (csrc/beam.hip KMAX)


def _beam_step(what, trie_args, logits, emb, ids_in, ids_out, pos, score, done, n_generated, pos64, parent, token, x_next, n_active,
               counter, node, num_beams, eos_id, stop_at_eos, count_any_live):
    """beam_step (trie_args None) and beam_step_trie: the same operands but for node and the trie."""
    N, K = _lead(logits), int(num_beams)
    _need(N >= 0, f"{what}: logits (B*K, V) fp32")
    _need(1 <= K <= BEAMS_MAX and K <= logits.shape[1] and N % K == 0,
          f"{what}: 1 <= num_beams <= {BEAMS_MAX}, <= V, rows a multiple of it")
    V, D, S = _token_step(what, logits, N, emb, x_next, ids_in, N,
                          _of(_I32, N, pos=pos, done=done, n_generated=n_generated, parent=parent, token=token,
                              **({} if trie_args is None else {"node": node})) + _of(_I32, 1, n_active=n_active, counter=counter) +
                          _of(_F32, N, score=score) + _of(_I64, N, pos64=pos64), ids_name="ids_in")
    _need(ids_out.dtype == _I64 and ids_out.shape == ids_in.shape and ids_in.data_ptr() != ids_out.data_ptr(),
          f"{what}: ids_in, ids_out (B*K, S) int64, two buffers")
    head = (_ptr(logits), _ptr(emb), int(eos_id), 1 if stop_at_eos else 0, 1 if count_any_live else 0, _ptr(ids_in), _ptr(ids_out),
            _ptr(pos), _ptr(score), _ptr(done), _ptr(n_generated), _ptr(pos64), _ptr(parent), _ptr(token), _ptr(x_next),
            _ptr(n_active), _ptr(counter))
    tail = (N // K, K, V, D, S, dt_code(emb.dtype), _stream())
    if trie_args is None:
        rc = _lib.load(emb.dtype).fvqa_beam_step(*head, *tail)
    else:
        nf, et, ec, n_nodes, n_edges = trie_args
        rc = _lib.load(emb.dtype).fvqa_beam_step_trie(*head, _ptr(node), _ptr(nf), _ptr(et), _ptr(ec), n_nodes, n_edges, *tail)
    _lib.check(rc, "fvqa_" + what)
    return parent, token


def beam_step(logits, emb, ids_in, ids_out, pos, score, done, n_generated, pos64, parent, token, x_next, n_active, counter, *,
              num_beams: int, eos_id: int = 2, stop_at_eos: bool = True, count_any_live: bool = False):
    """One step of beam search (include/fvqa.h fvqa_beam_step): logits (B*K, V) fp32 -> the K best continuations of each sample
    re-seated into its K slots: ids_out (B*K, S) int64 (ids_in is only read), pos / done / n_generated (B*K,) int32 and score
    (B*K,) fp32 in place, pos64 (B*K,) int64, parent / token (B*K,) int32, x_next (B*K, D), n_active (1,) int32. counter: one
    int32 word the caller zeroed once."""
    _dev(logits, emb, ids_in, ids_out, pos, score, done, n_generated, pos64, parent, token, x_next, n_active, counter)
    return _beam_step("beam_step", None, logits, emb, ids_in, ids_out, pos, score, done, n_generated, pos64, parent, token, x_next,
                      n_active, counter, None, num_beams, eos_id, stop_at_eos, count_any_live)


def beam_step_trie(logits, emb, ids_in, ids_out, pos, score, done, n_generated, pos64, parent, token, x_next, n_active, counter,
                   node, trie, *, num_beams: int, eos_id: int = 2, stop_at_eos: bool = True, count_any_live: bool = False):
    """beam_step under a trie of allowed answers (include/fvqa.h fvqa_beam_step_trie): on top of beam_step's operands node
    (B*K,) int32, in and out — each slot's trie node, -1: unconstrained —, and `trie` as decode_next_trie takes it."""
    trie_args = _trie_args("beam_step_trie", node, trie)
    _dev(logits, emb, ids_in, ids_out, pos, score, done, n_generated, pos64, parent, token, x_next, n_active, counter, node,
         *trie_args[:3])
    return _beam_step("beam_step_trie", trie_args, logits, emb, ids_in, ids_out, pos, score, done, n_generated, pos64, parent,
                      token, x_next, n_active, counter, node, num_beams, eos_id, stop_at_eos, count_any_live)


def kv_beam_move_scratch(n_seq: int, window_rows: int, D: int, L: int, dtype) -> int:
    return int(_lib.load(dtype).fvqa_kv_beam_move_scratch(n_seq, window_rows, D, L, dt_code(dtype)))


def kv_beam_move(dst, src, src_seq, lo, hi, *, S: int, A: int, scratch=None, window_rows: int = 0, group: int = 0):
    """Cached k / v rows follow the beams (include/fvqa.h fvqa_kv_beam_move). dst (L, n_dst*S + A, 3*D), src (L, n_src*S + A, 3*D);
    for destination sequence n the rows [lo[n], hi[n]) come from sequence src_seq[n] (+ the sample's first slot when group > 0).
    scratch None: dst is another buffer than src, adapter rows go along (one launch). scratch (bytes of kv_beam_move_scratch):
    the move inside one cache through the window of window_rows rows (two launches; slots that are their own source skipped)."""
    _dev(dst, src, src_seq, lo, hi, scratch)
    _need(dst.dim() == 3 and src.dim() == 3 and dst.dtype == src.dtype and dst.shape[0] == src.shape[0]
          and dst.shape[2] == src.shape[2] and dst.shape[2] % 3 == 0, "kv_beam_move: caches (L, n*S + A, 3*D) of one dtype")
    L, D = dst.shape[0], dst.shape[2] // 3
    _need(S >= 1 and A >= 0 and dst.shape[1] > A and (dst.shape[1] - A) % S == 0 and src.shape[1] > A
          and (src.shape[1] - A) % S == 0, "kv_beam_move: rows = n*S + A")
    n_dst, n_src = (dst.shape[1] - A) // S, (src.shape[1] - A) // S
    for t in (src_seq, lo, hi):
        _need(t.dtype == torch.int32 and t.numel() == n_dst, "kv_beam_move: src_seq / lo / hi (n_dst,) int32")
    _need((D * dst.element_size()) % 16 == 0, "kv_beam_move: rows of whole 16-byte words")
    if scratch is None:
        _need(dst.data_ptr() != src.data_ptr(), "kv_beam_move: inside one cache the move needs a scratch window")
    else:
        _need(n_dst == n_src and window_rows >= 1, "kv_beam_move: one geometry and a window of >= 1 rows with scratch")
        _need(scratch.dtype == torch.uint8, "kv_beam_move: scratch is a byte buffer")
    rc = _lib.load(dst.dtype).fvqa_kv_beam_move(_ptr(dst), _ptr(src), _ptr(scratch), 0 if scratch is None else scratch.numel(),
                                                _ptr(src_seq), _ptr(lo), _ptr(hi), n_dst, n_src, int(group), S, D, L, A,
                                                int(window_rows), dt_code(dst.dtype), _stream())
    _lib.check(rc, "fvqa_kv_beam_move")
    return dst


def attn_bwd_workspace(n_seq, S, H, Dh, A) -> int:
    return int(_lib.load().fvqa_attn_bwd_workspace(n_seq, S, H, Dh, A))


def attn_bwd(d_o, qkv, o, lse_a, lse_t, gate1, gate2, vstart, dqkv, dgate1, dgate2, workspace,
             n_seq, S, H, Dh, A, F, rope=None, prerotated=False):
    """`workspace`: attn_bwd_workspace(...) bytes, ZEROED once when allocated (its head holds the fused
    kernel's arrival counters, which every call leaves at zero again)."""
    _dev(d_o, qkv, o, lse_a, lse_t, gate1, gate2, vstart, dqkv, dgate1, dgate2, workspace)
    cos_t, sin_t = _rope_tables(rope, S, Dh, "attn_bwd")
    D = _attn_shapes(qkv, n_seq, S, H, Dh, A)
    _need(dqkv.dtype == qkv.dtype and dqkv.shape == qkv.shape, "attn_bwd: dqkv shape")
    for t in (d_o, o):
        _need(t.dtype == qkv.dtype and tuple(t.shape) == (n_seq * S, D), "attn_bwd: o/d_o shape")
    for t in (lse_a, lse_t):
        _need(t.dtype == torch.float32 and t.numel() == n_seq * H * S, "attn_bwd: lse shape")
    for t in (gate1, gate2, dgate1, dgate2):
        _need(t.dtype == torch.float32 and t.numel() == H, "attn_bwd: gate shape")
    _need(vstart.dtype == torch.int32 and vstart.numel() == n_seq, "attn_bwd: vstart")
    wbytes = workspace.numel() * workspace.element_size()
    _need(wbytes >= attn_bwd_workspace(n_seq, S, H, Dh, A), "attn_bwd: workspace too small")
    # prerotated: q, k in `qkv` were rotated by gemm_nt_rope; dqkv still receives the gradients of the raw projections
    fn = _lib.load(qkv.dtype).fvqa_attn_bwd_rotated if prerotated else _lib.load(qkv.dtype).fvqa_attn_bwd
    _need(not prerotated or cos_t is not None, "attn_bwd: prerotated needs the rope tables")
    rc = fn(_ptr(d_o), _ptr(qkv), _ptr(o), _ptr(lse_a), _ptr(lse_t), _ptr(gate1), _ptr(gate2), _ptr(vstart), _ptr(cos_t),
            _ptr(sin_t), _ptr(dqkv), _ptr(dgate1), _ptr(dgate2), _ptr(workspace), wbytes, n_seq, S, H, Dh, A, F,
            dt_code(qkv.dtype), _stream())
    _lib.check(rc, "fvqa_attn_bwd")
    return dqkv


# ------------------------------------------------------------------------------------ heads / splice
def visual_proj_fwd(video, W, temporal, vf_raw, vf_tok):
    _dev(video, W, temporal, vf_raw, vf_tok)
    R, K = video.shape
    D = W.shape[0]
    F = temporal.shape[0]
    _need(video.dtype == W.dtype == temporal.dtype == vf_raw.dtype == torch.float32, "visual_proj_fwd: fp32")
    _need(W.shape[1] == K and temporal.shape[1] == D and R % F == 0, "visual_proj_fwd: shapes")
    _need(tuple(vf_raw.shape) == (R, D) and tuple(vf_tok.shape) == (R, D), "visual_proj_fwd: out shapes")
    rc = _lib.load(vf_tok.dtype).fvqa_visual_proj_fwd(_ptr(video), _ptr(W), _ptr(temporal), _ptr(vf_raw), _ptr(vf_tok), R, F,
                                          K, D, dt_code(vf_tok.dtype), _stream())
    _lib.check(rc, "fvqa_visual_proj_fwd")


def visual_proj_bwd(d_tok, d_qav, video, dW, dtemporal):
    _dev(d_tok, d_qav, video, dW, dtemporal)
    R, K = video.shape
    D = dW.shape[0]
    F = dtemporal.shape[0]
    for t in (d_tok, d_qav):
        _need(t is None or (t.dtype == torch.float32 and tuple(t.shape) == (R, D)), "visual_proj_bwd: d_tok/d_qav")
    _need(dW.dtype == dtemporal.dtype == video.dtype == torch.float32, "visual_proj_bwd: fp32")
    _need(tuple(dW.shape) == (D, K) and tuple(dtemporal.shape) == (F, D) and R % F == 0, "visual_proj_bwd: shapes")
    rc = _lib.load().fvqa_visual_proj_bwd(_ptr(d_tok), _ptr(d_qav), _ptr(video), _ptr(dW), _ptr(dtemporal), R, F,
                                          K, D, _stream())
    _lib.check(rc, "fvqa_visual_proj_bwd")


def _proj_srcs(srcs, rows: int, dim: int, what: str):
    """[(x, w)] -> the fvqa_proj_src array: x (rows, k) fp32, w (dim, k) fp32 — a weight or a column range of one (forward),
    the same range of its gradient (backward); both may be row-pitched views."""
    arr = (_lib.ProjSrc * max(1, len(srcs)))()
    for i, (x, w) in enumerate(srcs):
        _dev(x, w, rows_strided=True)
        _need(x.dtype == w.dtype == torch.float32, f"{what}: fp32 sources")
        _need(x.shape[0] == rows and w.shape[0] == dim and x.shape[1] == w.shape[1], f"{what}: source shapes")
        arr[i].x, arr[i].w, arr[i].ldx, arr[i].ldw, arr[i].k = x.data_ptr(), w.data_ptr(), x.stride(0), w.stride(0), x.shape[1]
    return arr


def av_proj_fwd(srcs, out_raw, *, bias=None, temporal=None, out_tok=None):
    """out_raw (rows, dim) fp32 = sum of x·w^T over the 1..2 (x, w) sources (+ bias); with `temporal` (F, dim):
    out_tok = cast(out_raw + temporal[r % F]) in out_tok's dtype (include/fvqa.h fvqa_av_proj_fwd)."""
    _dev(out_raw, bias, temporal, out_tok)
    rows, dim = out_raw.shape
    _need(1 <= len(srcs) <= 2 and out_raw.dtype == torch.float32, "av_proj_fwd: one or two sources, fp32 output")
    _need((temporal is None) == (out_tok is None), "av_proj_fwd: temporal and out_tok come together")
    _need(bias is None or (bias.dtype == torch.float32 and tuple(bias.shape) == (dim,)), "av_proj_fwd: bias")
    F, dtype = 0, torch.float32
    if temporal is not None:
        F, dtype = temporal.shape[0], out_tok.dtype
        _need(temporal.dtype == torch.float32 and temporal.shape[1] == dim and tuple(out_tok.shape) == (rows, dim),
              "av_proj_fwd: temporal / out_tok shapes")
    arr = _proj_srcs(srcs, rows, dim, "av_proj_fwd")
    rc = _lib.load(dtype).fvqa_av_proj_fwd(C.addressof(arr), len(srcs), _ptr(bias), _ptr(temporal), _ptr(out_raw), _ptr(out_tok),
                                           rows, F, dim, dt_code(dtype), _stream())
    _lib.check(rc, "fvqa_av_proj_fwd")


def av_cross_attn_fwd(q, k, v, x, n_samples: int, n_query: int, n_key: int):
    """x = softmax(q·k^T / sqrt(dim))·v over the n_key keys of each sample (include/fvqa.h fvqa_av_cross_attn_fwd)."""
    _dev(q, k, v, rows_strided=True)
    _dev(x)
    dim = x.shape[1]
    _need(q.dtype == k.dtype == v.dtype == x.dtype == torch.float32, "av_cross_attn_fwd: fp32")
    _need(tuple(q.shape) == (n_samples * n_query, dim) == tuple(x.shape), "av_cross_attn_fwd: q / x shapes")
    _need(tuple(k.shape) == (n_samples * n_key, dim) == tuple(v.shape), "av_cross_attn_fwd: k / v shapes")
    rc = _lib.load().fvqa_av_cross_attn_fwd(_ptr(q), _ptr(k), _ptr(v), _ptr(x), n_samples, n_query, n_key, dim, q.stride(0),
                                            k.stride(0), v.stride(0), 1.0 / math.sqrt(dim), _stream())
    _lib.check(rc, "fvqa_av_cross_attn_fwd")


def av_proj_bwd(d_tok, d_qav, srcs, dtemporal):
    """dW += (d_tok + d_qav)^T·x for each (x, dW) of the 0..2 trainable sources — dW a weight gradient or a column range of
    one — and dtemporal += sum_b d_tok[b] (include/fvqa.h fvqa_av_proj_bwd)."""
    _dev(d_tok, d_qav, dtemporal)
    rows, dim = d_tok.shape
    F = dtemporal.shape[0]
    for t in (d_tok, d_qav):
        _need(t is None or (t.dtype == torch.float32 and tuple(t.shape) == (rows, dim)), "av_proj_bwd: d_tok/d_qav")
    _need(dtemporal.dtype == torch.float32 and dtemporal.shape[1] == dim and rows % F == 0 and len(srcs) <= 2,
          "av_proj_bwd: shapes")
    arr = _proj_srcs(srcs, rows, dim, "av_proj_bwd")
    rc = _lib.load().fvqa_av_proj_bwd(_ptr(d_tok), _ptr(d_qav), C.addressof(arr), len(srcs), _ptr(dtemporal), rows, F, dim,
                                      _stream())
    _lib.check(rc, "fvqa_av_proj_bwd")


def av_cross_attn_bwd(q, k, v, dx, dq, dk, dv, n_samples: int, n_query: int, n_key: int):
    """dq, dk, dv (written) of x = softmax(q·k^T / sqrt(dim))·v from dx; k | v and dk | dv may be column ranges of one buffer
    (include/fvqa.h fvqa_av_cross_attn_bwd)."""
    _dev(q, k, v, dq, dk, dv, rows_strided=True)
    _dev(dx)
    dim = dx.shape[1]
    _need(all(t.dtype == torch.float32 for t in (q, k, v, dx, dq, dk, dv)), "av_cross_attn_bwd: fp32")
    _need(tuple(q.shape) == (n_samples * n_query, dim) == tuple(dx.shape) == tuple(dq.shape), "av_cross_attn_bwd: q / dx / dq shapes")
    _need(tuple(k.shape) == (n_samples * n_key, dim) == tuple(v.shape) == tuple(dk.shape) == tuple(dv.shape),
          "av_cross_attn_bwd: k / v / dk / dv shapes")
    rc = _lib.load().fvqa_av_cross_attn_bwd(_ptr(q), _ptr(k), _ptr(v), _ptr(dx), _ptr(dq), _ptr(dk), _ptr(dv), n_samples, n_query,
                                            n_key, dim, q.stride(0), k.stride(0), v.stride(0), dq.stride(0), dk.stride(0),
                                            dv.stride(0), 1.0 / math.sqrt(dim), _stream())
    _lib.check(rc, "fvqa_av_cross_attn_bwd")


def av_proj_dx(g0, g1, w, dx):
    """dx (rows, k) = (g0 + g1)·w (written): g0, g1 (rows, dim) fp32 — g1 or None —, w (dim, k) a weight or a column range of
    one (include/fvqa.h fvqa_av_proj_dx)."""
    _dev(g0, g1, w, dx, rows_strided=True)
    rows, dim = g0.shape
    k = w.shape[1]
    _need(all(t is None or t.dtype == torch.float32 for t in (g0, g1, w, dx)), "av_proj_dx: fp32")
    _need(g1 is None or (tuple(g1.shape) == (rows, dim) and g1.stride(0) == g0.stride(0)), "av_proj_dx: g1")
    _need(w.shape[0] == dim and tuple(dx.shape) == (rows, k), "av_proj_dx: shapes")
    rc = _lib.load().fvqa_av_proj_dx(_ptr(g0), _ptr(g1), _ptr(w), _ptr(dx), rows, dim, k, g0.stride(0), w.stride(0), dx.stride(0),
                                     _stream())
    _lib.check(rc, "fvqa_av_proj_dx")


def av_linear_bwd(g, srcs, dbias=None):
    """dW += g^T·x for each (x, dW) of the 1..2 sources, g (rows, dim) fp32 — a column range of a wider matrix allowed —, and
    dbias (dim) += sum_rows g (include/fvqa.h fvqa_av_linear_bwd)."""
    _dev(g, rows_strided=True)
    _dev(dbias)
    rows, dim = g.shape
    _need(g.dtype == torch.float32 and 1 <= len(srcs) <= 2, "av_linear_bwd: fp32 g, one or two sources")
    _need(dbias is None or (dbias.dtype == torch.float32 and tuple(dbias.shape) == (dim,)), "av_linear_bwd: dbias")
    arr = _proj_srcs(srcs, rows, dim, "av_linear_bwd")
    rc = _lib.load().fvqa_av_linear_bwd(_ptr(g), g.stride(0), C.addressof(arr), len(srcs), _ptr(dbias), rows, dim, _stream())
    _lib.check(rc, "fvqa_av_linear_bwd")


def embed_splice(ids, emb, vf_tok, h, n_seq, S, F, *, vstart: int = 0, zero_labels=None, index=None, mode: int = 0):
    _dev(ids, emb, vf_tok, h, zero_labels, index)
    D = emb.shape[1]
    _need(ids.dtype == torch.int64 and ids.numel() == n_seq * S, "embed_splice: ids")
    _need(emb.dtype == vf_tok.dtype == h.dtype, "embed_splice: dtype")
    _need(vf_tok.numel() == n_seq * F * D and h.numel() >= n_seq * S * D and h.shape[-1] == D, "embed_splice: shapes")
    _need(zero_labels is None or (zero_labels.dtype == torch.int64 and zero_labels.numel() == n_seq * S),
          "embed_splice: zero_labels")
    _need(index is None or (index.dtype == torch.int64 and index.numel() == n_seq * F), "embed_splice: index")
    # ids must address the table: checked on the host copy by the caller (see model.py)
    rc = _lib.load(emb.dtype).fvqa_embed_splice(_ptr(ids), _ptr(emb), _ptr(vf_tok), _ptr(zero_labels), _ptr(index), _ptr(h),
                                       n_seq, S, D, F, vstart, mode, dt_code(h.dtype), _stream())
    _lib.check(rc, "fvqa_embed_splice")
    return h


def splice_bwd(dh, d_tok, n_seq, S, F, *, vstart: int = 0, index=None, mode: int = 0):
    _dev(dh, d_tok, index)
    D = dh.shape[-1]
    _need(dh.numel() >= n_seq * S * D, "splice_bwd: dh")
    _need(d_tok.dtype == torch.float32 and d_tok.numel() == n_seq * F * D, "splice_bwd: d_tok")
    _need(index is None or (index.dtype == torch.int64 and index.numel() == n_seq * F), "splice_bwd: index")
    rc = _lib.load(dh.dtype).fvqa_splice_bwd(_ptr(dh), _ptr(index), _ptr(d_tok), n_seq, S, D, F, vstart, mode,
                                     dt_code(dh.dtype), _stream())
    _lib.check(rc, "fvqa_splice_bwd")


def ce_fwd(logits, labels, lse, rowloss, loss_sum, n_seq, S, V, ignore_index: int):
    _dev(logits, labels, lse, rowloss, loss_sum)
    _need(logits.dtype == torch.float32 and logits.numel() == n_seq * S * V, "ce_fwd: logits")
    _need(labels.dtype == torch.int64 and labels.numel() == n_seq * S, "ce_fwd: labels")
    for t in (lse, rowloss):
        _need(t.dtype == torch.float32 and t.numel() >= n_seq * S, "ce_fwd: lse/rowloss")
    _need(loss_sum.dtype == torch.float32 and loss_sum.numel() >= 2, "ce_fwd: loss_sum")
    rc = _lib.load().fvqa_ce_fwd(_ptr(logits), _ptr(labels), _ptr(lse), _ptr(rowloss), _ptr(loss_sum), n_seq, S, V,
                                 ignore_index, _stream())
    _lib.check(rc, "fvqa_ce_fwd")


def ce_bwd(logits, labels, lse, loss_sum, gscale, dlogits, n_seq, S, V, ignore_index: int):
    _dev(logits, labels, lse, loss_sum, gscale, dlogits)
    _need(logits.dtype == torch.float32 and logits.numel() == n_seq * S * V, "ce_bwd: logits")
    _need(dlogits.numel() == n_seq * S * V, "ce_bwd: dlogits")
    _need(labels.dtype == torch.int64 and labels.numel() == n_seq * S, "ce_bwd: labels")
    _need(gscale.dtype == torch.float32 and gscale.numel() >= 1 and loss_sum.numel() >= 2, "ce_bwd: scalars")
    rc = _lib.load(dlogits.dtype).fvqa_ce_bwd(_ptr(logits), _ptr(labels), _ptr(lse), _ptr(loss_sum), _ptr(gscale), _ptr(dlogits),
                                 n_seq, S, V, ignore_index, dt_code(dlogits.dtype), _stream())
    _lib.check(rc, "fvqa_ce_bwd")


def qav_head_fwd(xn, vf_raw, labels, probs, rowloss, loss_sum, n_seq, S, D, F, tau: float):
    _dev(xn, vf_raw, labels, probs, rowloss, loss_sum)
    _need(xn.numel() >= n_seq * S * D and xn.shape[-1] == D, "qav_head_fwd: xn")
    _need(vf_raw.dtype == torch.float32 and vf_raw.numel() == n_seq * F * D, "qav_head_fwd: vf_raw")
    _need(labels.dtype == torch.int64 and labels.numel() == n_seq * S, "qav_head_fwd: labels")
    _need(probs.dtype == torch.float32 and probs.numel() >= n_seq * S * F, "qav_head_fwd: probs")
    _need(rowloss.dtype == torch.float32 and rowloss.numel() >= n_seq * S, "qav_head_fwd: rowloss")
    rc = _lib.load(xn.dtype).fvqa_qav_head_fwd(_ptr(xn), _ptr(vf_raw), _ptr(labels), _ptr(probs), _ptr(rowloss),
                                       _ptr(loss_sum), n_seq, S, D, F, float(tau), dt_code(xn.dtype), _stream())
    _lib.check(rc, "fvqa_qav_head_fwd")


def qav_head_bwd(xn, vf_raw, labels, probs, loss_sum, gscale, dxn, d_raw, n_seq, S, D, F, tau: float):
    _dev(xn, vf_raw, labels, probs, loss_sum, gscale, dxn, d_raw)
    _need(xn.numel() >= n_seq * S * D and dxn.numel() >= n_seq * S * D and dxn.dtype == xn.dtype, "qav_head_bwd: xn")
    _need(vf_raw.numel() == n_seq * F * D and d_raw.dtype == torch.float32 and d_raw.numel() == n_seq * F * D,
          "qav_head_bwd: vf")
    _need(labels.dtype == torch.int64 and labels.numel() == n_seq * S, "qav_head_bwd: labels")
    rc = _lib.load(xn.dtype).fvqa_qav_head_bwd(_ptr(xn), _ptr(vf_raw), _ptr(labels), _ptr(probs), _ptr(loss_sum),
                                       _ptr(gscale), _ptr(dxn), _ptr(d_raw), n_seq, S, D, F, float(tau),
                                       dt_code(xn.dtype), _stream())
    _lib.check(rc, "fvqa_qav_head_bwd")


# ------------------------------------------------------------------------------------ optimizer
def grad_norm_workspace(n_seg: int) -> int:
    return int(_lib.load().fvqa_grad_norm_workspace(n_seg))


def grad_unscale_norm(grad, seg_off, scale, seg_sq, found_inf, total_norm, workspace, grad_div: float = 1.0,
                      gemm_err: Optional[torch.Tensor] = None, err_lane: Optional[torch.Tensor] = None):
    """grad_div: replicas summed into `grad` (the data-parallel mean is applied here); gemm_err: the 8-byte error word of
    the GEMM workspace (gemm_error_word) — non-zero makes found_inf 2 and the optimizer step a no-op; err_lane: the fp32
    element data-parallel ranks all-reduce with the gradients (FlatParams.err_lane) — non-zero does the same on EVERY rank."""
    _dev(grad, seg_off, scale, seg_sq, found_inf, total_norm, workspace, gemm_err, err_lane)
    _need(err_lane is None or (err_lane.dtype == torch.float32 and err_lane.numel() >= 1), "grad_unscale_norm: err_lane")
    _need(grad_div >= 1.0, "grad_unscale_norm: grad_div")
    _need(gemm_err is None or gemm_err.numel() * gemm_err.element_size() >= 8, "grad_unscale_norm: gemm_err")
    n_seg = seg_off.numel() - 1
    _need(grad.dtype == torch.float32 and seg_off.dtype == torch.int64 and n_seg >= 1, "grad_unscale_norm: types")
    _need(seg_sq.numel() >= n_seg and seg_sq.dtype == torch.float32, "grad_unscale_norm: seg_sq")
    wbytes = workspace.numel() * workspace.element_size()
    rc = _lib.load().fvqa_grad_unscale_norm(_ptr(grad), _ptr(seg_off), n_seg, _ptr(scale), float(grad_div),
                                            _ptr(gemm_err), _ptr(err_lane), _ptr(seg_sq), _ptr(found_inf), _ptr(total_norm),
                                            _ptr(workspace), wbytes, _stream())
    _lib.check(rc, "fvqa_grad_unscale_norm")


def adamw_step(param, grad, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, weight_decay, step, found_inf=None):
    _dev(param, grad, exp_avg, exp_avg_sq, step, found_inf)
    n = param.numel()
    for t in (param, grad, exp_avg, exp_avg_sq):
        _need(t.dtype == torch.float32 and t.numel() == n, "adamw_step: fp32 tensors of equal size")
    rc = _lib.load().fvqa_adamw_step(_ptr(param), _ptr(grad), _ptr(exp_avg), _ptr(exp_avg_sq), n, float(lr),
                                     float(beta1), float(beta2), float(eps), float(weight_decay), _ptr(step),
                                     _ptr(found_inf), _stream())
    _lib.check(rc, "fvqa_adamw_step")


def scaler_update(step, scale, tracker, found_inf, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000):
    _dev(step, scale, tracker, found_inf)
    rc = _lib.load().fvqa_scaler_update(_ptr(step), _ptr(scale), _ptr(tracker), _ptr(found_inf),
                                        float(growth_factor), float(backoff_factor), int(growth_interval), _stream())
    _lib.check(rc, "fvqa_scaler_update")
