"""The row pass every KV-cached evaluation path runs, once: R rows — new tokens (fvqa/generate.py) or the suffix rows of answer
options (fvqa/score.py) — through the L layers against the cache a prefill left in its arena, then the final norm and the LM head.
Per layer: RMSNorm -> QKV row -> cached attention -> WO + residual -> RMSNorm -> W1|W3 -> SwiGLU -> W2 + residual. The paths
differ in ONE call, the cached attention (ops.attn_decode, ops.attn_suffix_append, ops.attn_suffix: which cache, which position
operands), so the caller supplies it. Every launch is an `ops.*` call looked up on the module when it is issued."""
from __future__ import annotations

import types

import torch

from . import ops


def cache_rotated(eng) -> bool:
    """What the cached-attention entries are told about the keys a prefill left in the arena: ROTATED keys (fp32 build; bf16
    build with RoPE in the QKV epilogue, the default) unless the bf16 build runs with FVQA_ROPE_IN_GEMM=0 (raw keys, rotated on
    the fly): cache_rotated = !attn_rope_fused || rope_in_gemm."""
    return not (ops.attn_rope_fused(eng.dtype) and not ops.rope_in_gemm(eng.dtype))


def buffers(eng, R: int, *, xin: bool = True, lg: bool = True) -> types.SimpleNamespace:
    """The buffers of a pass of R rows, allocated per call: xn, hn, h, xb, o (R, D), qkv (R, 3 D), ab (R, 2 Hf), z (R, Hf) and,
    where wanted, xin (R, D) — the rows a token step writes for the pass to read — and lg (R, V) fp32."""
    D, Hf = eng.D, eng.Hf
    e = lambda *s, dtype=eng.dtype: torch.empty(*s, dtype=dtype, device=eng.device)  # noqa: E731
    b = types.SimpleNamespace(R=R, xn=e(R, D), hn=e(R, D), h=e(R, D), xb=e(R, D), o=e(R, D), qkv=e(R, 3 * D), ab=e(R, 2 * Hf),
                              z=e(R, Hf))
    if xin:
        b.xin = e(R, D)
    if lg:
        b.lg = e(R, eng.V, dtype=torch.float32)
    return b


def layers(eng, b, attn, x=None) -> torch.Tensor:
    """x (R, D; default b.xin) through the L layers -> the last layer's output, in x or b.xb (the two alternate; x is written).
    attn(i, qkv_rows, o_rows): layer i's cached attention, from the raw projections b.qkv into b.o."""
    pk, R = eng.pack, b.R
    x, x2 = b.xin if x is None else x, b.xb
    for i in range(eng.L):
        ops.rmsnorm_fwd(x, pk.an[i], b.xn, None, eng.eps, rows=R)
        ops.gemm_nt(b.xn, pk.wqkv[i], b.qkv)
        attn(i, b.qkv, b.o)
        ops.gemm_nt(b.o, pk.wo[i], b.h, residual=x)
        ops.rmsnorm_fwd(b.h, pk.fn[i], b.hn, None, eng.eps, rows=R)
        ops.gemm_nt(b.hn, pk.w13[i], b.ab)
        ops.swiglu_fwd(b.ab, b.z, R, eng.Hf)
        ops.gemm_nt(b.z, pk.w2[i], x2, residual=b.h)
        x, x2 = x2, x
    return x


def head(eng, x, xn, lg) -> None:
    """The final norm of the rows x into xn and the LM head into lg (fp32), one logits row per row."""
    ops.rmsnorm_fwd(x, eng.pack.norm, xn, None, eng.eps, rows=x.shape[0])
    ops.gemm_nt(xn, eng.pack.wout, lg)
