"""Which frames an answer came from: the text softmax of Attention.forward (reference llama/model.py:116-120) summarised per query
row, layer and head as F + 2 numbers — the weight on each of the F frame keys [vs, vs + F), the weight in front of the window and
the weight behind it (include/fvqa.h fvqa_attn_decode_mass states the quantity). The decode attention already holds the
probabilities in LDS; `generate(frame_attention=True)` has it write the summary (ops.attn_decode_mass) and takes the first
token's row, which the prefill computed, from the arena (`arena_mass`, ops.attn_row_mass). `summarize` reduces a result of
`generate` to one frame profile per answer. `contrast="blind"` says how much of an answer came from the clip; this says from
which frames, and whether a trained gate2 lets the answer rows look at the video at all."""
from __future__ import annotations

import torch

from . import ops, rowpass


def arena_mass(eng, n_seq: int, S: int, seq, pos) -> torch.Tensor:
    """The summary of the rows (seq[r], pos[r]) of the arena the engine's last forward left behind (eng.saved: any forward
    that has not been followed by its backward or dropped) -> (L, R, H, F + 2) fp32. seq, pos: R integers each (tensors or
    lists): the sequence of the arena's n_seq and the position inside S of each query row. One launch per layer."""
    sv = eng.saved
    if sv is None or "ar" not in sv:
        raise ValueError("arena_mass: no forward has left its arena behind (eng.saved is empty)")
    qkv, vstart = sv["ar"].qkv, sv["vstart"]
    if qkv.dim() != 3 or qkv.shape[0] != eng.L or qkv.shape[1] != n_seq * S + eng.A:
        raise ValueError(f"arena_mass: the arena holds {tuple(qkv.shape)}, not {eng.L} layers of {n_seq} x {S} + {eng.A} rows")
    dev = eng.device
    seq = torch.as_tensor(seq).to(device=dev, dtype=torch.int32).contiguous().view(-1)
    pos = torch.as_tensor(pos).to(device=dev, dtype=torch.int32).contiguous().view(-1)
    R = seq.numel()
    if R == 0 or pos.numel() != R:
        raise ValueError("arena_mass: seq and pos hold one entry per row, at least one")
    mass = torch.empty(eng.L, R, eng.H, eng.F + 2, dtype=torch.float32, device=dev)
    rotated = rowpass.cache_rotated(eng)
    for i in range(eng.L):
        ops.attn_row_mass(qkv[i], seq, pos, mass[i], eng.model.gate_views(i)[1], vstart, (eng.cos, eng.sin), n_seq, S, eng.H,
                          eng.Dh, eng.A, eng.F, cache_rotated=rotated)
    return mass


def summarize(out: dict) -> dict:
    """A result of generate(frame_attention=True) -> {"frame_share" (B[, n], F): the weight on each frame, "video_mass" (B[, n]):
    their sum}, both the mean over the generated tokens (tokens != -1), the layers and the heads. A row without a token: zeros."""
    if "frame_attention" not in out:
        raise ValueError("summarize: the result has no \"frame_attention\" (generate(..., frame_attention=True))")
    fa, tok = out["frame_attention"], out["tokens"]
    if fa.dim() != tok.dim() + 3 or tuple(fa.shape[:tok.dim()]) != tuple(tok.shape):
        raise ValueError("summarize: \"frame_attention\" must be \"tokens\" x (L, H, F + 2)")
    F = fa.shape[-1] - 2
    live = (tok != -1).to(fa.dtype)
    per_token = fa[..., :F].mean(dim=(-3, -2))                                  # (B[, n], steps, F)
    share = (per_token * live.unsqueeze(-1)).sum(-2) / live.sum(-1, keepdim=True).clamp(min=1)
    return {"frame_share": share, "video_mass": share.sum(-1)}
