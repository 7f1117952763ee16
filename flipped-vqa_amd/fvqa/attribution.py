"""Which frames an answer came from: the text softmax of Attention.forward (reference llama/model.py:116-120) summarised per query
row, layer and head as F + 2 numbers — the weight on each of the F frame keys [vs, vs + F), the weight in front of the window and
the weight behind it (include/fvqa.h fvqa_attn_decode_mass states the quantity). The decode attention already holds the
probabilities in LDS; `generate(frame_attention=True)` has it write the summary (ops.attn_decode_mass) and takes the first
token's row, which the prefill computed, from the arena (`arena_mass`, ops.attn_row_mass). `summarize` reduces a result of
`generate` to one frame profile per answer. Option scoring reports the same summary for the suffix rows of every option
(`score_options(frame_attention=True)`: ops.attn_suffix_mass on the shared route, `arena_mass` on the dense one;
`summarize_options`), and `training_video_mass` reads it off a training step's arena. `contrast="blind"` says how much of an answer came from the clip; this says from
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


def training_video_mass(eng, label) -> torch.Tensor:
    """The training-time meter: between a training forward and its backward (eng.saved: the step's arena, read only), the weight
    the text softmax of the vqa stream's SCORED rows — row t of sample b with label[b, t + 1] > 0, the rows the vqa loss is made
    of — puts on the frame keys, mean over those rows, the layers and the heads -> a 0-d fp32 device tensor (None: no scored
    row). label: the batch's label["vqa"], (B, 1, S) or (B, S). The vqa stream is the arena's first B sequences (fvqa/step.py)."""
    sv = eng.saved
    if sv is None or "ar" not in sv:
        raise ValueError("training_video_mass: no forward has left its arena behind (eng.saved is empty)")
    B, S = sv["B"], sv["S"]
    b, t = torch.nonzero(torch.as_tensor(label).reshape(B, S)[:, 1:] > 0, as_tuple=True)
    if b.numel() == 0:
        return None
    n_seq = sv["ar"].qkv.shape[1] // S                       # every stream's sequences (the adapter rows are fewer than S)
    total = None
    for r0 in range(0, int(b.numel()), 65535):               # (ops.attn_row_mass takes 65535 rows a launch)
        m = arena_mass(eng, n_seq, S, b[r0:r0 + 65535], t[r0:r0 + 65535])[..., :eng.F].sum(-1)        # (L, R, H)
        total = m.sum() if total is None else total + m.sum()
    return total / float(b.numel() * eng.L * eng.H)


def summarize_options(out: dict) -> dict:
    """A result of score_options(frame_attention=True) -> {"frame_share" (B, O, F): the weight on each frame, "video_mass" (B, O):
    their sum}, both the mean over the option's SCORED rows (out["plan"].rows: the rows whose loss ranks the option), the layers
    and the heads. An option without a scored row: zeros."""
    if "frame_attention" not in out or "plan" not in out:
        raise ValueError("summarize_options: the result has no \"frame_attention\" (score_options(..., frame_attention=True))")
    fa, plan = out["frame_attention"], out["plan"]
    if fa.dim() != 6 or fa.shape[0] != plan.start.numel() or fa.shape[2] != plan.T:
        raise ValueError("summarize_options: \"frame_attention\" must be (B, O, plan.T, L, H, F + 2)")
    B, O, T = fa.shape[:3]
    F = fa.shape[-1] - 2
    n, c, t = plan.rows.unbind(1)
    live = torch.zeros(B, O, T, dtype=fa.dtype)
    live[n, c, t - plan.start[n]] = 1                                           # (every scored row lies in the suffix)
    live = live.to(fa.device)
    per_row = fa[..., :F].mean(dim=(-3, -2))                                    # (B, O, T, F)
    share = (per_row * live.unsqueeze(-1)).sum(-2) / live.sum(-1, keepdim=True).clamp(min=1)
    return {"frame_share": share, "video_mass": share.sum(-1)}


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
