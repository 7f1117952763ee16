"""Validation by scoring the answer options (reference engine.py:86-93,122-129 + llama/model_my_original_mod.py:332-377,506):
every option of a sample is run through the model, per-token cross-entropy with ignore_index 0, the option with the lowest mean
loss over its answer tokens is the prediction.

The reference runs B * n_options full sequences that differ only in their last few tokens. Two forms here:

  shared  the prompt is run ONCE per sample (option 0, the training forward in an arena of its own: every layer's k / v stay in
          the arena = the KV cache; no LM head on it), then only the SUFFIX rows of each option — from the first row that is
          scored or differs, to the last scored row — go through the layers: RMSNorm -> QKV -> fvqa_attn_suffix (several
          continuations read one cached prompt, nothing is written to it) -> WO + residual -> RMSNorm -> W1|W3 SwiGLU -> W2 +
          residual. With causal attention the hidden states in front of the first differing token are those of option 0, and
          rows behind an option's last scored row are never read, so the scored rows are what the dense form computes.
          S + n_options * T rows per sample instead of n_options * S (148 against 640 at S = 128, five options, T = 4).
  dense   the options flattened to (B * n_options, 1, S), front-end inputs repeated per option (model_my_original_mod.py:333),
          the existing forward with tail rows: the reference's computation on the step's own kernels. The fallback for batches
          the planner turns down, and what FVQA_SCORE=dense forces.

Both end in the same tail: the scored rows' losses in a compact array (fvqa_ce_fwd, shifted-label convention of fvqa/scored.py)
-> fvqa_option_pick -> individual_losses (B, n_options, S-1), per-option sum / count / mean, prediction.

score_options(contrast=...) is the scoring sibling of generate(contrast=...): the batch and its twin (the same text, the twin's
features) are scored with the same route, and the prediction is the argmin over the options with count > 0 of
mean+ + alpha * (mean+ - mean-) — host composition and a (B, n_options)-sized reduction on the device, no new kernel.

score_options(frame_attention=True) also reports where every suffix row of every option looked (fvqa/attribution.py): the shared
form's suffix attention writes the summary itself (fvqa_attn_suffix_mass), the dense form reads it off its arena (arena_mass).
"""
from __future__ import annotations

import os
from dataclasses import dataclass
from typing import Optional

import torch

from . import ops, rowpass, scored
from .generate import streams_only

ROUTES = ("shared", "dense")
DEFAULT_ROUTE = "shared"


@dataclass
class OptionPlan:
    """What plan_options found. start / length: (B,) int64 host — the suffix of sample n is rows [start[n], start[n] + length[n])
    of every option; T = max length; shared: whether the batch can take the shared form (why_dense says why not)."""
    start: torch.Tensor
    length: torch.Tensor
    T: int
    shared: bool
    why_dense: str
    rows: torch.Tensor             # (M, 3) int64: (n, c, t) of every scored row, row-major


def plan_options(text_id, label, prefix_index=None, video_start=None, F: int = 0, *, suffix_max: Optional[int] = None,
                 frames_in_suffix: bool = False, qav: bool = False) -> OptionPlan:
    """Host-only integer work. text_id, label: (B, O, S) int64 host tensors; video_start: per-sample first frame slot (or one
    int); prefix_index is not needed (the labels say where the answers are) and only checked for length when given.
    Per sample: lcp = the first position where any option differs from option 0 (S if none); row t is scored iff
    label[t + 1] > 0 (llama/model.py:348-350, ignore_index 0); start = min(lcp, first scored row) — every scored row then lies
    in the suffix, the prompt pass needs no LM head; length = last scored row of any option + 1 - start.
    Shared form iff every sample has a scored row, start >= video_start + F + 1 (no frame slot in a suffix: its inputs are token
    embeddings) and length <= ops.SUFFIX_MAX.
    The keywords are fvqa/flipped.py's; their defaults decide as ever. suffix_max: the longest suffix (None: ops.SUFFIX_MAX;
    ops.SUFFIX_WIDE_MAX for a caller that runs ops.attn_suffix_wide). frames_in_suffix: the suffix may hold frame slots (its
    inputs come from ops.suffix_embed) — the start >= video_start + F + 1 rule is dropped. qav: the QAV head's rule for a scored
    row, label[t + 1] >= 0 (ignore_index -1, llama/model.py:359-361)."""
    ids = torch.as_tensor(text_id)
    lab = torch.as_tensor(label)
    if ids.dim() != 3 or ids.shape != lab.shape:
        raise ValueError(f"plan_options: text_id {tuple(ids.shape)} and label {tuple(lab.shape)} must be (B, O, S)")
    B, O, S = ids.shape
    if prefix_index is not None and len(prefix_index) != B:
        raise ValueError("plan_options: one prefix index per sample")
    if video_start is None:
        vs = torch.zeros(B, dtype=torch.int64)
    elif isinstance(video_start, int):
        vs = torch.full((B,), video_start, dtype=torch.int64)
    else:
        vs = torch.as_tensor([int(v) for v in video_start], dtype=torch.int64)
    differs = (ids != ids[:, :1]).any(1)                                  # (B, S)
    pos = torch.arange(S)
    lcp = torch.where(differs, pos, torch.full_like(pos, S)).min(1).values
    limit = ops.SUFFIX_MAX if suffix_max is None else int(suffix_max)
    ok = (lab[:, :, 1:] >= 0) if qav else (lab[:, :, 1:] > 0)             # (B, O, S-1): row t scored
    any_t = ok.any(1)                                                     # (B, S-1)
    has = any_t.any(1)
    t = torch.arange(S - 1)
    first = torch.where(any_t, t, torch.full_like(t, S)).min(1).values
    last = torch.where(any_t, t, torch.full_like(t, -1)).max(1).values
    start = torch.minimum(lcp, first)
    length = torch.where(has, last + 1 - start, torch.zeros_like(start))
    why = ""
    if not bool(has.all()):
        why = "a sample has no scored row"
    elif not frames_in_suffix and bool((start < vs + F + 1).any()):
        why = "an option differs (or is scored) inside or in front of the frame slots"
    elif int(length.max()) > limit:
        why = f"a suffix of {int(length.max())} rows (> {limit})"
    return OptionPlan(start=start, length=length, T=int(length.max()) if B else 0, shared=not why, why_dense=why,
                      rows=torch.nonzero(ok))


def route_of(plan: OptionPlan) -> str:
    """FVQA_SCORE=shared|dense picks the form; a batch the planner turns down goes dense whatever was asked."""
    want = os.environ.get("FVQA_SCORE", "") or DEFAULT_ROUTE
    if want not in ROUTES:
        raise ValueError(f"FVQA_SCORE={want!r}: expected one of {ROUTES}")
    return want if plan.shared else "dense"


def _front_inputs(data: dict, repeat: int = 1) -> dict:
    sub = {}
    for k in ("video", "audio"):                           # (the audio-only batch has no "video")
        if k in data:
            sub[k] = data[k] if repeat == 1 else data[k].repeat_interleave(repeat, 0)
    return sub


def _pick(eng, rowloss, n_rows: int, at, entry, B: int, O: int, S: int):
    """fvqa_option_pick over rowloss (n_rows fp32 losses): its rows `at` (a slice or an int64 tensor; every other row is skipped)
    land at the entries `entry` = (n * O + c) * (S - 1) + t of individual_losses (B, O, S - 1) -> ops.option_pick's five."""
    row_map = torch.full((n_rows,), -1, dtype=torch.int64)
    row_map[at] = entry
    return ops.option_pick(rowloss, row_map.to(torch.int32).to(eng.device, non_blocking=True), n_rows, B, O, S)


def contrast_pick(mean_pos: torch.Tensor, mean_neg: torch.Tensor, count: torch.Tensor, alpha: float) -> torch.Tensor:
    """(B, O) means of the batch and of its twin, (B, O) counts -> (B,) int64: the argmin over the options with count > 0 of
    mean+ + alpha * (mean+ - mean-), the lowest index on ties (0 when no option has a scored token). Any device."""
    s = mean_pos + float(alpha) * (mean_pos - mean_neg)
    s = torch.where(count > 0, s, torch.full_like(s, float("inf")))
    O = s.shape[1]
    idx = torch.arange(O, device=s.device).expand_as(s)
    first = torch.where(s == s.min(1, keepdim=True).values, idx, torch.full_like(idx, O)).min(1).values
    return first.clamp(max=O - 1).to(torch.int64)


@torch.no_grad()
def score_options(eng, data: dict, route: Optional[str] = None, events: Optional[list] = None, *, contrast=None,
                  contrast_alpha: float = 1.0, frame_attention: bool = False):
    """-> dict(individual_losses (B, O, S-1) fp32, sum, count (int64), mean (B, O), prediction (B,) int64 — all on the device —,
    route, plan). route: None = route_of(plan). events: a list that receives (name, start, end) torch.cuda.Event triples of the
    passes (tools/score_bench.py).
    contrast (None: nothing changes; "blind" or a dict of replacement features, as generate's keyword): the twin batch is scored
    as well, by the same route. "prediction" becomes contrast_pick(mean, mean_blind, count, contrast_alpha); the result gains
    "mean_blind" (B, O), "prediction_blind" (the argmin of the twin's means: what the model answers without looking) and
    "prediction_plain" (the argmin of the batch's own means: the prediction without `contrast`). individual_losses, sum, count
    and mean stay the batch's own. Not built: negatives whose text differs.
    frame_attention (False: every call launches what it did): the result gains "frame_attention" (B, O, T, L, H, F + 2) fp32, T =
    plan.T — per suffix row j of option c of sample n (sequence position plan.start[n] + j), layer and head the summary of the
    text softmax that include/fvqa.h fvqa_attn_decode_mass defines: the weight on each frame key, in front of the window (index
    F) and behind it (index F + 1); rows j >= plan.length[n] are zeros. The shared route has the suffix attention write it
    (ops.attn_suffix_mass: the same o rows, bit for bit); the dense route reads it off its arena (attribution.arena_mass: the
    kernels generate() reports with), so the two routes check each other. attribution.summarize_options reduces it to one frame
    profile per option. ValueError with `contrast`: which of the two passes would it describe?"""
    if frame_attention and contrast is not None:
        raise ValueError("score_options: frame_attention is not built for contrast (two passes, one summary)")
    if contrast is not None:
        from .generate import _twin
        twin = _twin(data, contrast, contrast_alpha, 0.0)
    ids = data["text_id"]["vqa"]
    lab = data["label"]["vqa"]
    ids_h, lab_h = ids.cpu(), lab.cpu()
    if ids_h.dim() != 3:
        raise ValueError("score_options: text_id['vqa'] must be (B, n_options, S)")
    V = eng.V
    if int(ids_h.min()) < 0 or int(ids_h.max()) >= V:
        raise ValueError(f"text_id[vqa] outside [0, {V})")
    vs_list = [int(v) for v in data["video_start"]["vqa"]]
    plan = plan_options(ids_h, lab_h, data.get("prefix_index", {}).get("vqa"), vs_list, eng.F)
    route = route or route_of(plan)
    if route == "shared" and not plan.shared:
        raise ValueError(f"score_options: this batch cannot take the shared form ({plan.why_dense})")
    fn = _shared if route == "shared" else _dense
    fa = {} if frame_attention else None
    il, s, cnt, mean, pred = fn(eng, data, ids_h, lab_h, vs_list, plan, events, *(() if fa is None else (fa,)))
    out = dict(individual_losses=il, sum=s, count=cnt, mean=mean, prediction=pred, route=route, plan=plan)
    if fa is not None:
        out["frame_attention"] = fa["frame_attention"]
    if contrast is not None:
        blind = dict(data)
        blind.update(twin)
        _, _, _, mean_b, pred_b = fn(eng, blind, ids_h, lab_h, vs_list, plan, events)
        out.update(mean_blind=mean_b, prediction_blind=pred_b, prediction_plain=pred,
                   prediction=contrast_pick(mean, mean_b, cnt, contrast_alpha))
    return out


def _mark(events, name):
    if events is None:
        return lambda: None
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()

    def done():
        b.record()
        events.append((name, a, b))
    return done


def _suffix_rows(plan: OptionPlan, O: int):
    """(seq, pos, at) int64 host tensors of the suffix rows j < length[n] of every option, row-major over (n, c, j): the dense
    arena's sequence n * O + c, the position start[n] + j, and the row's index in a (B, O, T) array."""
    B, T = plan.start.numel(), plan.T
    live = (torch.arange(T)[None, :] < plan.length[:, None])[:, None, :].expand(B, O, T)
    n, c, j = torch.nonzero(live).unbind(1)
    return n * O + c, plan.start[n] + j, (n * O + c) * T + j


def _suffix_ids(plan: OptionPlan, ids_h, T: int):
    """Host integers of the suffix rows, (B, O, T) each: pos = start[n] + j (kept inside the sequence), ids = the token there, 0 at
    the padding rows j >= length[n]; and live (B, 1, T): j < length[n]. T >= plan.T."""
    B, O, S = ids_h.shape
    j = torch.arange(T)
    pos = (plan.start[:, None] + j[None, :]).clamp(max=S - 1)[:, None, :].expand(B, O, T)
    ids_suf = ids_h.gather(2, pos)
    live = (j[None, :] < plan.length[:, None])[:, None, :]
    return live, pos, torch.where(live, ids_suf, torch.zeros_like(ids_suf))


def _dense_mass(eng, plan: OptionPlan, B: int, O: int, S: int) -> torch.Tensor:
    """"frame_attention" of the dense form, from the arena its forward left (eng.saved): (B, O, T, L, H, F + 2)."""
    from . import attribution
    T = plan.T
    out = torch.zeros(B * O * T, eng.L, eng.H, eng.F + 2, dtype=torch.float32, device=eng.device)
    seq, pos, at = _suffix_rows(plan, O)
    for r0 in range(0, int(seq.numel()), 65535):               # (ops.attn_row_mass takes 65535 rows a launch)
        r1 = r0 + 65535
        m = attribution.arena_mass(eng, B * O, S, seq[r0:r1], pos[r0:r1])
        out[at[r0:r1].to(eng.device)] = m.permute(1, 0, 2, 3)
    return out.view(B, O, T, eng.L, eng.H, eng.F + 2)


def _dense_pass(eng, data, task, ids_h, lab_h, vs_list, video_index=None, fa=None, plan=None):
    """The B * O option sequences as ONE stream of `task` through the existing forward (tail rows: the last layer's second half
    and the head on scored rows) -> (eng.last_scored, the arena)."""
    B, O, S = ids_h.shape
    flat = ids_h.reshape(B * O, 1, S)
    sub = _front_inputs(data, O)
    sub.update({"text_id": {"vqa": flat, task: flat}, "label": {task: lab_h.reshape(B * O, 1, S)},
                "video_start": {"vqa": [vs_list[0]] * (B * O), "vaq": [vs_list[0]] * (B * O)}})
    if video_index is not None:
        sub["video_index"] = {"qav": video_index.reshape(B * O, -1)}
    with streams_only(eng, [task], "_score_arena", "scored"):
        eng.forward(sub)
        tl, ar = eng.last_scored, eng.saved["ar"]
        if fa is not None:
            fa["frame_attention"] = _dense_mass(eng, plan, B, O, S)
        eng.saved = None                                   # (no backward follows)
    return tl, ar


def _dense_pick(eng, tl, ar, plan, B: int, O: int, S: int):
    """The dense forward's compact scored rows -> ops.option_pick's five."""
    o0, rows = tl.segs[0]
    n, c, t = plan.rows.unbind(1)                          # the same row-major order as scored.lists_of over (B*O, S)
    assert tl.counts[0] == n.numel()
    return _pick(eng, ar.rowloss_c[o0:o0 + rows], rows, slice(0, n.numel()), (n * O + c) * (S - 1) + t, B, O, S)


def _dense(eng, data, ids_h, lab_h, vs_list, plan, events, fa=None):
    B, O, S = ids_h.shape
    done = _mark(events, "dense forward")
    tl, ar = _dense_pass(eng, data, "vqa", ids_h, lab_h, vs_list, fa=fa, plan=plan)
    done()
    return _dense_pick(eng, tl, ar, plan, B, O, S)


def _prompt_pass(eng, data, task, ids_h, vs_list, events, name, video_index=None) -> dict:
    """The prompt pass: option 0 of every sample as one stream of `task`, no scored row (its labels are all ignored: the head sees
    pad rows only) -> what the forward saved: ar (every layer's k / v stay in the arena = the KV cache), vstart, vf_raw."""
    B, _, S = ids_h.shape
    ids0 = ids_h[:, 0:1]
    sub = _front_inputs(data)
    sub.update({"text_id": {"vqa": ids0, task: ids0}, "video_start": {"vqa": vs_list, "vaq": vs_list},
                "label": {task: torch.full((B, 1, S), -1 if task == "qav" else 0, dtype=torch.int64)}})
    if video_index is not None:
        sub["video_index"] = {"qav": video_index}
    done = _mark(events, name)
    with streams_only(eng, [task], "_score_arena", "scored"):
        eng.forward(sub)
        saved, eng.saved = eng.saved, None                 # (no backward follows)
    done()
    return saved


def _suffix_lengths(eng, plan: OptionPlan):
    """plan.start and plan.length as the suffix kernels take them: (B,) int32 on the device."""
    mv = lambda t: t.to(eng.device, non_blocking=True)     # noqa: E731
    return mv(plan.start.to(torch.int32)), mv(plan.length.to(torch.int32))


def _suffix_layers(eng, saved: dict, start_d, len_d, x, B: int, O: int, T: int, S: int, *, wide: bool = False, mass=None):
    """x (B * O * T, D), the suffix rows' inputs, through the L layers against the cache the prompt pass left (several continuations
    read one cached prompt, nothing is written) -> the last layer's output. The one place that picks the suffix attention:
    ops.attn_suffix (T <= ops.SUFFIX_MAX), ops.attn_suffix_wide (wide: T <= ops.SUFFIX_WIDE_MAX) or ops.attn_suffix_mass (mass
    (L, rows, H, F + 2) fp32: the same attention, each layer writes its slice of the frame-attention summary)."""
    ar, m_ = saved["ar"], eng.model
    b = rowpass.buffers(eng, B * O * T, xin=False, lg=False)
    rotated = rowpass.cache_rotated(eng)

    def attn(i, qkv, o):
        rest = (*m_.gate_views(i), saved["vstart"], start_d, len_d, (eng.cos, eng.sin), B, O, T, S, eng.H, eng.Dh, eng.A, eng.F)
        if mass is not None:
            ops.attn_suffix_mass(qkv, ar.qkv[i], o, mass[i], *rest, cache_rotated=rotated)
        else:
            (ops.attn_suffix_wide if wide else ops.attn_suffix)(qkv, ar.qkv[i], o, *rest, cache_rotated=rotated)
    return rowpass.layers(eng, b, attn, x)


def _scored_head(eng, x, plan: OptionPlan, lab_h, B: int, O: int, T: int, S: int):
    """The scored rows of x (B * O * T, D): gather -> final norm -> LM head -> cross-entropy (one "sequence" of `rows` positions,
    fvqa/scored.py) -> ops.option_pick's five."""
    dev = eng.device
    mv = lambda t: t.to(dev, non_blocking=True)            # noqa: E731
    e = lambda *s, dtype=eng.dtype: torch.empty(*s, dtype=dtype, device=dev)  # noqa: E731
    n, c, t = plan.rows.unbind(1)
    M = int(n.numel())
    rows = scored.rows_of(M)
    gidx = torch.zeros(rows, dtype=torch.int32)
    gidx[:M] = ((n * O + c) * T + (t - plan.start[n])).to(torch.int32)
    lab_shift = torch.zeros(rows, dtype=torch.int64)
    lab_shift[1:M + 1] = lab_h[n, c, t + 1]
    xg, xf = e(rows, eng.D), e(rows, eng.D)
    lg = e(rows, eng.V, dtype=torch.float32)
    lse, rowloss = e(rows, dtype=torch.float32), e(rows, dtype=torch.float32)
    loss_sum = torch.zeros(2, dtype=torch.float32, device=dev)
    ops.gather_rows(x, xg, ops.row_segs([mv(gidx)], [0, rows], B * O * T))
    rowpass.head(eng, xg, xf, lg)
    ops.ce_fwd(lg, mv(lab_shift), lse, rowloss, loss_sum, 1, rows, eng.V, 0)
    return _pick(eng, rowloss, rows, slice(0, M), (n * O + c) * (S - 1) + t, B, O, S)


def _shared(eng, data, ids_h, lab_h, vs_list, plan, events, fa=None):
    dev = eng.device
    B, O, S = ids_h.shape
    T = plan.T
    ids_suf = _suffix_ids(plan, ids_h, T)[2]               # (host integers, staged in front of the prompt pass)
    saved = _prompt_pass(eng, data, "vqa", ids_h, vs_list, events, "prompt pass")
    done = _mark(events, "suffix pass")
    start_d, len_d = _suffix_lengths(eng, plan)
    R = B * O * T
    # token embeddings: the planner keeps frame slots out of a suffix
    x = eng.pack.emb[ids_suf.reshape(-1).to(dev, non_blocking=True)].contiguous()
    mass = None if fa is None else torch.empty(eng.L, R, eng.H, eng.F + 2, dtype=torch.float32, device=dev)
    x = _suffix_layers(eng, saved, start_d, len_d, x, B, O, T, S, mass=mass)
    if fa is not None:
        fa["frame_attention"] = mass.permute(1, 0, 2, 3).reshape(B, O, T, eng.L, eng.H, eng.F + 2)
    out = _scored_head(eng, x, plan, lab_h, B, O, T, S)
    done()
    return out
