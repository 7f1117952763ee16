"""Validation by all three flipped tasks: the answer options of a sample are ranked by the VQA loss (fvqa/score.py), by the VAQ
loss — how well the model predicts the QUESTION from the clip and each candidate answer — and by the QAV loss — how well it
predicts the FRAME ORDER from the question and each candidate answer. The reference trains the three losses (engine.py:27 sums
them) and validates with the first only; the validation batch of its reader already carries text_id["vaq"] and text_id["qav"],
(B, O, S), one row per option (llama/tokenizer.py:126-131,184-189).

`option_rows` builds the labels and frame indices of every option AT ITS OWN POSITIONS (see its docstring for the deviation from
the reference's reader). `score_flipped` scores the requested tasks and combines them: per task the per-option sum / count /
mean, total = sum_t w_t * mean_t, the argmin of the total and of each task, and each task's mean at the gold option — the
validation-time flipped losses.

The VQA entries are score_options' own. VAQ and QAV have the two routes score_options has:

  dense   the options flattened to B * O sequences and run through the existing forward as ONE stream of that task
          (generate.streams_only): VAQ with its own video_start, QAV with embed_splice(mode=1) at per-row indices, no frame window
          and the QAV head's per-row losses. The fallback for whatever the planner turns down; FVQA_SCORE=dense forces it.
  shared  the prompt pass once per task (option 0; for QAV a stream whose frame rows lie behind the shared prompt), then the
          suffix rows through rowpass.layers with ops.attn_suffix_wide (up to 64 rows per option) on inputs made by
          ops.suffix_embed (token rows, frame rows, padding), the LM head + cross-entropy (VAQ) or the QAV head on those rows.
"""
from __future__ import annotations

import os
from typing import Optional

import torch

from . import ops, score

TASKS = ("vqa", "vaq", "qav")
# The route a task takes when neither `route` nor FVQA_SCORE names one: shared for all three — measured faster than dense in
# every interleaved pair at 7B, 32 layers, bf16, 8 x 5 options (profiles/score_flipped.log: VAQ 31 ms against 58 ms at 26 suffix
# rows, 44 against 59 at 50; QAV 28 against 58).
DEFAULT_ROUTE = {"vqa": score.DEFAULT_ROUTE, "vaq": "shared", "qav": "shared"}
SUFFIX_LIMIT = {"vaq": ops.SUFFIX_WIDE_MAX, "qav": ops.SUFFIX_WIDE_MAX - 1}      # (QAV: one more row for its head, below)


def _first_index(ids: torch.Tensor, token: int, what: str) -> torch.Tensor:
    """ids (B, O, S) -> (B, O): the first index of `token` in every row."""
    hit = ids == int(token)
    if not bool(hit.any(-1).all()):
        raise ValueError(f"option_rows: a {what} row does not hold token {token}")
    S = ids.shape[-1]
    pos = torch.arange(S).expand_as(ids)
    return torch.where(hit, pos, torch.full_like(pos, S)).min(-1).values


def option_rows(data: dict, F: int, q_token_id: int = 16492, v_token_id: int = 15167) -> dict:
    """The VAQ / QAV labels and frame indices of every answer option, from the (B, O, S) ids of the validation batch (host):
      label["vaq"] (B, O, S)  option c's ids with everything in front of p = first index of q_token_id + 2 set to 0
                              (reference dataloader/base_dataset.py:73-76);
      label["qav"] (B, O, S)  -1 everywhere except [p, p + min(F, S - p)) = 0.., p = first index of v_token_id + 2;
      video_index["qav"] (B, O, F) = p + arange(F);  prefix_index["vaq"], ["qav"] (B, O) = p.
    Each option is handled at its OWN positions. The reference's reader takes p from the gold option and applies it to every
    option (and model.py:336's scatter_add_ reaches only the first B of B * O rows): with the multiple-choice reader every option
    is a letter of equal length and both rules agree; where options differ in length the gold option's positions would leak the
    gold answer's length into the scores."""
    out = {"label": {}, "video_index": {}, "prefix_index": {}}
    if "vaq" in data["text_id"]:
        ids = torch.as_tensor(data["text_id"]["vaq"]).cpu()
        p = _first_index(ids, q_token_id, "vaq") + 2
        S = ids.shape[-1]
        out["label"]["vaq"] = torch.where(torch.arange(S) >= p[..., None], ids, torch.zeros_like(ids))
        out["prefix_index"]["vaq"] = p
    if "qav" in data["text_id"]:
        ids = torch.as_tensor(data["text_id"]["qav"]).cpu()
        p = _first_index(ids, v_token_id, "qav") + 2
        S = ids.shape[-1]
        f = torch.arange(S) - p[..., None]                                    # (B, O, S): the frame a position holds
        out["label"]["qav"] = torch.where((f >= 0) & (f < F), f, torch.full_like(f, -1))
        out["video_index"]["qav"] = p[..., None] + torch.arange(F)
        out["prefix_index"]["qav"] = p
    return out


def pick_rule(mean: dict, count: dict, weights, answer=None):
    """fvqa_flipped_pick on the host (numpy arrays in, numpy out): what the kernel is held to (tests) and the statement of the
    rule. mean / count: {task: (B, O)}; -> total (B, O) fp32, prediction (B,), prediction_t (3, B), gold_loss (B, 3) or None."""
    import numpy as np
    tasks = [t for t in TASKS if t in mean]
    B, O = mean[tasks[0]].shape
    total = np.zeros((B, O), np.float32)
    for t in tasks:                                                           # fp32 products, fp32 sums, in this order
        total = (total + (np.float32(weights[TASKS.index(t)]) * mean[t].astype(np.float32)).astype(np.float32)).astype(np.float32)

    def pick(v, ok):
        best = -1
        for c in range(O):
            if not ok[c]:
                continue
            if v[c] != v[c]:
                return c
            if best < 0 or v[c] < v[best]:
                best = c
        return max(best, 0)
    elig = np.all([count[t] > 0 for t in tasks], 0)
    pred = np.array([pick(total[n], elig[n]) for n in range(B)], np.int64)
    pred_t = np.full((3, B), -1, np.int64)
    for t in tasks:
        pred_t[TASKS.index(t)] = [pick(mean[t][n], count[t][n] > 0) for n in range(B)]
    gold = None
    if answer is not None:
        gold = np.full((B, 3), np.nan, np.float32)
        for t in tasks:
            for n in range(B):
                if 0 <= answer[n] < O:
                    gold[n, TASKS.index(t)] = mean[t][n, answer[n]]
    return total, pred, pred_t, gold


def _route(task: str, plan, route: Optional[str]) -> str:
    """`route` (forced: ValueError when the planner turned the batch down), else FVQA_SCORE, else the task's default; a batch the
    planner turns down goes dense whatever the environment asks."""
    if route is not None:
        if route not in score.ROUTES:
            raise ValueError(f"score_flipped: route {route!r}: expected one of {score.ROUTES}")
        if route == "shared" and not plan.shared:
            raise ValueError(f"score_flipped: the {task} stream of this batch cannot take the shared form ({plan.why_dense})")
        return route
    want = os.environ.get("FVQA_SCORE", "") or DEFAULT_ROUTE[task]
    if want not in score.ROUTES:
        raise ValueError(f"FVQA_SCORE={want!r}: expected one of {score.ROUTES}")
    return want if plan.shared else "dense"


def _dense(eng, data, task, ids_h, lab_h, rows, plan, events):
    """The B * O option sequences as one stream of `task` through the existing forward -> per-option sums (B, O)."""
    B, O, S = ids_h.shape
    qav = task == "qav"
    vs = [int(v) for v in data["video_start"].get(task, data["video_start"]["vqa"])]
    done = score._mark(events, f"{task} dense forward")
    tl, ar = score._dense_pass(eng, data, task, ids_h, lab_h, vs, rows["video_index"]["qav"] if qav else None)
    if qav:                                                # the QAV head leaves its losses at the dense rows
        n, c, t = plan.rows.unbind(1)
        out = score._pick(eng, ar.rowloss[: B * O * S], B * O * S, (n * O + c) * S + t, (n * O + c) * (S - 1) + t, B, O, S)[1]
    else:
        out = score._dense_pick(eng, tl, ar, plan, B, O, S)[1]
    done()
    return out


def _shared(eng, data, task, ids_h, lab_h, rows, plan, events):
    """The prompt pass once (option 0, no scored row; for QAV its own frame rows lie at or behind start, no prompt row sees them),
    then the suffix rows of every option -> per-option sums (B, O)."""
    dev = eng.device
    B, O, S = ids_h.shape
    qav = task == "qav"
    # QAV: the head scores row j against the label of row j + 1 and never its last row: one padding row behind the suffix
    T = plan.T + (1 if qav else 0)
    start, length = plan.start, plan.length
    live, pos, ids_suf = score._suffix_ids(plan, ids_h, T)
    slot = None
    if qav:
        f = pos - rows["prefix_index"]["qav"][..., None]
        slot = torch.where(live & (f >= 0) & (f < eng.F), f, torch.full_like(f, -1)).to(torch.int32)
    vs = [int(v) for v in data["video_start"].get(task, data["video_start"]["vqa"])]
    saved = score._prompt_pass(eng, data, task, ids_h, vs, events, f"{task} prompt pass",
                               rows["video_index"]["qav"][:, 0] if qav else None)
    done = score._mark(events, f"{task} suffix pass")
    mv = lambda x: x.to(dev, non_blocking=True)            # noqa: E731
    e = lambda *s, dtype=eng.dtype: torch.empty(*s, dtype=dtype, device=dev)  # noqa: E731
    start_d, len_d = score._suffix_lengths(eng, plan)
    R = B * O * T
    x = e(R, eng.D)
    vf_tok = eng._front_fwd(data, B)[1] if qav else None   # (the frame tokens once more: the forward keeps vf_raw only)
    ops.suffix_embed(mv(ids_suf.reshape(-1).contiguous()), None if slot is None else mv(slot.reshape(-1).contiguous()),
                     eng.pack.emb, vf_tok, len_d, x, B, O, T, eng.F)
    x = score._suffix_layers(eng, saved, start_d, len_d, x, B, O, T, S, wide=True)
    if not qav:
        out = score._scored_head(eng, x, plan, lab_h, B, O, T, S)[1]
    else:
        # ---- the QAV head on the suffix rows: B * O "sequences" of T rows, each option against its sample's frames
        f32 = torch.float32
        xn = e(R, eng.D)
        ops.rmsnorm_fwd(x, eng.pack.norm, xn, None, eng.eps, rows=R)
        # row j reads the label of row j + 1: the labels of positions start .. start + length (<= S - 1: a scored row is <= S - 2)
        has_lab = (torch.arange(T)[None, :] <= length[:, None])[:, None, :].expand(B, O, T)
        lab_suf = torch.where(has_lab, lab_h.gather(2, pos), torch.full_like(pos, -1))
        vf_rep = saved["vf_raw"].view(B, eng.F, eng.D).repeat_interleave(O, 0).contiguous()
        probs, rowloss = e(R * eng.F, dtype=f32), torch.zeros(R, dtype=f32, device=dev)
        loss_sum = torch.zeros(2, dtype=f32, device=dev)
        ops.qav_head_fwd(xn, vf_rep, mv(lab_suf.reshape(B * O, T).contiguous()), probs, rowloss, loss_sum, B * O, T, eng.D, eng.F,
                         eng.tau)
        n, c, t = plan.rows.unbind(1)
        out = score._pick(eng, rowloss, R, (n * O + c) * T + (t - start[n]), (n * O + c) * (T - 1) + (t - start[n]), B, O, T)[1]
    done()
    return out


def _task(eng, data, task, rows, route, events):
    """One of vaq, qav -> dict(sum, count, mean (B, O), route, plan). count is the number of scored rows by the labels (a row
    whose loss is exactly 0 counts, as in the training loss)."""
    ids_h = torch.as_tensor(data["text_id"][task]).cpu()
    lab_h = rows["label"][task]
    if ids_h.dim() != 3:
        raise ValueError(f"score_flipped: text_id[{task!r}] must be (B, n_options, S)")
    B, O, S = ids_h.shape
    if int(ids_h.min()) < 0 or int(ids_h.max()) >= eng.V:
        raise ValueError(f"text_id[{task}] outside [0, {eng.V})")
    qav = task == "qav"
    if qav and int(rows["video_index"]["qav"].max()) >= S:
        raise ValueError("score_flipped: video_index[qav] outside the sequence (an option leaves no room for the frames)")
    vs = None if qav else [int(v) for v in data["video_start"][task]]
    plan = score.plan_options(ids_h, lab_h, None, vs, eng.F, suffix_max=SUFFIX_LIMIT[task], frames_in_suffix=qav, qav=qav)
    r = _route(task, plan, route)
    s = (_shared if r == "shared" else _dense)(eng, data, task, ids_h, lab_h, rows, plan, events)
    ok = (lab_h[:, :, 1:] >= 0) if qav else (lab_h[:, :, 1:] > 0)
    count = ok.sum(-1).to(eng.device)
    return dict(sum=s, count=count, mean=s / count, route=r, plan=plan)


@torch.no_grad()
def score_flipped(eng, data: dict, tasks=TASKS, weights=(1.0, 1.0, 1.0), route: Optional[str] = None, answer=None,
                  events: Optional[list] = None, q_token_id: int = 16492, v_token_id: int = 15167) -> dict:
    """-> dict with, per requested task t of (vqa, vaq, qav): mean_t, sum_t, count_t (B, O) and prediction_t (B,); total (B, O)
    fp32 = sum_t weights[t] * mean_t in the order vqa, vaq, qav; prediction (B,) int64: the argmin of total over the options every
    requested task scored (include/fvqa.h fvqa_flipped_pick: ties to the lowest index, the first NaN wins, 0 when none is
    eligible); gold_loss (B, 3) when `answer` (B,) is given: each task's mean at the gold option (NaN for a task not requested) —
    the validation-time vqa / vaq / qav losses; route and plan: {task: ...}. All tensors on the device.
    weights: (w_vqa, w_vaq, w_qav); the default follows the training loss, which sums the three. route: None — per task FVQA_SCORE,
    else DEFAULT_ROUTE, dense for what the planner turns down —, or "shared" / "dense" for every task (ValueError where the planner
    turned the shared form down). The vqa entries are score_options' own, bit for bit. events: as score_options."""
    tasks = tuple(tasks)
    if not tasks or any(t not in TASKS for t in tasks) or len(set(tasks)) != len(tasks):
        raise ValueError(f"score_flipped: tasks {tasks!r}: a non-empty selection of {TASKS}")
    tasks = tuple(t for t in TASKS if t in tasks)
    if len(weights) != 3:
        raise ValueError("score_flipped: three weights (vqa, vaq, qav)")
    for t in tasks:
        if t not in data["text_id"]:
            raise ValueError(f"score_flipped: the batch carries no text_id[{t!r}]")
    out = {"route": {}, "plan": {}}
    res = {}
    if "vqa" in tasks:
        r = score.score_options(eng, data, route=route, events=events)
        res["vqa"] = {k: r[k] for k in ("sum", "count", "mean", "route", "plan")}
        out["individual_losses"] = r["individual_losses"]
    if set(tasks) - {"vqa"}:
        rows = option_rows(data, eng.F, q_token_id, v_token_id)
        for t in tasks[1 if "vqa" in tasks else 0:]:
            res[t] = _task(eng, data, t, rows, route, events)
    for t in tasks:
        for k in ("sum", "count", "mean"):
            out[f"{k}_{t}"] = res[t][k]
        out["route"][t], out["plan"][t] = res[t]["route"], res[t]["plan"]
    mean = {t: res[t]["mean"].contiguous() for t in tasks}
    count = {t: res[t]["count"].contiguous() for t in tasks}
    ans = None if answer is None else torch.as_tensor(answer).to(eng.device, dtype=torch.int64).contiguous()
    total, pred, pred_t, gold = ops.flipped_pick(mean, count, weights, ans)
    out.update(total=total, prediction=pred)
    for t in tasks:
        out[f"prediction_{t}"] = pred_t[TASKS.index(t)]
    if gold is not None:
        out["gold_loss"] = gold
    return out
