"""`engine.train_one_epoch` with the reference's signature and return value (reference
engine.py:10-56): per-iteration LR schedule, forward, sum of the three flipped losses, finite
check, gradient accumulation through the loss scaler, meters.

`--log_video_mass EVERY` (0: off) adds a `video_mass` meter: on every EVERY-th iteration, between the forward and the backward,
the weight the text softmax of the vqa stream's scored rows puts on the frame keys is read off the step's arena
(fvqa/attribution.py: training_video_mass — what a trained gate2 lets the answer rows see of the clip). It reads the arena only and
rides in the losses' transfer: losses, gradients and the optimizer step are those of the run without the flag, bit for bit.

Host-side differences that do not change results: the three loss values come back in ONE
device->host transfer per iteration instead of four `.item()` calls + a full device sync; that
transfer is WAITED FOR only after the backward (and, at an accumulation boundary, the optimizer
step) of the iteration has been launched, so the device never idles while the host reads the
loss (reading first, as the reference does, leaves the GPU idle from the end of the forward until
the host has issued the first backward kernel: 0.5-1 ms of a 29 ms step). A non-finite loss still
prints the reference's message and exits with status 1 before anything else happens on the host;
the one difference is that the backward / optimizer step of THAT iteration has already been queued
on the device when the process exits (a non-finite gradient is skipped by the fused optimizer; a
finite one — e.g. the other two losses when only one CE had no scored token — is applied), which
nothing observes: the reference's train.py does not catch the exit and saves nothing after it. The logging period is clamped to >= 1 (the reference crashes on loaders shorter
than 4 batches).
"""
import math
import sys
from typing import Iterable

import torch

import util.lr_sched as lr_sched
import util.misc as misc


def train_one_epoch(model: torch.nn.Module, data_loader: Iterable, optimizer: torch.optim.Optimizer, epoch: int,
                    loss_scaler, args=None):
    model.train(True)
    log = misc.MetricLogger(delimiter="  ")
    log.add_meter("lr", misc.SmoothedValue(window_size=1, fmt="{value:.6f}"))
    n_iter = len(data_loader)
    accum = args.accum_iter
    optimizer.zero_grad()
    host_vals, copied = None, None
    watch = int(getattr(args, "log_video_mass", 0) or 0)      # --log_video_mass EVERY: a video_mass meter (fvqa/attribution.py)

    for it, data in enumerate(log.log_every(data_loader, n_iter // 4, f"Epoch: [{epoch}]")):
        boundary_start = it % accum == 0
        boundary_end = (it + 1) % accum == 0
        if boundary_start:
            lr_sched.adjust_learning_rate(optimizer, it / n_iter + epoch, args)

        vqa_loss, vaq_loss, qav_loss = model(data)
        loss = vqa_loss + vaq_loss + qav_loss
        mass_dev = None
        if watch and (it + 1) % watch == 0:                   # between the forward and the backward: the arena is read, not written
            eng = getattr(getattr(model, "module", model), "_engine", None)
            if eng is not None and eng.saved is not None:
                from fvqa import attribution
                with torch.no_grad():
                    mass_dev = attribution.training_video_mass(eng, data["label"]["vqa"])
        # the three losses and — riding in the same transfer, at no cost of its own — the found-inf word the loss scaler
        # left on the device in the PREVIOUS iteration (2 = the GEMM error word was set: include/fvqa.h)
        found_dev = getattr(loss_scaler, "_found", None)
        prev_found = found_dev.reshape(()).float() if torch.is_tensor(found_dev) and found_dev.device == vqa_loss.device \
            else torch.zeros((), dtype=torch.float32, device=vqa_loss.device)
        vals_dev = torch.stack([vqa_loss.reshape(()).float(), vaq_loss.reshape(()).float(),
                                qav_loss.reshape(()).float(), prev_found]
                               + ([mass_dev.reshape(()).float()] if mass_dev is not None else []))      # (the meter rides along)
        if vals_dev.is_cuda:                                  # one asynchronous D2H copy into pinned memory
            if host_vals is None:
                host_vals, copied = torch.empty(5, dtype=torch.float32, pin_memory=True), torch.cuda.Event()
            host_vals[:vals_dev.numel()].copy_(vals_dev, non_blocking=True)
            copied.record()

        loss_scaler(loss / accum, optimizer, parameters=model.parameters(), update_grad=boundary_end)

        if vals_dev.is_cuda:
            copied.synchronize()                              # the forward has finished; the backward is queued
            vals = host_vals.tolist()
            if vals[3] == 2.0:                                # (sticky: the error word stays set until someone clears it)
                raise RuntimeError("fvqa: a split-K exchange of the persistent GEMM timed out (found_inf = 2): the "
                                   "previous optimizer step was skipped and the results of its launches are invalid")
        else:
            vals = vals_dev.tolist()
        loss_value = vals[0] + vals[1] + vals[2]
        if not math.isfinite(loss_value):
            print("Loss is {}, stopping training".format(loss_value))
            sys.exit(1)
        if boundary_end:
            optimizer.zero_grad()

        log.update(loss=loss_value, vqa_loss=vals[0], vaq_loss=vals[1], qav_loss=vals[2])
        if mass_dev is not None:
            log.update(video_mass=vals[4])
        log.update(lr=optimizer.param_groups[0]["lr"])
        if getattr(args, "debug", False):
            break

    # The LAST iteration's error state. found_inf = 2 is the all-reduced error lane (fvqa/parallel.py: every rank sees it when
    # ANY rank's split-K exchange timed out), so every rank stops here together; reading only the local error word would raise
    # on the faulty rank alone and leave the healthy ones waiting in the meter all-reduce below (round-4 advisor finding).
    found_dev = getattr(loss_scaler, "_found", None)
    if torch.is_tensor(found_dev) and float(found_dev.reshape(-1)[0].item()) == 2.0:
        raise RuntimeError("fvqa: a split-K exchange of the persistent GEMM timed out on some rank (found_inf = 2): the last "
                           "optimizer step was skipped on every rank and the results of its launches are invalid")
    eng = getattr(getattr(model, "module", model), "_engine", None)
    if eng is not None:
        eng.check_gemm_error()                                # this rank's own word (include/fvqa.h: error word)
    log.synchronize_between_processes()
    print("Averaged stats:", log)
    return {k: m.global_avg for k, m in log.meters.items()}


def _val_flipped(owner, data, log, optimizer, args):
    """One multiple-choice batch under --val_flipped: the four predictions and the gold option's losses in ONE host read."""
    if not hasattr(owner, "score_flipped"):
        raise NotImplementedError("--val_flipped needs a model with score_flipped (llama/model.py)")
    answer = data["answer"]
    bsz = answer.shape[0]
    w = getattr(args, "val_flipped_weights", None) or (1.0, 1.0)
    with torch.no_grad():
        r = owner.score_flipped(data, weights=(1.0, float(w[0]), float(w[1])), answer=answer)
    preds = torch.stack([r["prediction"], r["prediction_vqa"], r["prediction_vaq"], r["prediction_qav"]])      # (4, B)
    packed = torch.cat([preds.reshape(-1).to(torch.float64), r["gold_loss"].to(torch.float64).mean(0)]).cpu()
    pred_h = packed[: 4 * bsz].to(torch.int64).view(4, bsz)
    hit = answer.cpu() == pred_h
    misc.log_qtype(data, hit[0], log, args)
    log.update(lr=optimizer.param_groups[0]["lr"])
    log.update(n=bsz, acc=hit[0].sum().item() / bsz, acc_vqa=hit[1].sum().item() / bsz, acc_vaq=hit[2].sum().item() / bsz,
               acc_qav=hit[3].sum().item() / bsz, vaq_loss=float(packed[-2]), qav_loss=float(packed[-1]))


def vocab_gold(data, answers) -> list:
    """Per sample the index of its gold answer's text in `answers` (the --answer_vocab list), -1 if it is not a member. The gold
    text is the option the batch's `answer` names (MusicAVQA: its one free-text option)."""
    where = {}
    for i, a in enumerate(answers):
        where.setdefault(str(a).strip(), i)
    return [where.get(str(t["options"][int(g)]).strip(), -1) for t, g in zip(data["text"], data["answer"].tolist())]


def _val_vocab(owner, data, log, optimizer, args):
    """One generation batch under --val_vocab: the prediction, the top-5 hit, the gold answer's -log posterior and whether it is
    in the vocabulary, in ONE host read."""
    if not hasattr(owner, "score_vocab") or not hasattr(owner, "answer_vocab"):
        raise NotImplementedError("--val_vocab needs a model with score_vocab and answer_vocab (llama/model.py)")
    bsz = data["answer"].shape[0]
    answers, cons = owner.answer_vocab()
    contrast = getattr(args, "contrast", None)
    kw = {"contrast": contrast, "contrast_alpha": float(getattr(args, "contrast_alpha", 1.0))} if contrast else {}
    with torch.no_grad():
        r = owner.score_vocab(data, cons, top=min(5, len(answers)), **kw)
    gold = torch.as_tensor(vocab_gold(data, answers), dtype=torch.int64).to(r["prediction"].device, non_blocking=True)
    inside = gold >= 0
    nll = -r["log_posterior"].gather(1, gold.clamp(min=0).view(-1, 1)).view(-1)
    f = lambda t: t.to(torch.float64)                      # noqa: E731
    packed = torch.stack([f((r["prediction"] == gold) & inside), f((r["ranking"] == gold.view(-1, 1)).any(1) & inside), f(inside),
                          torch.where(inside, f(nll), torch.zeros_like(f(nll)))]).cpu()
    hit, n_in = packed[0].bool(), int(packed[2].sum())
    misc.log_qtype(data, hit, log, args)
    log.update(lr=optimizer.param_groups[0]["lr"])
    log.update(n=bsz, acc=float(packed[0].sum()) / bsz, acc_top5=float(packed[1].sum()) / bsz, gold_in_vocab=n_in / bsz)
    if n_in:
        log.update(n=n_in, gold_nll=float(packed[3].sum()) / n_in)


def val_one_epoch(model: torch.nn.Module, data_loader: Iterable, optimizer: torch.optim.Optimizer, epoch: int,
                  args=None):
    """Validation with the reference's signature and return value (reference engine.py:59-145), both modes.
    `--is_generation_task` (the mode every run script of the reference uses): greedy answer generation, nearest-choice matching.
    Otherwise the original multiple-choice protocol (engine.py:86-93,122-129): every option is scored by its mean
    cross-entropy over the answer tokens and the lowest wins — `model.score_options(data)` (llama/model.py; a model without it
    is rejected) returns the reference's `individual_losses` and leaves count / prediction, reduced on the device, in
    `last_scoring`: one host read per batch. Accuracy overall and per question type either way.
    `--contrast blind` (multiple choice): the prediction is the contrastive one (fvqa/score.py) and `acc_blind` / `acc_plain` —
    the accuracy of the blind twin's and of the plain prediction — are logged from the same single host read.
    `--val_frame_attention` (multiple choice): a `video_mass` meter — the weight the text softmax of the predicted option's scored
    rows puts on the frame keys (fvqa/attribution.py: summarize_options), mean over the samples, reduced on the device and read
    with the prediction.
    `--val_flipped [--val_flipped_weights W_VAQ W_QAV]` (multiple choice): the options are scored by all three flipped tasks
    (`model.score_flipped`, fvqa/flipped.py) and the prediction is the argmin of their weighted sum; `acc`, `acc_vqa`, `acc_vaq`,
    `acc_qav` and `vaq_loss` / `qav_loss` — each task's mean loss at the gold option — come from the batch's one host read.
    `--gen_stream SLOTS` (generation task): the loader's batches are materialised and decoded through ONE stream of SLOTS rows
    with in-flight batching (`model.inference_stream`, fvqa/stream.py) before the per-batch body below runs on each batch's rows;
    without the flag every call launches what it did.
    `--val_vocab` (generation task, with `--answer_vocab FILE`): the batch is classified over the answer vocabulary
    (`model.score_vocab`, fvqa/vocab.py: every member's exact log-probability in one pass); `acc`, `acc_top5`, `gold_nll` — the
    gold answer's -log posterior, over the samples whose gold answer is in the vocabulary — and `gold_in_vocab` come from the
    batch's one host read. Nothing is decoded.
    `--gen_frame_attention` (generation task, through `generate`): a `video_mass` meter — the weight the answer rows' text softmax
    puts on the frame keys (fvqa/attribution.py) — and `frame_share` in every entry of the extracted-answers file.
    `--gen_vote N` (generation task): every row decodes N samples and the vote's winner is the answer (llama/model.py); a
    `vote_share` meter — the winner's share of the samples, mean over the batch — is read with the hits in the batch's one host read."""
    gen = bool(getattr(args, "is_generation_task", False))
    owner = None
    if not gen:
        owner = next((m for m in (model, getattr(model, "module", None)) if hasattr(m, "score_options")), None)
        if owner is None:
            raise NotImplementedError("validation without --is_generation_task needs a model with score_options "
                                      "(reference engine.py:86-93)")
    model.eval()
    log = misc.MetricLogger(delimiter="  ")
    log.add_meter("lr", misc.SmoothedValue(window_size=1, fmt="{value:.6f}"))
    streamed = None
    n_slots = int(getattr(args, "gen_stream", 0) or 0) if gen else 0
    if n_slots >= 1:
        owner = next((m for m in (model, getattr(model, "module", None)) if hasattr(m, "inference_stream")), None)
        if owner is None:
            raise NotImplementedError("--gen_stream needs a model with inference_stream (llama/model.py)")
        data_loader = list(data_loader)[: 1 if getattr(args, "debug", False) else None]
        with torch.no_grad():
            streamed = iter(owner.inference_stream(data_loader, n_slots, getattr(args, "gen_stream_admit", None)))
    for data in log.log_every(data_loader, max(1, len(data_loader) // 4), f"Epoch: [{epoch}]"):
        answer = data["answer"]
        bsz = answer.shape[0]
        if gen and getattr(args, "val_vocab", False):
            owner = owner or next((m for m in (model, getattr(model, "module", None)) if hasattr(m, "score_vocab")), None)
            _val_vocab(owner, data, log, optimizer, args)
            if getattr(args, "debug", False):
                break
            continue
        if not gen and getattr(args, "val_flipped", False):
            _val_flipped(owner, data, log, optimizer, args)
            if getattr(args, "debug", False):
                break
            continue
        if not gen:
            contrast = getattr(args, "contrast", None)       # --contrast blind: the prediction discounts the blind twin's means
            watch = bool(getattr(args, "val_frame_attention", False))
            kw = {"contrast": contrast, "contrast_alpha": float(getattr(args, "contrast_alpha", 1.0))} if contrast else {}
            if watch:                                        # (with --contrast: score_options' ValueError, as the parser's)
                kw["frame_attention"] = True
            with torch.no_grad():
                individual_losses = owner.score_options(data, **kw)
            last = getattr(owner, "last_scoring", None)
            if last is not None:
                prediction = last["prediction"]
            else:                                            # (a model that only returns the losses: engine.py:88-93)
                count = (individual_losses != 0).sum(-1)
                prediction = (individual_losses.sum(-1) / count).argmin(-1)
            extra = None
            if contrast and last is not None and "prediction_blind" in last:
                prediction = torch.stack([prediction, last["prediction_blind"], last["prediction_plain"]])
                extra = True
            mass_h = None
            if watch and last is not None and "video_mass" in last:      # the meter rides behind the predictions
                picked = last["video_mass"].gather(1, prediction.view(-1, 1)).mean()
                packed = torch.cat([prediction.to(torch.float64), picked.to(torch.float64).view(1)]).cpu()
                pred_h, mass_h = packed[:-1].to(torch.int64), float(packed[-1])
            else:
                pred_h = prediction.cpu()                    # the batch's one device->host read
            hit = answer.cpu() == (pred_h[0] if extra else pred_h)
            misc.log_qtype(data, hit, log, args)
            log.update(lr=optimizer.param_groups[0]["lr"])
            log.update(n=bsz, acc=hit.sum().item() / bsz)
            if mass_h is not None:
                log.update(n=bsz, video_mass=mass_h)
            if extra:                                        # what the model answers without looking, and without the contrast
                log.update(n=bsz, acc_blind=(answer.cpu() == pred_h[1]).sum().item() / bsz,
                           acc_plain=(answer.cpu() == pred_h[2]).sum().item() / bsz)
            if getattr(args, "debug", False):
                break
            continue
        with torch.no_grad():
            best, extracted = next(streamed) if streamed is not None else model(data, inference=True)
        if getattr(args, "gen_frame_attention", False) and extracted and "video_mass" in extracted[0]:
            log.update(n=bsz, video_mass=sum(e["video_mass"] for e in extracted) / len(extracted))
        if getattr(args, "output_dir", None):
            import os
            os.makedirs(os.path.join(args.output_dir, "extracted_answers"), exist_ok=True)
            misc.save_result(extracted, os.path.join(args.output_dir, "extracted_answers"),
                             "extracted_answers_epoch%d" % epoch)
        if getattr(args, "dataset", None) == "musicavqa":
            # one free-text option: a hit is a generated answer that starts with it (reference engine.py:100-116)
            hit = torch.tensor([g["generated_answer"].startswith(t["options"][0]) for t, g in zip(data["text"], extracted)],
                               device=best.device)
        else:
            hit = answer.to(best.device) == best
        misc.log_qtype(data, hit, log, args)
        log.update(lr=optimizer.param_groups[0]["lr"])
        share = None
        if int(getattr(args, "gen_vote", 0) or 0) > 1:      # --gen_vote N: the winner's share rides behind the hits
            last = next((m.last_generation for m in (model, getattr(model, "module", None))
                         if isinstance(getattr(m, "last_generation", None), dict)), {})
            share = last.get("vote_share")
        if share is not None:
            packed = torch.stack([hit.sum().to(torch.float64), share.to(hit.device).to(torch.float64).mean()]).cpu()
            log.update(n=bsz, acc=float(packed[0]) / bsz, vote_share=float(packed[1]))
        else:
            log.update(n=bsz, acc=hit.sum().item() / bsz)
        if getattr(args, "debug", False):
            break
    log.synchronize_between_processes()
    print("Averaged stats:", log)
    return {k: m.global_avg for k, m in log.meters.items()}
