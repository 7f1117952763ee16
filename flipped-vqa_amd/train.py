"""Training entry point with the reference's CLI (reference train.py:24-176): same flags,
`get_args_parser()`, `main(args)`, `validate_args(args)`; launch with
`torchrun --nproc_per_node N train.py ...` (one process per MI355X, RCCL over xGMI).

Extra flags (all optional): --dtype {bf16,fp32}, --random_init, --synthetic, --synthetic_batches N
select closed-form weights / batches so the path runs without LLaMA assets or datasets.
"""
import argparse
import datetime
import json
import os
import time
from pathlib import Path

import numpy as np
import torch

import util.misc as misc
from engine import train_one_epoch
from fvqa import synth
from fvqa.batch_producer import DeviceBatchProducer
from fvqa.optim import FusedAdamW, param_groups_weight_decay
from fvqa.parallel import DataParallel
from llama_vqa import LLaMA_VQA
from util.misc import NativeScalerWithGradNormCount as NativeScaler

# (flag, kwargs) — the reference's flag set, names and defaults (train.py:26-73)
_FLAGS = [
    ("--batch_size", dict(default=64, type=int, help="batch size per GPU (effective = batch_size * accum_iter * #gpus)")),
    ("--epochs", dict(default=400, type=int)),
    ("--accum_iter", dict(default=1, type=int, help="gradient accumulation iterations")),
    ("--llama_model_path", dict(default="./pretrained/llama/", type=str)),
    ("--model", dict(default="llama7B_adapter", type=str, metavar="MODEL")),
    ("--adapter_layer", dict(type=int, default=32, metavar="LENGTH")),
    ("--adapter_len", dict(type=int, default=10, metavar="LENGTH")),
    ("--max_seq_len", dict(type=int, default=512, metavar="LENGTH")),
    ("--max_feats", dict(type=int, default=10, metavar="LENGTH")),
    ("--weight_decay", dict(type=float, default=0.05)),
    ("--lr", dict(type=float, default=None, metavar="LR", help="absolute learning rate")),
    ("--blr", dict(type=float, default=1e-3, metavar="LR", help="base lr: lr = blr * total_batch / 256")),
    ("--min_lr", dict(type=float, default=0.0, metavar="LR")),
    ("--warmup_epochs", dict(type=int, default=40, metavar="N")),
    ("--dataset", dict(default="nextqa", type=str)),
    ("--output_dir", dict(default="./output_dir")),
    ("--device", dict(default="cuda")),
    ("--seed", dict(default=0, type=int)),
    ("--resume", dict(default="")),
    ("--start_epoch", dict(default=0, type=int, metavar="N")),
    ("--num_workers", dict(default=2, type=int)),
    ("--pin_mem", dict(action="store_true")),
    ("--no_pin_mem", dict(action="store_false", dest="pin_mem")),
    ("--world_size", dict(default=1, type=int)),
    ("--local_rank", dict(default=-1, type=int)),
    ("--dist_on_itp", dict(action="store_true")),
    ("--dist_url", dict(default="env://")),
    ("--vaq", dict(action="store_true", help="vaq loss")),
    ("--qav", dict(action="store_true", help="qav loss")),
    ("--bias", dict(type=float, default=3.0, help="attention bias")),
    ("--tau", dict(type=float, default=100.0)),
    ("--sub", dict(action="store_true")),
    ("--is_generation_task", dict(action="store_true")),
    ("--debug", dict(action="store_true")),
    ("--jobid", dict(type=int)),
    ("--audio", dict(action="store_true")),
    ("--audio_only", dict(action="store_true")),
    ("--audio_merge", dict(type=str, choices=["sum", "concat", "attention", "none"], default="none")),
    # MI355X build additions
    ("--train_audio", dict(action="store_true", help="train (and checkpoint) audio_proj and the audio-video cross-attention, "
                                                     "which the reference's freeze filter leaves at their random initialisation")),
    ("--train_norm", dict(action="store_true", help="train (and checkpoint) the RMSNorm weights of the layers the adapter walks and "
                                                    "the final norm, which the reference's freeze filter keeps frozen: fp32 masters "
                                                    "beside the other trainables, no weight decay (they are 1-D)")),
    ("--gen_stop_eos", dict(action="store_true", help="generation-task validation decodes through fvqa.generate.generate: each "
                                                      "sample stops at its EOS and the batch stops when every sample has")),
    ("--num_beams", dict(type=int, default=1, help="generation-task validation: beam search with N slots per sample "
                                                   "(fvqa.generate.beam_search; 1: the decode chosen by --gen_stop_eos)")),
    ("--gen_constrain", dict(type=str, choices=["options", "vocab"], default=None,
                             help="generation-task validation decodes under a set of allowed answers (fvqa.generate.generate("
                                  "constraints=...)): 'options' — the sample's own answer options, the prediction is the option "
                                  "generated; 'vocab' — the shared answers of --answer_vocab. --num_beams applies as before")),
    ("--answer_vocab", dict(type=str, default=None, help="a file with one allowed answer per line (needed by --gen_constrain vocab)")),
    ("--contrast", dict(type=str, choices=["blind"], default=None,
                        help="validation only: contrastive decoding / scoring against the video-blind twin of every prompt (the "
                             "same text, zero features): generation-task validation decodes through fvqa.generate.generate("
                             "contrast='blind'), alone or with --gen_constrain; multiple-choice validation predicts by "
                             "mean + alpha * (mean - mean_blind) and logs acc_blind / acc_plain. Not with --num_beams > 1")),
    ("--contrast_alpha", dict(type=float, default=1.0, help="--contrast: the weight of the difference to the twin (>= 0)")),
    ("--contrast_beta", dict(type=float, default=0.1, help="--contrast: a token is plausible iff its probability with the clip "
                                                           "is at least beta times the largest (0 .. 1; generation only)")),
    ("--lookahead", dict(type=int, default=0,
                         help="generation-task validation: draft-and-verify greedy decoding with up to T rows per pass "
                              "(fvqa.generate.generate(lookahead=T)): greedy's tokens, each row ended by its EOS, several tokens "
                              "per pass where the prompt-lookup draft is right. 0, 1: off. Not with --num_beams > 1, "
                              "--gen_constrain or --contrast")),
    ("--lookup_ngram", dict(type=int, default=2, help="--lookahead: the longest n-gram of committed tokens the prompt lookup "
                                                      "matches (1 .. 4)")),
    ("--gen_draft", dict(type=str, choices=["options", "vocab"], default=None,
                         help="generation-task validation with --lookahead R (2 .. 64): the drafts are a trie of likely answers, "
                              "verified in one tree pass (fvqa.generate.generate(lookahead=R, draft_answers=...)): 'options' — each "
                              "sample's own answer options as the prompt asks for them; 'vocab' — the answers of --answer_vocab. "
                              "A draft, not a rule: the protocol, the tokens and the answers file are the plain run's, in fewer "
                              "passes where the model answers with a drafted answer. Not with --num_beams > 1, --gen_constrain, "
                              "--contrast, --gen_jump_forward, --gen_stream, --val_vocab or --gen_frame_attention")),
    ("--gen_jump_forward", dict(type=int, default=0,
                                help="--gen_constrain: jump-forward decoding with up to T rows per pass (fvqa.generate.generate("
                                     "constraints=..., jump_forward=T)): the tokens the trie of allowed answers fixes are committed "
                                     "without a pass of their own — the same answers in fewer passes. 0, 1: off. Not with "
                                     "--num_beams > 1, --contrast or --lookahead > 1")),
    ("--gen_stream", dict(type=int, default=0, metavar="SLOTS",
                          help="generation-task validation with in-flight batching (fvqa.stream.generate_stream): the split's "
                               "questions go through one decode batch of SLOTS rows in which a finished row hands its slot to "
                               "the next question; greedy with EOS stop (--gen_stop_eos's answers), or --gen_constrain. 0: off. "
                               "Not with --num_beams > 1, --contrast, --lookahead > 1 or --gen_jump_forward > 1")),
    ("--gen_stream_admit", dict(type=int, default=None, metavar="M",
                                help="--gen_stream (answer.py: --slots / --admit): questions admitted per prefill, 1 .. SLOTS "
                                     "(default: SLOTS // 2)")),
    ("--gen_frame_attention", dict(action="store_true",
                                   help="generation-task validation through fvqa.generate.generate(frame_attention=True) (needs "
                                        "--gen_stop_eos or --gen_constrain): where the answer rows looked — a video_mass meter (the "
                                        "text softmax's weight on the frame keys, mean over tokens, layers and heads) and "
                                        "frame_share, the weight per frame, in every entry of the extracted-answers file. Not with "
                                        "--num_beams > 1, --contrast, --lookahead > 1, --gen_jump_forward > 1 or --gen_stream")),
    ("--gen_vote", dict(type=int, default=0, metavar="N",
                        help="generation-task validation by self-consistency (fvqa.generate.generate(num_return_sequences=N, "
                             "vote=True, seed=--seed)): every row decodes N samples (2 .. 64) from one prefill, the samples with "
                             "equal tokens form a group and the largest group's answer goes through the unchanged answer matching "
                             "(with --gen_constrain options the winner's choice is the prediction); logs a vote_share meter, the "
                             "winner's share of the samples. 0: off. Not with --num_beams > 1, --lookahead > 1, "
                             "--gen_jump_forward > 1, --gen_stream, --val_vocab or --gen_frame_attention")),
    ("--gen_vote_temperature", dict(type=float, default=1.0, help="--gen_vote: the samples' temperature (> 0)")),
    ("--gen_vote_top_p", dict(type=float, default=1.0, help="--gen_vote: the samples' nucleus bound, in (0, 1]")),
    ("--gen_no_repeat_ngram", dict(type=int, default=0, metavar="N",
                                   help="generation-task validation through fvqa.generate.generate(no_repeat_ngram_size=N) (needs "
                                        "--gen_stop_eos or --gen_vote): no N-gram occurs twice among a row's generated tokens; the "
                                        "prompt is not scanned. 0: off. Not with --gen_constrain, --contrast or what --gen_vote refuses")),
    ("--gen_min_new_tokens", dict(type=int, default=0, metavar="M",
                                  help="generation-task validation through fvqa.generate.generate(min_new_tokens=M) (needs "
                                       "--gen_stop_eos or --gen_vote): the EOS is banned before a row's M-th token. 0: off. Not "
                                       "with --gen_constrain, --contrast or what --gen_vote refuses")),
    ("--log_video_mass", dict(type=int, default=0, metavar="EVERY",
                              help="training: on every EVERY-th iteration log a video_mass meter — the weight the text softmax "
                                   "of the vqa stream's scored rows puts on the frame keys, mean over rows, layers and heads, "
                                   "read off the step's arena between the forward and the backward (the step itself is "
                                   "unchanged). 0: off")),
    ("--val_frame_attention", dict(action="store_true",
                                   help="multiple-choice validation (no --is_generation_task) through "
                                        "score_options(frame_attention=True): a video_mass meter — the weight the text softmax of "
                                        "the predicted option's scored rows puts on the frame keys, mean over rows, layers and "
                                        "heads (fvqa.attribution.summarize_options). Not with --contrast")),
    ("--val_flipped", dict(action="store_true",
                           help="multiple-choice validation (no --is_generation_task) by all three flipped tasks "
                                "(fvqa.flipped.score_flipped): the prediction is the argmin of vqa + W_VAQ * vaq + W_QAV * qav mean "
                                "losses per option; logs acc, acc_vqa, acc_vaq, acc_qav and the vaq / qav losses at the gold "
                                "option. Not with --contrast or --val_frame_attention")),
    ("--val_flipped_weights", dict(type=float, nargs=2, default=None, metavar=("W_VAQ", "W_QAV"),
                                   help="--val_flipped: the weights of the vaq and qav means (default 1 1, as the training loss "
                                        "sums the three)")),
    ("--val_vocab", dict(action="store_true",
                         help="generation-task validation as a classifier over --answer_vocab (fvqa.vocab.score_vocab): every "
                              "allowed answer's exact log-probability in one pass over their trie; the prediction is the member "
                              "with the highest mean; logs acc, acc_top5, gold_nll (-log posterior of the gold answer, over the "
                              "samples whose gold answer is in the vocabulary) and gold_in_vocab. Needs --answer_vocab and "
                              "--is_generation_task. Not with --num_beams > 1, --lookahead, --gen_jump_forward, --gen_stream or "
                              "--gen_frame_attention")),
    ("--val_batch_size", dict(type=int, default=None, help="batch size of every split but train (default: --batch_size)")),
    ("--dtype", dict(type=str, choices=["bf16", "fp32"], default="bf16", help="storage dtype of frozen weights/activations")),
    ("--random_init", dict(action="store_true", help="closed-form weights instead of a checkpoint")),
    ("--synthetic", dict(action="store_true", help="synthetic tokenizer constants + synthetic batches")),
    ("--synthetic_batches", dict(type=int, default=8, help="batches per epoch with --synthetic")),
]


def _check_pick_rules(self, a, la):
    """(self: the parser.) The pick rules and the vote, under train.py's names (gen_*) and answer.py's: what fvqa.generate.generate refuses."""
    beams = int(getattr(a, "num_beams", 1) or 1) > 1
    jump = int(getattr(a, "gen_jump_forward", 0) or 0) > 1 or int(getattr(a, "jump_forward", 0) or 0) > 1
    stream = int(getattr(a, "gen_stream", 0) or 0) >= 1 or int(getattr(a, "slots", 0) or 0) >= 1
    min_p = getattr(a, "min_p", 0.0)
    ngram = getattr(a, "gen_no_repeat_ngram", 0) or getattr(a, "no_repeat_ngram", 0)
    m_new = getattr(a, "gen_min_new_tokens", 0) or getattr(a, "min_new_tokens", 0)
    if not 0 <= min_p < 1:
        self.error("0 <= --min_p < 1 (0: off)")
    if ngram < 0 or m_new < 0:
        self.error("the n-gram size and the minimum length are >= 0 (0: off)")
    if hasattr(a, "max_new_tokens") and m_new > a.max_new_tokens:
        self.error("--min_new_tokens <= --max_new_tokens")
    if min_p > 0 and not float(getattr(a, "temperature", 0.0) or 0.0) > 0:
        self.error("--min_p cuts a sampled distribution: it needs --temperature > 0")
    vote_n = int(getattr(a, "gen_vote", 0) or 0)
    if min_p != 0 or ngram != 0 or m_new != 0:
        if (beams or la > 1 or jump or stream or getattr(a, "gen_constrain", None) or getattr(a, "constrain", False)
                or getattr(a, "contrast", None) or getattr(a, "val_vocab", False) or int(getattr(a, "rank", 0) or 0)
                or (getattr(a, "answer_vocab", None) and hasattr(a, "min_p"))):
            self.error("the pick rules (min-p, n-gram blocking, minimum length) run in the plain token loop: not with "
                       "--num_beams > 1, constrained or contrastive decoding, --lookahead > 1, drafts, jump-forward, a stream "
                       "or a vocabulary scoring")
        if hasattr(a, "gen_no_repeat_ngram") and not hasattr(a, "min_p") and not (getattr(a, "gen_stop_eos", False) or vote_n):
            self.error("--gen_no_repeat_ngram and --gen_min_new_tokens are served by fvqa.generate.generate: they need "
                       "--gen_stop_eos or --gen_vote")
    if vote_n:
        if not 2 <= vote_n <= 64:
            self.error("--gen_vote N counts samples: 2 <= N <= 64 (0: off)")
        if not getattr(a, "is_generation_task", False):
            self.error("--gen_vote belongs to generation-task validation: it needs --is_generation_task")
        if not getattr(a, "gen_vote_temperature", 1.0) > 0 or not 0 < getattr(a, "gen_vote_top_p", 1.0) <= 1:
            self.error("--gen_vote_temperature > 0, 0 < --gen_vote_top_p <= 1")
        if beams or la > 1 or jump or stream or getattr(a, "val_vocab", False) or getattr(a, "gen_frame_attention", False):
            self.error("--gen_vote draws samples in the plain token loop: not with --num_beams > 1, --lookahead > 1, "
                       "--gen_jump_forward > 1, --gen_stream, --val_vocab or --gen_frame_attention")
    if getattr(a, "vote", False):
        if not 2 <= int(getattr(a, "num_samples", 1) or 1) <= 64 or not float(getattr(a, "temperature", 0.0) or 0.0) > 0:
            self.error("--vote counts samples: it needs --num_samples N, 2 <= N <= 64, and --temperature > 0")
        if beams or la > 1 or jump or stream or int(getattr(a, "rank", 0) or 0):
            self.error("--vote draws samples in the plain token loop: not with --num_beams > 1, --lookahead > 1, jump-forward, "
                       "a stream or --rank")


class ArgumentParser(argparse.ArgumentParser):
    """argparse's parser, which also refuses --gen_constrain vocab without its --answer_vocab file and --contrast with
    --num_beams > 1 (a contrastive beam step is not built) or with parameters out of range, and --lookahead or
    --gen_jump_forward (answer.py: --jump_forward) out of range or together with a decode they are not built for, and
    --gen_stream (answer.py: --slots) with a decode the stream does not run (answer.py uses it too), and
    --gen_frame_attention (answer.py: --frame_attention) with a decode that does not report it, and --val_frame_attention
    with a validation that does not score options or scores them twice, and --val_flipped with a validation that does not
    score options or combines their scores another way, and --val_vocab without its vocabulary and generation prompts or with
    a decode (it runs none), and --gen_draft (answer.py: --draft) without its --lookahead R, its prompts or its vocabulary, or
    with a decode the tree drafts are not built for; --lookahead may reach 64 only with it; and the pick rules (--gen_no_repeat_ngram,
    --gen_min_new_tokens; answer.py: --min_p, --no_repeat_ngram, --min_new_tokens) and the vote (--gen_vote; answer.py: --vote) out
    of range or with a decode fvqa.generate.generate refuses them with."""

    def parse_args(self, args=None, namespace=None):
        a = super().parse_args(args, namespace)
        if getattr(a, "gen_constrain", None) == "vocab" and not getattr(a, "answer_vocab", None):
            self.error("--gen_constrain vocab needs --answer_vocab FILE (one answer per line)")
        if getattr(a, "contrast", None):
            if int(getattr(a, "num_beams", 1) or 1) > 1:
                self.error("--contrast decodes with num_beams == 1: a contrastive beam search is not built")
            if not a.contrast_alpha >= 0 or not 0 <= a.contrast_beta <= 1:
                self.error("--contrast_alpha >= 0, 0 <= --contrast_beta <= 1")
        la = int(getattr(a, "lookahead", 0) or 0)
        drafted = getattr(a, "gen_draft", None) or getattr(a, "draft", None)
        if la < 0 or la > (64 if drafted else 16):
            self.error("0 <= --lookahead <= 16 (64 rows per pass with --gen_draft / --draft)")
        for flag in ("gen_draft", "draft"):
            d = getattr(a, flag, None)
            if not d:
                continue
            if la < 2:
                self.error(f"--{flag} drafts a trie of answers for a tree pass: it needs --lookahead R, 2 <= R <= 64")
            if flag == "gen_draft" and not getattr(a, "is_generation_task", False):
                self.error("--gen_draft belongs to generation-task validation: it needs --is_generation_task")
            if d == "vocab" and not getattr(a, "answer_vocab", None):
                self.error(f"--{flag} vocab needs --answer_vocab FILE (one answer per line)")
            if flag == "draft" and d == "options" and not getattr(a, "options", None):
                self.error("--draft options needs --options")
            if (int(getattr(a, "num_beams", 1) or 1) > 1 or getattr(a, "gen_constrain", None) or getattr(a, "constrain", False)
                    or getattr(a, "contrast", None) or int(getattr(a, "gen_jump_forward", 0) or 0) > 1
                    or int(getattr(a, "jump_forward", 0) or 0) > 1 or int(getattr(a, "gen_stream", 0) or 0) >= 1
                    or int(getattr(a, "slots", 0) or 0) >= 1 or getattr(a, "val_vocab", False)
                    or getattr(a, "gen_frame_attention", False) or getattr(a, "frame_attention", False)
                    or int(getattr(a, "rank", 0) or 0) or int(getattr(a, "num_samples", 1) or 1) > 1
                    or (float(getattr(a, "temperature", 0.0) or 0.0) > 0 and getattr(a, "seed", None) is None)):
                self.error(f"--{flag} verifies a draft trie against the model's own pick: not with --num_beams > 1, constrained "
                           "or contrastive decoding, jump-forward, a stream, --val_vocab / --rank, frame attention, several "
                           "samples per prompt or sampling without a --seed")
        if la > 1:
            if int(getattr(a, "num_beams", 1) or 1) > 1 or getattr(a, "gen_constrain", None) or getattr(a, "contrast", None):
                self.error("--lookahead verifies drafts against the model's own pick: not with --num_beams > 1, --gen_constrain "
                           "or --contrast")
            if int(getattr(a, "num_samples", 1) or 1) > 1:
                self.error("--lookahead keeps its pass state on the prefill's cache: not with --num_samples > 1")
            if float(getattr(a, "temperature", 0.0) or 0.0) > 0 and getattr(a, "seed", None) is None:
                self.error("--lookahead with --temperature > 0 gives the plain sampled answer of the same --seed: it needs --seed")
            if not float(getattr(a, "temperature", 0.0) or 0.0) > 0 and (
                    int(getattr(a, "top_k", 0) or 0) != 0 or float(getattr(a, "repetition_penalty", 1.0) or 1.0) != 1.0):
                self.error("--lookahead without --temperature > 0 verifies drafts against the plain greedy choice: --top_k and "
                           "--repetition_penalty need --temperature > 0 here")
            if not 1 <= int(getattr(a, "lookup_ngram", 2)) <= 4:
                self.error("1 <= --lookup_ngram <= 4")
        for flag, constrained in (("gen_jump_forward", getattr(a, "gen_constrain", None)),
                                  ("jump_forward", getattr(a, "constrain", False) or getattr(a, "answer_vocab", None))):
            jf = int(getattr(a, flag, 0) or 0)
            if jf < 0 or jf > 16:
                self.error(f"0 <= --{flag} <= 16")
            if jf > 1:
                if not constrained:
                    self.error(f"--{flag} commits the tokens a trie of allowed answers fixes: it needs "
                               + ("--gen_constrain" if flag == "gen_jump_forward" else "--constrain or --answer_vocab"))
                if int(getattr(a, "num_beams", 1) or 1) > 1 or getattr(a, "contrast", None) or la > 1:
                    self.error(f"--{flag} is built for the greedy pick: not with --num_beams > 1, --contrast or --lookahead > 1")
        for flag, admit in (("gen_stream", "gen_stream_admit"), ("slots", "admit")):
            n = int(getattr(a, flag, 0) or 0)
            if n < 0 or n > 65535:
                self.error(f"0 <= --{flag} <= 65535")
            m = getattr(a, admit, None)
            if m is not None and not (n >= 1 and 1 <= int(m) <= n):
                self.error(f"--{admit} lies in [1, --{flag}]")
            if n >= 1 and (int(getattr(a, "num_beams", 1) or 1) > 1 or getattr(a, "contrast", None) or la > 1
                           or int(getattr(a, "gen_jump_forward", 0) or 0) > 1 or int(getattr(a, "jump_forward", 0) or 0) > 1
                           or int(getattr(a, "num_samples", 1) or 1) > 1):
                self.error(f"--{flag} decodes one token per row and pass: not with --num_beams > 1, --contrast, --lookahead > 1, "
                           "jump-forward or several samples per prompt")
        for flag in ("gen_frame_attention", "frame_attention"):
            if not getattr(a, flag, False):
                continue
            if flag == "gen_frame_attention" and not (getattr(a, "gen_stop_eos", False) or getattr(a, "gen_constrain", None)):
                self.error("--gen_frame_attention is reported by fvqa.generate.generate: it needs --gen_stop_eos or --gen_constrain")
            if (int(getattr(a, "num_beams", 1) or 1) > 1 or getattr(a, "contrast", None) or la > 1
                    or int(getattr(a, "gen_jump_forward", 0) or 0) > 1 or int(getattr(a, "jump_forward", 0) or 0) > 1
                    or int(getattr(a, "gen_stream", 0) or 0) >= 1 or int(getattr(a, "slots", 0) or 0) >= 1):
                self.error(f"--{flag} is served by the plain token loop: not with --num_beams > 1, --contrast, --lookahead > 1, "
                           "jump-forward or a stream")
        _check_pick_rules(self, a, la)
        if int(getattr(a, "log_video_mass", 0) or 0) < 0:
            self.error("--log_video_mass EVERY >= 0 (0: off)")
        if getattr(a, "val_frame_attention", False):
            if getattr(a, "is_generation_task", False):
                self.error("--val_frame_attention belongs to multiple-choice validation: with --is_generation_task use "
                           "--gen_frame_attention")
            if getattr(a, "contrast", None):
                self.error("--val_frame_attention describes one scoring pass: not with --contrast")
        if getattr(a, "val_flipped_weights", None) is not None and not getattr(a, "val_flipped", False):
            self.error("--val_flipped_weights W_VAQ W_QAV belongs to --val_flipped")
        if getattr(a, "val_flipped", False):
            if getattr(a, "is_generation_task", False):
                self.error("--val_flipped belongs to multiple-choice validation: not with --is_generation_task")
            if getattr(a, "contrast", None) or getattr(a, "val_frame_attention", False):
                self.error("--val_flipped combines the three tasks' scores: not with --contrast or --val_frame_attention")
        if getattr(a, "val_vocab", False):
            if not getattr(a, "answer_vocab", None) or not getattr(a, "is_generation_task", False):
                self.error("--val_vocab scores the answers of --answer_vocab FILE behind generation prompts: it needs "
                           "--answer_vocab and --is_generation_task")
            if (int(getattr(a, "num_beams", 1) or 1) > 1 or la > 1 or int(getattr(a, "gen_jump_forward", 0) or 0) > 1
                    or int(getattr(a, "gen_stream", 0) or 0) >= 1 or getattr(a, "gen_frame_attention", False)):
                self.error("--val_vocab scores every member in one pass, nothing is decoded: not with --num_beams > 1, "
                           "--lookahead, --gen_jump_forward, --gen_stream or --gen_frame_attention")
        return a


def get_args_parser():
    parser = ArgumentParser("Flipped-VQA training (MI355X)", add_help=False)
    for flag, kw in _FLAGS:
        parser.add_argument(flag, **kw)
    parser.set_defaults(pin_mem=True)
    return parser


def validate_args(args):
    """Audio flag consistency (reference train.py:154-168)."""
    assert isinstance(args.audio, bool) and isinstance(args.audio_only, bool)
    if args.audio_only:
        assert args.audio, "If audio_only is True, audio must also be set to True"
    if args.audio and args.audio_only:
        assert args.audio_merge == "none", "If you only need audio, you should not specify merge method"
        args.audio_merge = None
    if args.audio and not args.audio_only:
        assert args.audio_merge in ("sum", "concat", "attention"), \
            "An audio_merge method must be specified if audio is True and audio_only is False"
    if getattr(args, "train_audio", False):
        assert args.audio, "--train_audio needs --audio: without it the model has no audio front end"
        if args.audio_merge == "concat":
            print("--train_audio changes nothing with --audio_merge concat: that mode has no frozen audio part "
                  "(the audio columns of visual_proj train already)")


def build_loaders(args, model):
    if args.synthetic or args.dataset == "synthetic":
        p = model.params
        cfg = synth.SynthConfig(dim=p.dim, n_heads=p.n_heads, n_layers=p.n_layers, vocab_size=model.vocab_size,
                                max_feats=args.max_feats, max_seq_len=args.max_seq_len, batch_size=args.batch_size,
                                vaq=args.vaq, qav=args.qav, audio=model.audio_mode,
                                audio_len=1 if model.audio_mode == "attention" else 0)   # (one audio row per clip, as MusicAVQA hands)
        val = None
        if getattr(args, "val_flipped", False):          # --val_flipped validates on synthetic options with all three streams
            val = [synth.make_flipped_option_batch(cfg, 5, seed=4321 + misc.get_rank() + misc.get_world_size() * i,
                                                   batch_size=args.val_batch_size or args.batch_size)
                   for i in range(min(2, args.synthetic_batches))]
        return synth.SyntheticLoader(cfg, args.synthetic_batches, misc.get_rank(), misc.get_world_size(), pin=True), val
    from dataloader import load_data          # NExT-QA / MusicAVQA readers + collate of this package (dataloader/)
    return load_data(args, model.tokenizer, split="train"), load_data(args, model.tokenizer, split="val")


def main(args):
    misc.init_distributed_mode(args)
    print("job dir: {}".format(os.path.dirname(os.path.realpath(__file__))))
    print("{}".format(args).replace(", ", ",\n"))
    torch.cuda.set_device(args.gpu)

    seed = args.seed + misc.get_rank()
    torch.manual_seed(seed)
    np.random.seed(seed)

    model = LLaMA_VQA(args)
    model.to(torch.device("cuda", args.gpu))
    model_without_ddp = model
    train_loader, val_loader = build_loaders(args, model)

    eff_batch_size = args.batch_size * args.accum_iter * misc.get_world_size()
    if args.lr is None:
        args.lr = args.blr * eff_batch_size / 256
    print("base lr: %.2e" % (args.lr * 256 / eff_batch_size))
    print("actual lr: %.2e" % args.lr)
    print("accumulate grad iterations: %d" % args.accum_iter)
    print("effective batch size: %d" % eff_batch_size)

    groups = param_groups_weight_decay(model_without_ddp, args.weight_decay)
    if getattr(model_without_ddp, "train_norm", False):       # the norm weights are 1-D: the rule above leaves them undecayed
        own = dict(model_without_ddp.named_parameters())
        no_decay = {id(p) for p in groups[0]["params"]}
        assert all(id(own[n]) in no_decay for n in synth.norm_train_names(model_without_ddp.engine_layer_ids())), \
            "--train_norm: a norm weight landed in the weight-decay group"
    optimizer = FusedAdamW(groups, lr=args.lr, betas=(0.9, 0.95), flat=model_without_ddp.flat_params())
    if args.distributed:
        model = DataParallel(model)
        optimizer.grad_sync = model.sync_grads
    print(optimizer)
    loss_scaler = NativeScaler()
    misc.load_model(args=args, model_without_ddp=model_without_ddp, optimizer=optimizer, loss_scaler=loss_scaler)
    if args.distributed:                       # whatever each rank loaded, replicas start from rank 0's state
        model.broadcast_params()
        model.broadcast_optimizer(optimizer, loss_scaler)

    print(f"Start training for {args.epochs} epochs")
    t0 = time.time()
    best_acc = 0.0
    for epoch in range(args.start_epoch, args.epochs):
        sampler = getattr(train_loader, "sampler", None)
        if args.distributed and hasattr(sampler, "set_epoch"):
            sampler.set_epoch(epoch)
        # pinned single-copy H2D staging on a side stream: the step never waits for a pageable copy
        staged = DeviceBatchProducer(train_loader, torch.device("cuda", args.gpu), depth=3)
        train_stats = train_one_epoch(model, staged, optimizer, epoch, loss_scaler, args=args)
        log_stats = {**{f"train_{k}": v for k, v in train_stats.items()}, "epoch": epoch}
        val_stats = None
        if val_loader is not None:
            try:
                from engine import val_one_epoch        # provided by the reference checkout, if present
                val_stats = val_one_epoch(model_without_ddp, val_loader, optimizer, epoch, args=args)
            except ImportError:
                val_stats = None
        if val_stats is not None:
            log_stats.update({f"val_{k}": v for k, v in val_stats.items()})
        improved = val_stats is None or best_acc < val_stats["acc"]
        if args.output_dir and improved:
            best_acc = val_stats["acc"] if val_stats is not None else best_acc
            misc.save_model(args=args, model=model, model_without_ddp=model_without_ddp, optimizer=optimizer,
                            loss_scaler=loss_scaler, epoch=epoch, name="checkpoint_best")
        if args.output_dir and misc.is_main_process():
            with open(os.path.join(args.output_dir, "log.txt"), mode="a", encoding="utf-8") as f:
                f.write(json.dumps(log_stats) + "\n")
    print("Training time {}".format(str(datetime.timedelta(seconds=int(time.time() - t0)))))


if __name__ == "__main__":
    args = get_args_parser().parse_args()
    validate_args(args)
    if args.output_dir:
        Path(args.output_dir).mkdir(parents=True, exist_ok=True)
    main(args)
