"""Validation / generation path (reference llama/model.py:367-546, engine.py:59-145).

The reference decodes greedily by re-running the WHOLE sequence through all layers once per generated token
and per sample (31 forwards of (1, S) per sample, no KV cache). Here the prompt is run once for the whole
batch (the training forward, which already keeps every layer's q/k/v in the arena = the KV cache); each
further token recomputes only its own row per sample: RMSNorm -> QKV row -> the one-query-row gated attention
kernel over the cached keys (RoPE inside; the row's k, v join the cache) -> WO -> SwiGLU MLP -> LM head row -> argmax. Causality makes this identical to
the reference's re-forward: rows before the new token do not change, rows after it are never read.
The answer is then matched to the choices by cosine similarity of mean token embeddings, with the
reference's quirks kept (choices padded with id 0 before averaging, llama/model.py:566-575)."""
from __future__ import annotations

import contextlib
import types
from typing import List, Tuple

import torch

from . import attribution, constrain, ops, rowpass

N_NEW = 31          # reference llama/model.py:438: positions prefix-1 .. prefix+29


@contextlib.contextmanager
def vqa_stream_only(eng, arenas: str, lm_head_rows: str):
    """The engine as an evaluation path runs it — the VQA stream alone, in the arenas kept under the attribute `arenas`
    (`_gen_arena`, `_score_arena`: the training step's activations stay where they are), the LM head on `lm_head_rows` — with
    the training configuration (tasks / n_streams / _arena / _vstart / lm_head_rows) put back on the way out."""
    with streams_only(eng, ["vqa"], arenas, lm_head_rows):
        yield eng


@contextlib.contextmanager
def streams_only(eng, tasks, arenas: str, lm_head_rows: str):
    """vqa_stream_only for any streams: the engine runs `tasks` (of vqa, vaq, qav, in that order) for the call, in the arenas kept
    under the attribute `arenas`, and gets its training configuration back on the way out (fvqa/flipped.py: the VAQ and QAV
    streams of the answer options)."""
    saved = (eng.tasks, eng.n_streams, eng._arena, eng._vstart, eng.lm_head_rows)
    eng.tasks, eng.n_streams, eng._arena, eng._vstart = list(tasks), len(tasks), getattr(eng, arenas), {}
    eng.lm_head_rows = lm_head_rows
    try:
        yield eng
    finally:
        setattr(eng, arenas, eng._arena)
        eng.tasks, eng.n_streams, eng._arena, eng._vstart, eng.lm_head_rows = saved


def _need_prefix(data: dict) -> None:
    if "prefix_index" not in data or "vqa" not in data["prefix_index"]:
        raise ValueError("generation needs data['prefix_index']['vqa'] (where each answer starts; "
                         "reference llama/model.py:381)")


def _option0(data: dict, twin=None) -> dict:
    """The prefill's batch: option 0 of every sample with its features; under `contrast` the B prompts with their clips, then
    the same prompts with the twin's."""
    sub = {k: data[k] for k in ("video", "audio") if k in data}      # (the audio-only batch has no "video")
    sub.update({"text_id": {"vqa": data["text_id"]["vqa"][:, 0:1]}, "label": {"vqa": data["label"]["vqa"][:, 0:1]},
                "video_start": {"vqa": data["video_start"]["vqa"], "vaq": data["video_start"]["vqa"]}})
    if twin is not None:
        for k, v in twin.items():
            sub[k] = torch.cat([sub[k], v.to(device=sub[k].device, dtype=sub[k].dtype)], 0)
        sub["text_id"] = {"vqa": sub["text_id"]["vqa"].repeat(2, 1, 1)}
        sub["label"] = {"vqa": sub["label"]["vqa"].repeat(2, 1, 1)}
    return sub


def _prefill(eng, data: dict, twin=None) -> types.SimpleNamespace:
    """The prompt, once: the training forward on `_option0` — logits of every position, and every layer's k / v stay in the arena
    = the KV cache. -> B (the prefill's rows: twice the samples under `contrast`), S, ar (the arena), vstart, ids (B, S) int64 (a
    copy of the prompts), prefix (B,) int64, start = prefix - 1 (the position the first token is predicted at), first (B, V) (the
    logits rows at `start`), rows = arange(B), rotated (rowpass.cache_rotated)."""
    sub = _option0(data, twin)
    dev = eng.device
    B, _, S = sub["text_id"]["vqa"].shape
    with vqa_stream_only(eng, "_gen_arena", "all"):         # the prefill's logits are read at the prefix positions: every row
        eng.forward(sub)
        ar, vstart = eng.arena(B, S), eng.saved["vstart"]
    rotated = rowpass.cache_rotated(eng)
    ids = sub["text_id"]["vqa"][:, 0].to(dev).clone()
    prefix = torch.as_tensor([int(p) for p in data["prefix_index"]["vqa"]] * (1 if twin is None else 2), device=dev)
    start = prefix - 1
    rows = torch.arange(B, device=dev)
    first = ar.logits.view(B, S, eng.V)[rows, start.clamp(0, S - 1)]
    return types.SimpleNamespace(B=B, S=S, ar=ar, vstart=vstart, ids=ids, prefix=prefix, start=start, first=first, rows=rows,
                                 rotated=rotated)


def _one_row_attn(eng, p, kv, vstart, pos, mass=None):
    """rowpass.layers' attention for one new row per sequence: the row against the cached keys / values of `kv` (+ adapter
    prefix); its k, v join the cache at `pos`. mass (None: the launch of every call before the keyword existed): a one-element
    list that holds the (L, R, H, F + 2) fp32 tensor of the pass being queued — layer i writes its rows' frame-attention
    summary into slice i (ops.attn_decode_mass: the same output and cache bits)."""
    def attn(i, qkv, o):
        ops.attn_decode(qkv, kv[i], o, *eng.model.gate_views(i), vstart, pos, (eng.cos, eng.sin), qkv.shape[0], p.S, eng.H,
                        eng.Dh, eng.A, eng.F, cache_rotated=p.rotated)

    def attn_mass(i, qkv, o):
        ops.attn_decode_mass(qkv, kv[i], o, mass[0][i], *eng.model.gate_views(i), vstart, pos, (eng.cos, eng.sin), qkv.shape[0],
                             p.S, eng.H, eng.Dh, eng.A, eng.F, cache_rotated=p.rotated)
    return attn if mass is None else attn_mass


class _LagOneStop:
    """The stop that lags by one step (generate's docstring): after token step t the count of running rows goes to pinned host
    memory behind an event, and step t + 1 is only launched once the count of step t - 1 has arrived and is not zero.
    early_stop=False: every step may be launched."""

    def __init__(self, max_steps: int, early_stop: bool = True):
        self.running = torch.empty(max_steps, dtype=torch.int32).pin_memory()
        self.arrived = []
        self.early_stop = early_stop

    def may_launch(self, t: int) -> bool:
        if t < 2 or not self.early_stop:
            return True
        self.arrived[t - 2].synchronize()                   # the count of step t - 2 left the device a whole step ago
        return int(self.running[t - 2]) != 0

    def queued(self, t: int, n_active: torch.Tensor) -> None:
        """Step t is queued; n_active (1,) int32 on the device is where it leaves its count."""
        self.running[t:t + 1].copy_(n_active, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self.arrived.append(ev)


def _read_back(ids, prefix, n_generated, col):
    """ids (B, S) int64, prefix and n_generated (B,) int64, col = arange(width)[None] -> (tokens (B, width) int32: the generated
    tokens of each row as its id row holds them, -1 from n_generated on; inside (B, width) bool: col < n_generated)."""
    inside = col < n_generated.unsqueeze(1)
    tok = ids.gather(1, (prefix.unsqueeze(1) + col).clamp(max=ids.shape[1] - 1)).to(torch.int32)
    return torch.where(inside, tok, torch.full_like(tok, -1)), inside


@torch.no_grad()
def greedy_decode(eng, data: dict, n_new: int = N_NEW) -> torch.Tensor:
    """-> ids (B, S) int64 on the device: option 0's prompt with the generated tokens written from
    position prefix_index['vqa'][b] on (reference llama/model.py:428-470)."""
    _need_prefix(data)
    p = _prefill(eng, data)
    pk, dev, B, S = eng.pack, eng.device, p.B, p.S
    ids, pos = p.ids, p.start                               # start_idx of the first iteration
    pred = p.first.argmax(-1)
    b = rowpass.buffers(eng, B, xin=False)
    for _ in range(n_new):
        ok = pos + 1 < S                                    # the reference would index past the end here
        tgt = (pos + 1).clamp(max=S - 1)
        ids[torch.arange(B, device=dev), tgt] = torch.where(ok, pred, ids[torch.arange(B, device=dev), tgt])
        pos = tgt
        x = pk.emb[ids[torch.arange(B, device=dev), pos]].contiguous()
        x = rowpass.layers(eng, b, _one_row_attn(eng, p, p.ar.qkv, p.vstart, pos), x)
        rowpass.head(eng, x, b.xn, b.lg)
        pred = b.lg.argmax(-1)
    return ids


@torch.no_grad()
def match_answers(model, data: dict, ids: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, List[dict]]:
    """-> (index of the most similar choice (B,), similarities (B, n_options), extracted answers)
    (reference llama/model.py:476-546 and helpers :551-623)."""
    tok = model.tokenizer
    emb = model.tok_embeddings.weight.data
    ids_all = data["text_id"]["vqa"].to(ids.device)
    label0 = data["label"]["vqa"][:, 0].to(ids.device)
    B, n_opt, S = ids_all.shape
    a_id, eos = tok.a_token_id, tok.eos_id
    out_vec, choice_vec, extracted = [], [], []
    for b in range(B):
        gen = ids[b, 1:][label0[b, 1:] != 0]                # generated tokens at the gold answer's positions
        hit = (gen == eos).nonzero()
        if hit.numel():
            gen = gen[: int(hit[0])]
        out_vec.append(emb[gen].float().mean(0) if gen.numel() else torch.zeros(emb.shape[1], device=ids.device))
        row0 = ids_all[b, 0].tolist()
        start = row0.index(a_id) + 5
        answers = []
        for c in range(n_opt):
            tail = ids_all[b, c, start:].tolist()
            end = start + tail.index(eos) if eos in tail else S
            answers.append(ids_all[b, c, start:end])
        padded = torch.nn.utils.rnn.pad_sequence(answers, batch_first=True, padding_value=0)
        choice_vec.append(emb[padded].float().mean(1))      # the padding id 0 is averaged in, as in the reference
        seq = ids[b].tolist()
        try:
            q0 = seq.index(894) + 2                          # "Question" at a line start (reference :519)
        except ValueError:
            q0 = 0
        q1 = seq.index(a_id)
        ans = seq[q1 + 5:]
        stop = ans.index(eos) if eos in ans else next((k for k, t in enumerate(ans) if t == 0), len(ans))
        extracted.append({"video_id": data["vid"][b] if "vid" in data else None,
                          "question": tok.decode(seq[q0:q1]), "generated_answer": tok.decode(ans[:stop])})
    o = torch.nn.functional.normalize(torch.stack(out_vec), p=2, dim=1)
    c = torch.nn.functional.normalize(torch.stack(choice_vec), p=2, dim=2)
    sims = torch.bmm(c, o.unsqueeze(-1)).squeeze(-1)
    return sims.argmax(1), sims, extracted


# ---------------------------------------------------------------------------------------------- the generation API
@torch.no_grad()
def generate(eng, data: dict, *, max_new_tokens: int = N_NEW, temperature: float = 0.0, top_p: float = 1.0,
             stop_at_eos: bool = True, seed=None, num_beams: int = 1, length_penalty: float = 0.0, top_k: int = 0,
             repetition_penalty: float = 1.0, return_logprobs: bool = False, num_return_sequences: int = 1,
             constraints=None, contrast=None, contrast_alpha: float = 1.0, contrast_beta: float = 0.1,
             lookahead: int = 0, lookup_ngram: int = 2, draft_tokens=None, jump_forward: int = 0,
             frame_attention: bool = False, draft_answers=None, min_p: float = 0.0, no_repeat_ngram_size: int = 0,
             min_new_tokens: int = 0, vote: bool = False) -> dict:
    """A prompt in, tokens out: greedy (temperature == 0) or temperature / nucleus sampling with the reference's rule
    (llama/generation.py:17-68), each row ended by its EOS. `data` is a validation batch or one of `prompt_batch`. The prefill
    and the per-layer kernel sequence are those of `greedy_decode`; the token step — pick, write, advance, raise `done`, gather
    the next embedding, count the running rows — is ONE launch (ops.decode_next, csrc/sample.hip).
    -> {"ids" (B, S) int64, "n_generated" (B,) int64, "steps": token steps launched, "tokens" (B, steps) int32 (-1: no token)}.
    Sampling draws its uniforms from one device generator seeded with `seed` once per call (None: the default generator).
    The stop lags by one step so that the device never idles: after token step t the count of running rows goes to pinned host
    memory behind an event, and token step t + 1 is only launched once the count of step t - 1 has arrived and is not zero —
    the host never waits for the step it has just queued, and at most one superfluous step is computed.
    num_beams > 1 (with temperature == 0): beam search, `beam_search` below — the keys above for the best hypothesis plus
    "score" and "beams". num_beams == 1 is the code below.
    top_k, repetition_penalty, return_logprobs, num_return_sequences: at their defaults (0, 1.0, False, 1) the call launches
    exactly what it launched before they existed; any other value sends the token step through ops.decode_next_ex, still one
    launch (include/fvqa.h fvqa_decode_next_ex states the rule).
      top_k >= 1: only the k most likely tokens are sampled from; top_p then bounds the mass in front of a token by top_p times
        the mass of those k. Ignored when temperature == 0.
      repetition_penalty r >= 1 (CTRL): the logits of the tokens GENERATED so far in the row are divided (if positive) or
        multiplied (if not) by r before the pick, each id once. The prompt's tokens are not penalised — it lists the answer
        options and must not push the model away from them (Hugging Face's processor penalises the prompt too).
      return_logprobs: adds "logprobs" (B, steps) fp32 — log_softmax of the RAW logits at each picked token (no penalty,
        temperature 1, no cut: the model's own log-probability, what beam search sums into "score"), 0 where "tokens" is -1 —
        and "sum_logprob" (B,).
      num_return_sequences n > 1 (needs temperature > 0, num_beams == 1, B * n <= 65535): n samples per prompt from ONE prefill —
        its cache rows and the adapter rows are fanned out to n rows per sample (ops.kv_beam_move into beam search's cache, one
        launch; samples never change parent, so nothing moves per token) and the token loop runs on B * n rows; the uniforms
        are one torch.rand(max_new_tokens, B * n). The results gain a sample axis: "ids" (B, n, S), "n_generated" (B, n),
        "tokens" / "logprobs" (B, n, steps), "sum_logprob" (B, n).
    constraints (None: every code path above runs untouched): the set of allowed answers — a fvqa.constrain.TokenTrie, or raw
      token sequences (one list for the batch, or one list per sample) that are compiled here. Every token step may only continue
      a prefix of an allowed answer, and only the EOS ends one: greedy and sampled rows are members of the set by construction,
      and beam search with num_beams >= the number of members returns the most likely member under the model (length_penalty 1:
      by the mean log-probability of its tokens, the multiple-choice criterion). The token step goes through
      ops.decode_next_trie / ops.beam_step_trie, still one launch (include/fvqa.h states the rule); all other keywords keep
      their meaning, with "every token" read as "every allowed token". The results gain "choice": the index of the generated
      member in its sample's list, (B,) — (B, n) with num_return_sequences = n; under beam search the best hypothesis' and
      "beams"["choice"] (B, K) —, -1 for a row that ended before a leaf. ValueError: stop_at_eos=False (a leaf is reached by
      the EOS), a member (EOS included) longer than max_new_tokens, a member that does not fit behind its prompt inside S.
    contrast (None: every code path above runs untouched): contrastive decoding against a TWIN of the prompt — the same text run
      a second time with other features — so that every token is picked from the difference of the two predictions and the
      language prior is discounted (visual contrastive decoding; classifier-free guidance for language models).
      contrast="blind": the twin's "video" and / or "audio" (whichever the batch has) are zeros — visual_proj has no bias, so a
      zero frame becomes temporal_emb alone, which is what every zero-padded frame slot of a short clip looks like in training.
      contrast={"video": ..., "audio": ...}: replacement tensors of the batch's own shapes (another clip, shuffled frames).
      The rule, per sample and token step in fp32 (include/fvqa.h fvqa_decode_next_pair states it), with lp = log_softmax(l) of
      the raw row: P = {i allowed : l+_i - max_allowed l+ >= log(contrast_beta)} is the plausible set (beta 0: everything,
      beta 1: the maxima), c_i = l+_i + contrast_alpha * (lp+_i - lp-_i) for i in P, and everything else — the repetition
      penalty, the greedy pick, temperature, top_k, top_p, the trie of `constraints` — sees c over P where it saw l over the
      allowed tokens. alpha == 0 (or a twin equal to the batch) picks from l+ itself. "logprobs" stay lp+ of the picked token.
      The flow: ONE prefill of 2 * B sequences (the features concatenated, the ids repeated), the fan-out of
      num_return_sequences over 2 * B parents (rows: B * n positives, then B * n negatives), the token loop unchanged on
      2 * B * n rows with ops.decode_next_pair as its token step — still one launch, which steps both rows of a pair with one
      token —, the lag-one stop on the count of pairs. The results have today's shapes, taken from the positive rows, and gain
      "n_plausible" (B[, n], steps) int32: |P| at each step, 0 where "tokens" is -1.
      ValueError: a key the batch lacks, a tensor of another shape, contrast_alpha < 0, contrast_beta outside [0, 1],
      num_beams > 1, 2 * B * num_return_sequences > 65535. Not built: a contrastive beam step; negatives whose TEXT differs.
    lookahead T (0 or 1: every code path above runs untouched): draft-and-verify decoding, `_generate_lookahead` below —
      several tokens per pass through the layers (prompt-lookup / assisted generation). A pass carries up
      to T rows per sample: the last committed token and a draft of up to T - 1 tokens behind it; every draft token that equals
      the model's own choice is committed, so "ids", "n_generated" and "tokens" are those of the plain call with the same
      arguments, token for token ("tokens" is (B, longest row), padded with -1). temperature == 0: the choice is greedy's.
      temperature > 0 (with top_p, top_k, repetition_penalty as in the plain call, and a seed, which is required): the choice at token index t is the
      plain sampler's with the plain loop's draw u[t] — the draws are the same one torch.rand(max_new_tokens, B) of the seeded
      generator, read by token index and not by step —, and a draft is kept iff it equals the sampled token: for a deterministic
      draft that IS the rejection rule of speculative sampling, nothing is approximate. The draft: with draft_tokens (B, max_new_tokens) int32 the answer someone
      else proposes, read at each row's n_generated (an entry outside [0, vocab) ends a draft); without, prompt lookup — the
      longest suffix of up to lookup_ngram (1 .. 4) committed tokens that occurs earlier in the row, most recent occurrence, and
      what followed it (a multiple-choice prompt lists its answers). include/fvqa.h fvqa_spec_step states the rule. "steps" counts
      the token steps launched; the results gain "n_committed" and "n_drafted" (B, steps) int32: the tokens each step committed
      and the draft tokens it was offered. return_logprobs is served as above ("logprobs" (B, longest row), "sum_logprob").
      ValueError: temperature > 0 without a seed, num_beams > 1, num_return_sequences > 1 (the pass state sits on the prefill arena, not the fan-out cache),
      top_k or repetition_penalty != 1 at temperature == 0, constraints, contrast, lookahead > 16 (ops.SUFFIX_MAX) or < 0,
      draft_tokens of another shape or without lookahead >= 2, lookup_ngram outside [1, 4], B * T > 65535; under sampling also
      top_p outside (0, 1], top_k < 0, repetition_penalty < 1. Not built: several samples per prompt on a draft pass, drafts
      under beam search, a trie or a contrastive pick; a draft model (a draft with a distribution of its own).
    draft_answers C (None: every code path above runs untouched; needs lookahead = R, 2 <= R <= 64): the drafts are a TRIE of
      likely answers — what `constraints` accepts: one list of token sequences, or one list per sample —, verified in one tree pass,
      `_generate_tree_draft` below. The trie is a draft, not a rule: "ids", "n_generated" and "tokens" are the plain call's,
      token for token, whatever the model says — greedy's at temperature == 0, the plain sampled call's at temperature > 0 (as
      under lookahead: the pick at token index t is the plain sampler's with the draw u[t], and the walk follows it). A pass feeds up to R rows per sample: a pre-order prefix of the subtree under the
      row's trie node (ops.attn_suffix_tree: a row sees the cache and its ancestors); the token step walks the tree along the
      model's own picks (include/fvqa.h fvqa_tree_spec_step states the rule) and ops.kv_tree_commit appends the accepted path to
      the cache. A row that leaves the trie goes on one token per pass and does not re-enter; once every running row has left
      (known one step late, as the stop is) the passes carry one row per sample and launch what lookahead's loop launches at T = 1.
      The results gain "n_committed", "n_drafted" (B, steps) int32 — rows fed minus one — and "rows_per_pass" (steps,) int32: the
      rows per sample of the pass each step verified (step 0: the prefill's row, 1). return_logprobs is served as under lookahead.
      ValueError: no lookahead >= 2, R > 64, B * R > 65535, draft_tokens, temperature > 0 without a seed, top_k or repetition_penalty != 1 at temperature == 0,
      num_return_sequences > 1, num_beams > 1, constraints, contrast, jump_forward, frame_attention. Not built: several samples
      per prompt, beams, constraints or contrast on a tree pass; tree drafts in the stream; a draft root other than the start
      of the answer; compacting a pass to the live rows of each sample.
    jump_forward T (0 or 1: every code path above runs untouched; needs `constraints`): jump-forward constrained greedy decoding,
      `_generate_jump` below. Once a row's trie node has a single child the next token is fixed whatever the logits say, so a
      token step picks the one token that is a decision and commits the tokens the trie fixes behind it, up to T per step; the
      next pass feeds all of them (T rows per sample, lookahead's layer loop), so that their K / V join the cache without a pass
      of their own. Nothing is drafted and nothing rejected: "ids", "n_generated", "tokens" ((B, longest row), -1 padded) and
      "choice" are those of the plain generate(temperature=0, constraints=C) call, in as many passes as the generated path has
      real decisions, plus those that chains longer than T tokens are cut into. include/fvqa.h fvqa_trie_jump_step states the
      rule. The results gain "n_committed" (B, steps) int32. return_logprobs is served as above: a picked token's from its own
      step, a chained token's from the pass that fed it — the EOS is then always PICKED, never chained, so that a row is still
      running when the pass that owes its log-probabilities comes back (one more pass for an answer that ends in a chain).
      ValueError: no constraints, temperature > 0, num_beams > 1, top_k, repetition_penalty != 1, num_return_sequences > 1,
      contrast, lookahead >= 2, T > 16 (ops.SUFFIX_MAX) or < 0, B * T > 65535, stop_at_eos=False. Not built: sampling at the
      picks, beams, contrast; the LM head on each sample's last fed row only (the other rows' logits are computed and, without
      return_logprobs, never read).
    frame_attention (False: every code path above runs untouched): where each generated token looked. The results gain
      "frame_attention" (B[, n], steps, L, H, F + 2) fp32: per token, layer and head the weight of the text softmax
      (llama/model.py:116-120, gate2 included; the adapter softmax is not part of it) on each of the F frame keys, in front of
      the window (index F) and behind it (index F + 1) — include/fvqa.h fvqa_attn_decode_mass states it; the entries of a row sum
      to 1. Index t is the summary of the row whose logits picked token t: index 0 is read from the prefill's arena
      (attribution.arena_mass at `start`, one launch per layer and call; computed on the B prefill rows and repeated under
      num_return_sequences), index t + 1 is written by the decode pass that follows token step t (ops.attn_decode_mass in place of
      ops.attn_decode: the same launch count, the same output and cache bits, so "ids", "tokens" and "logprobs" are those of the
      call without the keyword). Zero where "tokens" is -1. attribution.summarize reduces it to a frame profile per answer.
      Served with greedy and sampled decoding, top_k, repetition_penalty, return_logprobs, num_return_sequences and constraints.
      ValueError: num_beams > 1, contrast, lookahead >= 2, jump_forward >= 2. Not built: the summary for option scoring (the
      suffix kernel's online softmax keeps no probabilities), under beams, twins, several rows per pass and the stream.
    min_p, no_repeat_ngram_size, min_new_tokens (0, 0, 0: every code path above runs untouched): three more pick rules; any of
      them off its default sends the plain token loop's step through ops.decode_next_rules, still one launch per token
      (include/fvqa.h fvqa_decode_next_rules states the rule).
      min_p in [0, 1): a token is sampled only if its probability is at least min_p times the most likely token's — on top of
        top_k and top_p: the kept set is the shortest of the three cuts, which is what Hugging Face's warpers give in sequence
        (the ratio to the maximum survives every renormalisation, and every cut keeps the maximum). Ignored at temperature == 0.
      no_repeat_ngram_size n >= 1: no n-gram occurs twice among the GENERATED tokens of a row — the tokens that would complete a
        repeat are banned before the pick. The prompt is not scanned, for the reason given for repetition_penalty: it lists the
        answer options and the answer is meant to copy one (Hugging Face's processor scans the prompt too).
      min_new_tokens m >= 1: the EOS is banned while a row has generated fewer than m tokens (needs stop_at_eos).
      A banned token takes no part in the pick at all — greedy returns the best of the others, a sampled row renormalises over
      them, top_k counts them —; "logprobs" stay the raw row's. A row whose every token is banned ends (token -1).
      Served with top_k, top_p, repetition_penalty, return_logprobs, num_return_sequences and frame_attention.
      ValueError: min_p outside [0, 1), a negative n or m, m > max_new_tokens, m > 0 with stop_at_eos=False, num_beams > 1,
      constraints, contrast, lookahead >= 2, draft_tokens, draft_answers, jump_forward >= 2. Not built: the rules under a trie,
      a twin, a draft pass or the stream; typical, eta and epsilon sampling.
    vote (False: every code path above runs untouched; needs 2 <= num_return_sequences <= ops.VOTE_SAMPLES_MAX): self-consistency
      — the samples of a prompt whose token rows are equal form a group and the largest group wins; ties go to the group whose
      first sample has the larger mean raw log-probability per generated token, then to the lower index (include/fvqa.h
      fvqa_sample_vote; one launch behind the token loop, ops.sample_vote). Served wherever num_return_sequences is — constraints
      (a group is then a `choice`) and contrast included —: it only reads the token rows. The log-probabilities are collected
      whether or not return_logprobs asks for them. The results gain "vote": {"winner" (B,), "group" (B, n), "votes" (B, n),
      "n_groups" (B,) int32, "share" (B,) fp32 = votes[winner] / n}. Not built: probability-weighted votes, votes over
      normalised answer strings."""
    rules = _pick_rules(min_p, no_repeat_ngram_size, min_new_tokens, max_new_tokens, stop_at_eos)
    if rules is not None:
        if num_beams != 1:
            raise ValueError("generate: min_p, no_repeat_ngram_size and min_new_tokens are not built for num_beams > 1")
        if constraints is not None or contrast is not None:
            raise ValueError("generate: min_p, no_repeat_ngram_size and min_new_tokens are not built for constraints or contrast")
        if lookahead >= 2 or draft_tokens is not None or draft_answers is not None:
            raise ValueError("generate: min_p, no_repeat_ngram_size and min_new_tokens are not built for lookahead or drafts")
        if jump_forward >= 2:
            raise ValueError("generate: min_p, no_repeat_ngram_size and min_new_tokens are not built for jump_forward")
    if vote:
        if int(num_return_sequences) != num_return_sequences or not 2 <= num_return_sequences <= ops.VOTE_SAMPLES_MAX:
            raise ValueError(f"generate: vote counts samples: 2 <= num_return_sequences <= {ops.VOTE_SAMPLES_MAX}")
    if frame_attention:
        if num_beams != 1:
            raise ValueError("generate: frame_attention is not built for num_beams > 1")
        if contrast is not None:
            raise ValueError("generate: frame_attention is not built for contrast")
        if lookahead >= 2 or draft_tokens is not None or draft_answers is not None:
            raise ValueError("generate: frame_attention is not built for lookahead")
        if jump_forward >= 2:
            raise ValueError("generate: frame_attention is not built for jump_forward")
    if draft_answers is not None:
        if int(lookahead) != lookahead or not 2 <= lookahead <= ops.TREE_SPEC_ROWS_MAX:
            raise ValueError(f"generate: draft_answers are verified by 2 <= lookahead <= {ops.TREE_SPEC_ROWS_MAX} rows per pass")
        if draft_tokens is not None:
            raise ValueError("generate: draft_answers and draft_tokens are two drafts: one of them")
        if jump_forward >= 2:
            raise ValueError("generate: draft_answers are not built for jump_forward")
        if num_beams != 1:
            raise ValueError("generate: draft_answers are verified against the model's own pick, not a beam: num_beams == 1")
        if num_return_sequences != 1:
            raise ValueError("generate: draft_answers are not built for num_return_sequences (the pass state sits on the "
                             "prefill's cache)")
        if constraints is not None or contrast is not None:
            raise ValueError("generate: draft_answers are not built for constraints or contrast (a draft is not a rule)")
        sampling = _draft_sampling("draft_answers", temperature, top_p, top_k, repetition_penalty, seed)
        return _generate_tree_draft(eng, data, R=int(lookahead), draft_answers=draft_answers, max_new_tokens=max_new_tokens,
                                    stop_at_eos=stop_at_eos, return_logprobs=return_logprobs, sampling=sampling, seed=seed)
    if int(lookahead) != lookahead or not 0 <= lookahead <= ops.SUFFIX_MAX:
        raise ValueError(f"generate: 0 <= lookahead <= {ops.SUFFIX_MAX} (0, 1: one token per pass)")
    if int(jump_forward) != jump_forward or not 0 <= jump_forward <= ops.SUFFIX_MAX:
        raise ValueError(f"generate: 0 <= jump_forward <= {ops.SUFFIX_MAX} (0, 1: one token per pass)")
    if jump_forward >= 2:
        if constraints is None:
            raise ValueError("generate: jump_forward commits the tokens a trie fixes: it needs constraints")
        if lookahead >= 2 or draft_tokens is not None:
            raise ValueError("generate: jump_forward and lookahead are two token steps: one of them")
        if temperature > 0 or num_beams != 1:
            raise ValueError("generate: jump_forward is built for the greedy pick: temperature == 0, num_beams == 1")
        if top_k != 0 or repetition_penalty != 1 or num_return_sequences != 1:
            raise ValueError("generate: jump_forward is not built for top_k, repetition_penalty or num_return_sequences")
        if contrast is not None:
            raise ValueError("generate: jump_forward is not built for contrast")
        return _generate_jump(eng, data, T=int(jump_forward), constraints=constraints, max_new_tokens=max_new_tokens,
                              stop_at_eos=stop_at_eos, return_logprobs=return_logprobs)
    if lookahead < 2 and draft_tokens is not None:
        raise ValueError("generate: draft_tokens are verified by lookahead >= 2")
    if lookahead >= 2:
        if num_beams != 1:
            raise ValueError("generate: lookahead verifies drafts against the model's own pick, not a beam: num_beams == 1")
        if num_return_sequences != 1:
            raise ValueError("generate: lookahead is not built for num_return_sequences (the pass state sits on the prefill's "
                             "cache)")
        if constraints is not None or contrast is not None:
            raise ValueError("generate: lookahead is not built for constraints or contrast")
        if draft_tokens is None and (int(lookup_ngram) != lookup_ngram or not 1 <= lookup_ngram <= ops.LOOKUP_NGRAM_MAX):
            raise ValueError(f"generate: 1 <= lookup_ngram <= {ops.LOOKUP_NGRAM_MAX}")
        sampling = _draft_sampling("lookahead", temperature, top_p, top_k, repetition_penalty, seed)
        return _generate_lookahead(eng, data, T=int(lookahead), G=int(lookup_ngram), draft_tokens=draft_tokens,
                                   max_new_tokens=max_new_tokens, stop_at_eos=stop_at_eos, return_logprobs=return_logprobs,
                                   sampling=sampling, seed=seed)
    if int(num_beams) != num_beams or not 1 <= num_beams <= ops.BEAMS_MAX:
        raise ValueError(f"generate: 1 <= num_beams <= {ops.BEAMS_MAX}")
    if num_beams > 1 and temperature > 0:
        raise ValueError("generate: num_beams > 1 searches, it does not sample: temperature must be 0")
    if int(top_k) != top_k or top_k < 0 or not repetition_penalty >= 1:
        raise ValueError("generate: top_k >= 0 (0: off), repetition_penalty >= 1")
    if int(num_return_sequences) != num_return_sequences or num_return_sequences < 1:
        raise ValueError("generate: num_return_sequences >= 1")
    n = int(num_return_sequences)
    if n > 1 and (num_beams > 1 or not temperature > 0):
        raise ValueError("generate: num_return_sequences > 1 draws samples: temperature > 0 and num_beams == 1")
    ex = top_k != 0 or repetition_penalty != 1 or bool(return_logprobs) or n > 1 or rules is not None
    if num_beams > 1 and ex:
        raise ValueError("generate: top_k, repetition_penalty, return_logprobs and num_return_sequences belong to "
                         "num_beams == 1 (beam search reports \"score\")")
    twin = None if contrast is None else _twin(data, contrast, contrast_alpha, contrast_beta, num_beams)
    trie = None if constraints is None else _compiled(eng, data, constraints, stop_at_eos, max_new_tokens)
    if num_beams > 1 or (_BEAM_PATH_AT_ONE and twin is None and not frame_attention):
        kw = {} if trie is None else {"constraints": trie}
        return beam_search(eng, data, max_new_tokens=max_new_tokens, stop_at_eos=stop_at_eos, num_beams=int(num_beams),
                           length_penalty=float(length_penalty), **kw)
    _need_prefix(data)
    if max_new_tokens < 1 or not temperature >= 0 or not 0 < top_p <= 1:
        raise ValueError("generate: max_new_tokens >= 1, temperature >= 0, 0 < top_p <= 1")
    NP = data["text_id"]["vqa"].shape[0] * n                # the token steps' results: one per row — per PAIR under `contrast`
    B = NP if twin is None else 2 * NP                      # the rows of the token loop
    if twin is not None and B > 65535:
        raise ValueError("generate: contrast runs two rows per sample: 2 * samples * num_return_sequences <= 65535")
    if B > 65535:
        raise ValueError("generate: at most 65535 rows (samples times num_return_sequences)")
    p = _prefill(eng, data, twin)
    pk, dev, S, V = eng.pack, eng.device, p.S, eng.V
    vstart, ids, prefix, start, first, kv = p.vstart, p.ids, p.prefix, p.start, p.first, p.ar.qkv
    i32 = dict(dtype=torch.int32, device=dev)
    if n > 1:                                               # one prefill, n rows per sample: beam search's fan-out, no re-seating
        rep = lambda t: t.repeat_interleave(n, 0).contiguous()  # noqa: E731  per sample -> per row
        kv = _beam_cache(eng, B, S, min(int(max_new_tokens), S))["qkv"]
        ops.kv_beam_move(kv, p.ar.qkv, rep(torch.arange(p.B, **i32)), torch.zeros(B, **i32), rep(prefix).to(torch.int32),
                         S=S, A=eng.A)
        vstart, ids, prefix, start = rep(vstart), rep(ids), rep(prefix), rep(start)
        first = first.unsqueeze(1).expand(p.B, n, V).reshape(B, V)
    fa = cur_mass = None
    if frame_attention:                                     # (steps, L, rows, H, F + 2): a pass writes the slice of its step
        fa = torch.zeros(max_new_tokens, eng.L, B, eng.H, eng.F + 2, dtype=torch.float32, device=dev)
        m0 = attribution.arena_mass(eng, p.B, S, p.rows, p.start.clamp(0, S - 1))      # the prefill's rows picked token 0
        fa[0].copy_(m0 if n == 1 else m0.repeat_interleave(n, 1))
        cur_mass = [fa[0]]
    b = rowpass.buffers(eng, B)
    lg, xin = b.lg, b.xin
    lg.copy_(first)
    pos = start.to(torch.int32)
    pos64 = start.clone()
    done = torch.zeros(B, **i32)
    tokens = torch.full((max_new_tokens, NP), -1, **i32)
    n_kept = torch.zeros(max_new_tokens, NP, **i32)
    n_active = torch.zeros(max_new_tokens, **i32)
    if ex or trie is not None or twin is not None:
        gen_start = prefix.to(torch.int32)
        logprobs = torch.zeros(max_new_tokens, NP, dtype=torch.float32, device=dev)
        counter = torch.zeros(1, **i32)
    if twin is not None:
        n_plausible = torch.zeros(max_new_tokens, NP, **i32)
    dtrie = node = None
    if trie is not None:                                    # every row starts at its sample's root (n rows per sample: repeated)
        dtrie = trie.to(dev)
        node = torch.as_tensor(trie.roots(NP // n), dtype=torch.int32).repeat_interleave(n).to(dev).contiguous()
    u = _draws(dev, seed, max_new_tokens, NP) if temperature > 0 else None
    kw = dict(pos64=pos64, temperature=temperature, top_p=top_p, eos_id=eng.model.tokenizer.eos_id, stop_at_eos=stop_at_eos)
    kw_ex = dict(kw, top_k=int(top_k), repetition_penalty=float(repetition_penalty))
    # a finished row stays in the batch (it is rectangular): it goes through every layer on the embedding of its last token
    # and attn_decode rewrites its K/V at its frozen position — the same values each time, read by nobody
    attn = _one_row_attn(eng, p, kv, vstart, pos64, cur_mass)
    stop = _LagOneStop(max_new_tokens)
    steps = 0
    for t in range(max_new_tokens):
        if not stop.may_launch(t):
            break
        act, ut = n_active[t:t + 1], None if u is None else u[t]
        if twin is not None:                                # both rows of every pair, one token (a trie node per pair)
            ops.decode_next_pair(lg, pk.emb, ids, pos, done, gen_start, xin, tokens[t], n_kept[t], n_plausible[t], logprobs[t],
                                 act, counter, alpha=float(contrast_alpha), beta=float(contrast_beta), node=node, trie=dtrie,
                                 u=ut, **kw_ex)
        elif trie is not None:
            ops.decode_next_trie(lg, pk.emb, ids, pos, done, gen_start, xin, tokens[t], n_kept[t], logprobs[t], act, counter,
                                 node, dtrie, u=ut, **kw_ex)
        elif rules is not None:
            ops.decode_next_rules(lg, pk.emb, ids, pos, done, gen_start, xin, tokens[t], n_kept[t], logprobs[t], act, counter,
                                  u=ut, **kw_ex, **rules)
        elif ex:
            ops.decode_next_ex(lg, pk.emb, ids, pos, done, gen_start, xin, tokens[t], n_kept[t], logprobs[t], act, counter,
                               u=ut, **kw_ex)
        else:
            ops.decode_next(lg, pk.emb, ids, pos, done, xin, tokens[t], n_kept[t], act, u=ut, **kw)
        stop.queued(t, act)
        steps = t + 1
        if steps == max_new_tokens:
            break                                           # (the logits after the last token pick nothing)
        if fa is not None:
            cur_mass[0] = fa[t + 1]                         # this pass's rows pick token t + 1
        rowpass.head(eng, rowpass.layers(eng, b, attn), b.xn, lg)
    out = {"ids": ids, "n_generated": pos.to(torch.int64) - start, "steps": steps,
           "tokens": tokens[:steps].t().contiguous()}
    if fa is not None:                                      # (rows, steps, L, H, F + 2); a finished row's passes are not tokens
        live = (out["tokens"] != -1).view(B, steps, 1, 1, 1)
        out["frame_attention"] = fa[:steps].permute(2, 0, 1, 3, 4).contiguous() * live
    B0 = NP // n                                            # the samples
    if twin is not None:                                    # the positive rows; the twins hold the same tokens
        out["ids"], out["n_generated"] = out["ids"][:NP].contiguous(), out["n_generated"][:NP]
        out["n_plausible"] = n_plausible[:steps].t().contiguous()
    if return_logprobs:
        out["logprobs"] = logprobs[:steps].t().contiguous()
        out["sum_logprob"] = out["logprobs"].sum(1)
    if vote:                                                # (n >= 2: logprobs exist) the mean raw log-probability per token
        tk = out["tokens"]
        score = logprobs[:steps].t().contiguous().sum(1) / (tk != -1).sum(1).clamp(min=1).to(torch.float32)
        out["vote"] = ops.sample_vote(tk.view(B0, n, steps), score.view(B0, n))
    if n > 1:
        for k in ("ids", "n_generated", "tokens", "logprobs", "sum_logprob", "n_plausible", "frame_attention"):
            if k in out:
                out[k] = out[k].view(B0, n, *out[k].shape[1:])
    if trie is not None:
        out["choice"] = torch.as_tensor(constrain.choice_of(trie, out["tokens"]), device=dev)
    return out


def _pick_rules(min_p, no_repeat_ngram_size, min_new_tokens, max_new_tokens, stop_at_eos):
    """The keywords of the three pick rules -> None at their defaults (the entries launched as ever), else the keywords of
    ops.decode_next_rules. Needs no device."""
    if not 0 <= min_p < 1:                                  # (a NaN fails the comparison)
        raise ValueError("generate: 0 <= min_p < 1 (0: off)")
    if int(no_repeat_ngram_size) != no_repeat_ngram_size or no_repeat_ngram_size < 0:
        raise ValueError("generate: no_repeat_ngram_size >= 0 (0: off)")
    if int(min_new_tokens) != min_new_tokens or min_new_tokens < 0:
        raise ValueError("generate: min_new_tokens >= 0 (0: off)")
    if min_new_tokens > max_new_tokens:
        raise ValueError("generate: min_new_tokens <= max_new_tokens")
    if min_new_tokens > 0 and not stop_at_eos:
        raise ValueError("generate: min_new_tokens holds the EOS back: it needs stop_at_eos")
    if min_p == 0 and no_repeat_ngram_size == 0 and min_new_tokens == 0:
        return None
    return dict(min_p=float(min_p), no_repeat_ngram=int(no_repeat_ngram_size), min_new_tokens=int(min_new_tokens))


def _draws(dev, seed, max_new_tokens: int, rows: int) -> torch.Tensor:
    """The uniforms of a sampled call, (max_new_tokens, rows) fp32: ONE torch.rand from a device generator seeded with `seed`
    (None: the default generator). Row t belongs to token index t of every row, whichever step commits it."""
    gen = None
    if seed is not None:
        gen = torch.Generator(device=dev)
        gen.manual_seed(int(seed))
    return torch.rand(max_new_tokens, rows, dtype=torch.float32, device=dev, generator=gen)


# ------------------------------------------------------------------------------- several rows per sample and pass
def _draft_sampling(keyword: str, temperature, top_p, top_k, repetition_penalty, seed):
    """The sampling keywords of a draft-and-verify call -> None at temperature == 0 (the greedy entries, launched as ever), else
    the keywords of the sampled token steps (ops.spec_step_sample, ops.tree_spec_step_sample). Needs no device. The unseeded
    form (seed None: the default generator) stays refused, as every sampled draft call was: tests/test_lookahead_cpu.py and
    tests/test_treedraft_cpu.py hold it so. With a seed the call has a plain call to be set against, token for token."""
    if int(top_k) != top_k or top_k < 0 or not repetition_penalty >= 1:
        raise ValueError("generate: top_k >= 0 (0: off), repetition_penalty >= 1")
    if not temperature > 0:
        if top_k != 0 or repetition_penalty != 1:
            raise ValueError(f"generate: at temperature == 0 {keyword} verifies against the plain greedy choice: top_k and "
                             "repetition_penalty need temperature > 0 here")
        return None
    if seed is None:
        raise ValueError(f"generate: {keyword} with temperature > 0 commits the tokens of the plain sampled call with the same "
                         "seed: pass seed=")
    if not 0 < top_p <= 1:
        raise ValueError("generate: 0 < top_p <= 1")
    return dict(temperature=float(temperature), top_p=float(top_p), top_k=int(top_k),
                repetition_penalty=float(repetition_penalty))


def _pass_checks(data: dict, T: int, max_new_tokens: int, keyword: str) -> int:
    """What a loop of T rows per sample and pass refuses before it reads the batch -> B."""
    _need_prefix(data)
    if max_new_tokens < 1:
        raise ValueError("generate: max_new_tokens >= 1")
    B = data["text_id"]["vqa"].shape[0]
    if B * T > 65535:
        raise ValueError(f"generate: at most 65535 rows per pass (samples times {keyword})")
    return B


def _pass_state(eng, data: dict, T: int, max_new_tokens: int) -> types.SimpleNamespace:
    """The prefill, the buffers at B * T rows and the operands every token step of T rows per sample keeps: the first step finds
    one row per sample, the prefill's (w = -1, length = 1), in logits that are zero elsewhere."""
    p = _prefill(eng, data)
    B, dev = p.B, eng.device
    b = rowpass.buffers(eng, B * T, lg=False)
    b.lg = torch.zeros(B * T, eng.V, dtype=torch.float32, device=dev)
    b.lg.view(B, T, eng.V)[:, 0].copy_(p.first)
    i32 = dict(dtype=torch.int32, device=dev)
    return types.SimpleNamespace(
        p=p, b=b, B=B, T=T, ids=p.ids, pos=p.start.to(torch.int32), pos64=p.start.clone(), done=torch.zeros(B, **i32),
        n_gen=torch.zeros(B, **i32), at=torch.zeros(B, **i32), w=torch.full((B, T), -1, **i32), length=torch.ones(B, **i32),
        tokens=torch.full((max_new_tokens, B, T), -1, **i32), n_active=torch.zeros(max_new_tokens, **i32),
        counter=torch.zeros(1, **i32))


def _pass_loop(eng, st, max_new_tokens: int, token_step) -> dict:
    """The loop of T rows per sample and pass: the lag-one stop, token_step(t, n_active[t:t + 1]) — one launch that commits
    tokens into st.ids and writes the next pass's rows (st.b.xin), their positions (st.at) and number (st.length) —, then the
    layers with the suffix attention whose rows join the cache (ops.attn_suffix_append) and the LM head on all B * T rows.
    -> ids, n_generated, steps and tokens (B, longest row), read back from ids; st.inside marks them."""
    p, b = st.p, st.b

    def attn(i, qkv, o):
        ops.attn_suffix_append(qkv, p.ar.qkv[i], o, *eng.model.gate_views(i), p.vstart, st.at, st.length, (eng.cos, eng.sin),
                               st.B, st.T, p.S, eng.H, eng.Dh, eng.A, eng.F, cache_rotated=p.rotated)
    stop = _LagOneStop(max_new_tokens)
    steps = 0
    for t in range(max_new_tokens):
        if not stop.may_launch(t):
            break
        act = st.n_active[t:t + 1]
        token_step(t, act)
        stop.queued(t, act)
        steps = t + 1
        if steps == max_new_tokens:
            break                                           # (every row has committed at least one token per step)
        rowpass.head(eng, rowpass.layers(eng, b, attn), b.xn, b.lg)
    out, st.inside = _pass_result(eng, st.ids, p.prefix, st.n_gen, steps)
    return out


def _pass_result(eng, ids, prefix, n_gen, steps: int):
    """A stopped loop of passes -> (ids, n_generated, steps and tokens (B, longest row) read back from ids; `inside`, their mask)."""
    n_generated = n_gen.to(torch.int64)
    col = torch.arange(int(n_generated.max()), device=eng.device).unsqueeze(0)
    tokens, inside = _read_back(ids, prefix, n_generated, col)
    return {"ids": ids, "n_generated": n_generated, "steps": steps, "tokens": tokens}, inside


def _token_order(tokens, values, inside):
    """tokens, values (steps, B, T), inside (B, longest) -> (B, longest): the values at the tokens >= 0 of each row, the steps in
    order and without their padding; 0 outside."""
    steps, B, T = tokens.shape
    flat = tokens.permute(1, 0, 2).reshape(B, steps * T)
    order = (flat < 0).to(torch.int8).argsort(dim=1, stable=True)[:, :inside.shape[1]]
    v = values.permute(1, 0, 2).reshape(B, steps * T).gather(1, order)
    return torch.where(inside, v, torch.zeros_like(v))


def _draft_results(out: dict, tokens, logprobs, n_committed, n_drafted, inside, return_logprobs: bool) -> dict:
    """What draft-and-verify adds to a result: the steps' counts as (B, steps), on request the log-probabilities in token order."""
    steps = out["steps"]
    out.update({"n_committed": n_committed[:steps].t().contiguous(), "n_drafted": n_drafted[:steps].t().contiguous()})
    if return_logprobs:
        out["logprobs"] = _token_order(tokens[:steps], logprobs[:steps], inside)
        out["sum_logprob"] = out["logprobs"].sum(1)
    return out


@torch.no_grad()
def _generate_lookahead(eng, data: dict, *, T: int, G: int, draft_tokens, max_new_tokens: int, stop_at_eos: bool,
                        return_logprobs: bool, sampling=None, seed=None) -> dict:
    """generate(lookahead=T >= 2): `_pass_loop` with fvqa_spec_step as its token step (verify the pass's drafts, commit, draft the
    next pass: one launch). Rejected drafts leave k / v behind a row's position; the next pass overwrites them from its `start`
    on and reads nothing behind it. sampling (`_draft_sampling`; None: greedy, the launches of every call before the keyword
    existed): the token step is fvqa_spec_step_sample with the plain loop's draws (`_draws`), read by token index."""
    B = _pass_checks(data, T, max_new_tokens, "lookahead")
    dev = eng.device
    if draft_tokens is not None:
        draft_tokens = torch.as_tensor(draft_tokens)
        if tuple(draft_tokens.shape) != (B, int(max_new_tokens)) or draft_tokens.is_floating_point():
            raise ValueError(f"generate: draft_tokens must be integers of shape (B, max_new_tokens) = ({B}, {int(max_new_tokens)})")
        draft_tokens = draft_tokens.to(device=dev, dtype=torch.int32).contiguous()
    st = _pass_state(eng, data, T, max_new_tokens)
    logprobs = torch.zeros(max_new_tokens, B, T, dtype=torch.float32, device=dev)
    n_committed, n_drafted = (torch.zeros(max_new_tokens, B, dtype=torch.int32, device=dev) for _ in range(2))
    kw = dict(max_new_tokens=int(max_new_tokens), draft_tokens=draft_tokens, lookup_ngram=G, pos64=st.pos64,
              eos_id=eng.model.tokenizer.eos_id, stop_at_eos=stop_at_eos)

    if sampling is not None:
        u = _draws(dev, seed, int(max_new_tokens), B)
        gen_start = st.p.prefix.to(torch.int32)
        n_kept = torch.zeros(B, T, dtype=torch.int32, device=dev)

    def token_step(t, n_active):
        if sampling is None:
            ops.spec_step(st.b.lg, eng.pack.emb, st.ids, st.pos, st.done, st.n_gen, st.w, st.length, st.at, st.b.xin, st.tokens[t],
                          logprobs[t], n_committed[t], n_drafted[t], n_active, st.counter, **kw)
        else:                                               # the same step, every pick the plain sampler's
            ops.spec_step_sample(st.b.lg, eng.pack.emb, st.ids, st.pos, st.done, st.n_gen, gen_start, st.w, st.length, st.at,
                                 st.b.xin, st.tokens[t], n_kept, logprobs[t], n_committed[t], n_drafted[t], n_active, st.counter,
                                 u=u, **sampling, **kw)
    out = _pass_loop(eng, st, max_new_tokens, token_step)
    return _draft_results(out, st.tokens, logprobs, n_committed, n_drafted, st.inside, return_logprobs)


class _LagOneNarrow(_LagOneStop):
    """_LagOneStop that also carries the count of running rows still on their draft trie, by the same copy and event."""

    def __init__(self, max_steps: int):
        super().__init__(max_steps)
        self.on_trie = torch.empty(max_steps, dtype=torch.int32).pin_memory()

    def queued(self, t: int, n_active: torch.Tensor, n_on_trie: torch.Tensor) -> None:   # noqa: D102
        self.on_trie[t:t + 1].copy_(n_on_trie, non_blocking=True)
        super().queued(t, n_active)

    def off_trie(self, t: int) -> bool:
        """After may_launch(t): has the snapshot of step t - 2 shown no running row on its trie? (It never rises again.)"""
        return t >= 2 and int(self.on_trie[t - 2]) == 0


@torch.no_grad()
def _generate_tree_draft(eng, data: dict, *, R: int, draft_answers, max_new_tokens: int, stop_at_eos: bool,
                         return_logprobs: bool, sampling=None, seed=None) -> dict:
    """generate(lookahead=R, draft_answers=C): the loop of `_pass_loop` with fvqa_tree_spec_step as its token step and two kinds
    of pass. WIDE (R rows per sample): the layers with ops.attn_suffix_tree, which writes no cache row — siblings share a position
    —; every layer's raw q | k | v rows stay in a per-layer buffer (L, B * R, 3 D) — 403 MB at B = 8, R = 64, 7B in 16 bits:
    rowpass.layers is handed layer i + 1's slice by layer i's attention callback, nothing is copied —, and after the NEXT step
    ops.kv_tree_commit appends the accepted path to the cache in one launch: step, commit, layers. NARROW (one row per sample,
    from the step after a snapshot shows no running row on its trie): ops.attn_suffix_append at T = 1 and no commit, what
    lookahead's loop launches at T = 1. sampling (`_draft_sampling`; None: greedy, the launches of every call before the keyword
    existed): the token step is fvqa_tree_spec_step_sample with the plain loop's draws (`_draws`), read by token index."""
    from . import vocab
    B = _pass_checks(data, R, max_new_tokens, "lookahead")
    eos = eng.model.tokenizer.eos_id
    trie = constrain.compile_constraints(draft_answers, eos, eng.V)
    trie.roots(B)                                           # (a per-sample set built for another batch size)
    hp = vocab.plan_draft(trie, B)
    p = _prefill(eng, data)
    dev, S, V, L, D = eng.device, p.S, eng.V, eng.L, eng.D
    plan = {k: torch.as_tensor(hp[k], dtype=torch.int32).to(dev).contiguous() for k in ("n_plan", "token", "depth", "end", "parent")}
    i32 = dict(dtype=torch.int32, device=dev)
    W = ops.TREE_SPEC_WALK
    wide, narrow = rowpass.buffers(eng, B * R, lg=False), rowpass.buffers(eng, B, lg=False)
    wide.lg = torch.empty(B * R, V, dtype=torch.float32, device=dev)
    narrow.lg = p.first.to(torch.float32).contiguous().clone()   # the first step finds one row per sample: the prefill's
    qkv_all = torch.empty(L, B * R, 3 * D, dtype=eng.dtype, device=dev)
    tiles = lambda r: (r + ops.TREE_TILE - 1) // ops.TREE_TILE    # noqa: E731
    tree = {r: (torch.zeros(B * r, **i32), torch.zeros(B * r, **i32), torch.full((B * tiles(r) * ops.TREE_TILE,), -1, **i32))
            for r in (R, 1)}                                # depth, end, tile_anc of the next pass, at either width
    ids, pos, pos64 = p.ids, p.start.to(torch.int32), p.start.clone()
    done, n_gen, node, at, n_path, start_old = (torch.zeros(B, **i32) for _ in range(6))
    length = torch.ones(B, **i32)
    path = torch.zeros(B, W, **i32)
    tokens = torch.full((max_new_tokens, B, W), -1, **i32)
    logprobs = torch.zeros(max_new_tokens, B, W, dtype=torch.float32, device=dev)
    n_committed, n_drafted = (torch.zeros(max_new_tokens, B, **i32) for _ in range(2))
    n_active, n_on_trie = torch.zeros(max_new_tokens, **i32), torch.zeros(max_new_tokens, **i32)
    counter = torch.zeros(2, **i32)
    rope, gates = (eng.cos, eng.sin), eng.model.gate_views
    if sampling is not None:
        u = _draws(dev, seed, int(max_new_tokens), B)
        gen_start = p.prefix.to(torch.int32)
        n_kept = torch.zeros(B, W, **i32)

    def attn_tree(i, qkv, o):
        ops.attn_suffix_tree(qkv, p.ar.qkv[i], o, *gates(i), p.vstart, at, length, *tree[R], rope, B, R, S, eng.H, eng.Dh, eng.A,
                             eng.F, cache_rotated=p.rotated)
        wide.qkv = qkv_all[(i + 1) % L]                     # layer i + 1 projects into its own slice: the rows stay for the commit

    def attn_one(i, qkv, o):
        ops.attn_suffix_append(qkv, p.ar.qkv[i], o, *gates(i), p.vstart, at, length, rope, B, 1, S, eng.H, eng.Dh, eng.A, eng.F,
                               cache_rotated=p.rotated)
    stop = _LagOneNarrow(max_new_tokens)
    steps, fed, r_out, cur, widths = 0, 1, R, narrow, []
    for t in range(max_new_tokens):
        if not stop.may_launch(t):
            break
        if r_out > 1 and stop.off_trie(t):
            r_out = 1
        nxt = wide if r_out > 1 else narrow
        if sampling is None:
            ops.tree_spec_step(cur.lg, eng.pack.emb, plan, ids, pos, done, n_gen, node, length, at, nxt.xin, *tree[r_out], path,
                               n_path, start_old, tokens[t], logprobs[t], n_committed[t], n_drafted[t], n_active[t:t + 1],
                               n_on_trie[t:t + 1], counter, max_new_tokens=int(max_new_tokens), pos64=pos64, eos_id=eos,
                               stop_at_eos=stop_at_eos)
        else:
            ops.tree_spec_step_sample(cur.lg, eng.pack.emb, plan, ids, pos, done, n_gen, gen_start, node, length, at, nxt.xin,
                                      *tree[r_out], path, n_path, start_old, tokens[t], n_kept, logprobs[t], n_committed[t],
                                      n_drafted[t], n_active[t:t + 1], n_on_trie[t:t + 1], counter, u=u,
                                      max_new_tokens=int(max_new_tokens), pos64=pos64, eos_id=eos, stop_at_eos=stop_at_eos,
                                      **sampling)
        stop.queued(t, n_active[t:t + 1], n_on_trie[t:t + 1])
        widths.append(fed)
        steps = t + 1
        if fed > 1:                                         # the pass this step verified was a tree pass: its accepted rows
            ops.kv_tree_commit(p.ar.qkv, qkv_all, path, n_path, start_old, rope, n_seq=B, S=S, H=eng.H, Dh=eng.Dh, A=eng.A,
                               cache_rotated=p.rotated)
        if steps == max_new_tokens:
            break                                           # (every row has committed at least one token per step)
        if r_out > 1:
            wide.qkv = qkv_all[0]
        rowpass.head(eng, rowpass.layers(eng, nxt, attn_tree if r_out > 1 else attn_one), nxt.xn, nxt.lg)
        cur, fed = nxt, r_out
    out, inside = _pass_result(eng, ids, p.prefix, n_gen, steps)
    out["rows_per_pass"] = torch.as_tensor(widths, **i32)
    return _draft_results(out, tokens, logprobs, n_committed, n_drafted, inside, return_logprobs)


@torch.no_grad()
def _generate_jump(eng, data: dict, *, T: int, constraints, max_new_tokens: int, stop_at_eos: bool,
                   return_logprobs: bool) -> dict:
    """generate(constraints=C, jump_forward=T >= 2): `_pass_loop` with fvqa_trie_jump_step as its token step: pick one token on
    each row's last fed logits row, commit the tokens the trie fixes behind it, feed them all. Every row a pass feeds is a
    committed token at its own position, so nothing rejected ever enters the cache."""
    B = _pass_checks(data, T, max_new_tokens, "jump_forward")
    trie = _compiled(eng, data, constraints, stop_at_eos, max_new_tokens)
    want_lp = bool(return_logprobs)
    st = _pass_state(eng, data, T, max_new_tokens)
    dev = eng.device
    dtrie = trie.to(dev)
    node = torch.as_tensor(trie.roots(B), dtype=torch.int32).to(dev).contiguous()
    lp_pick = torch.zeros(max_new_tokens, B, dtype=torch.float32, device=dev)
    lp_fed = torch.zeros(max_new_tokens + 1, B, T, dtype=torch.float32, device=dev)
    n_committed = torch.zeros(max_new_tokens, B, dtype=torch.int32, device=dev)

    def token_step(t, n_active):
        # with log-probabilities the EOS is never chained: a row that owes some is still live when they are read
        ops.trie_jump_step(st.b.lg, eng.pack.emb, st.ids, st.pos, st.done, st.n_gen, node, st.w, st.length, st.at, st.b.xin,
                           st.tokens[t], lp_pick[t], lp_fed[t], n_committed[t], n_active, st.counter, dtrie,
                           max_new_tokens=int(max_new_tokens), chain_eos=not want_lp, want_logprobs=want_lp, pos64=st.pos64,
                           eos_id=eng.model.tokenizer.eos_id)
    out = _pass_loop(eng, st, max_new_tokens, token_step)
    steps = out["steps"]
    out["n_committed"] = n_committed[:steps].t().contiguous()
    if return_logprobs:                                     # token order: a step's pick, then its chain as the NEXT step read it
        lp = torch.cat([lp_pick[:steps].unsqueeze(2), lp_fed[1:steps + 1, :, 1:]], 2)
        out["logprobs"] = _token_order(st.tokens[:steps], lp, st.inside)
        out["sum_logprob"] = out["logprobs"].sum(1)
    out["choice"] = torch.as_tensor(constrain.choice_of(trie, out["tokens"]), device=dev)
    return out


def _twin(data: dict, contrast, alpha, beta, num_beams=1) -> dict:
    """generate's `contrast` -> the twin's feature tensors {"video" and / or "audio": ...}, after the checks that need no device."""
    if not alpha >= 0 or not 0 <= beta <= 1:
        raise ValueError("generate: contrast_alpha >= 0, 0 <= contrast_beta <= 1")
    if num_beams > 1:
        raise ValueError("generate: contrast belongs to num_beams == 1 (a contrastive beam step is not built)")
    have = [k for k in ("video", "audio") if k in data]
    if isinstance(contrast, str):
        if contrast != "blind":
            raise ValueError("generate: contrast is None, \"blind\" or a dict of replacement features")
        if not have:
            raise ValueError("generate: contrast=\"blind\" needs a batch with \"video\" or \"audio\"")
        return {k: torch.zeros_like(data[k]) for k in have}
    if not isinstance(contrast, dict) or not contrast:
        raise ValueError("generate: contrast is None, \"blind\" or a dict of replacement features")
    twin = {}
    for k, v in contrast.items():
        if k not in have:
            raise ValueError(f"generate: contrast[{k!r}]: the batch has no such features (it has {have})")
        if not torch.is_tensor(v) or tuple(v.shape) != tuple(data[k].shape):
            raise ValueError(f"generate: contrast[{k!r}] must be a tensor of the batch's own shape {tuple(data[k].shape)}")
        twin[k] = v
    return twin


def _compiled(eng, data: dict, constraints, stop_at_eos: bool, max_new_tokens: int):
    """generate's `constraints` -> the host TokenTrie, after the three checks that need no device."""
    if not stop_at_eos:
        raise ValueError("generate: constraints end an answer by its EOS: stop_at_eos=False cannot be served")
    if isinstance(constraints, constrain.TokenTrie):
        trie = constraints.host()
    else:
        trie = constrain.TokenTrie.from_sequences(constraints, eng.model.tokenizer.eos_id, eng.V)
    _need_prefix(data)
    prefix = [int(p) for p in data["prefix_index"]["vqa"]]
    S = int(data["text_id"]["vqa"].shape[2])
    trie.roots(len(prefix))                                 # (a per-sample set built for another batch size)
    longest = trie.max_len * len(prefix) if trie.shared else trie.max_len
    if max(longest) > max_new_tokens:
        raise ValueError(f"generate: an allowed answer takes {max(longest)} tokens with its EOS, max_new_tokens = {max_new_tokens}")
    for b, (p, n_tok) in enumerate(zip(prefix, longest)):
        if p + n_tok > S:
            raise ValueError(f"generate: sample {b}: an allowed answer of {n_tok} tokens (EOS included) does not fit behind "
                             f"the prompt of {p} tokens inside max_seq_len = {S}")
    return trie


_BEAM_PATH_AT_ONE = False   # (tests) send num_beams == 1 through beam_search too: K = 1 must reproduce the greedy ids


@torch.no_grad()
def beam_search(eng, data: dict, *, max_new_tokens: int = N_NEW, stop_at_eos: bool = True, num_beams: int,
                length_penalty: float = 0.0, early_stop: bool = True, constraints=None) -> dict:
    """The most likely answers under the model: K = num_beams slots per sample, every token step ranks the K * V continuations
    of a sample and keeps the K best (include/fvqa.h fvqa_beam_step states the rule; a slot's score is the fp32 sum of the
    log-probabilities of its generated tokens, the EOS included; finished slots are carried and compete with their score).
    The prompt is prefilled ONCE per sample, at B rows, as `generate` does it; its cache rows [0, prefix) and the adapter rows
    are fanned out into a cache of B * K sequences (ops.kv_beam_move) and the token loop runs `generate`'s per-layer kernel
    sequence on B * K rows. Between the LM head and the next RMSNorm: the beam step (one launch) and the move of the generated
    cache rows from parent to child slot (two launches through a scratch window, all layers at once) — no torch index kernels.
    The stop lags by one step like `generate`'s: the count that leaves the device is the number of samples whose slot 0 is not
    finished (length_penalty == 0: scores only fall and ties go to the lower slot, nothing can overtake a finished slot 0) or
    that have any unfinished slot (length_penalty != 0). The penalty only ranks the final slots: score / n_generated ** penalty,
    the lowest slot on ties; it never enters the search. early_stop=False runs all max_new_tokens steps.
    -> generate's keys for the best hypothesis, "score" (B,) fp32, "beams": {"ids" (B, K, S), "score" (B, K), "n_generated"
    (B, K), "done" (B, K)} in slot order, and per step "parents" / "step_tokens" (steps, B, K) int32 (token -1: carried).
    constraints (generate's keyword; None: nothing changes): every slot carries its trie node through ops.beam_step_trie and
    offers its allowed tokens only. The stop then always waits for every slot (as with length_penalty != 0): the slots are the
    ranking of the allowed set, and with num_beams >= the number of members the finite final slots are exactly the members.
    The results gain "choice" (B,) and "beams"["choice"] (B, K)."""
    K = int(num_beams)
    _need_prefix(data)
    if max_new_tokens < 1 or not 1 <= K <= ops.BEAMS_MAX:
        raise ValueError(f"beam_search: max_new_tokens >= 1, 1 <= num_beams <= {ops.BEAMS_MAX}")
    trie = None if constraints is None else _compiled(eng, data, constraints, stop_at_eos, max_new_tokens)
    p = _prefill(eng, data)
    pk, dev, B, S, V, rows, eos = eng.pack, eng.device, p.B, p.S, eng.V, p.rows, eng.model.tokenizer.eos_id
    N = B * K
    i32 = dict(dtype=torch.int32, device=dev)
    rep = lambda t: t.repeat_interleave(K).contiguous()  # noqa: E731  per sample -> per slot
    vstart, start = rep(p.vstart), rep(p.start)
    prefix = rep(p.prefix).to(torch.int32)
    W = min(int(max_new_tokens), S)                         # the generated rows a slot can have: the move's window
    cache = _beam_cache(eng, N, S, W)
    # fan-out: rows [0, prefix) of sample b and the adapter rows -> the K slots of b, every layer, one launch
    ops.kv_beam_move(cache["qkv"], p.ar.qkv, rep(torch.arange(B, **i32)), torch.zeros(N, **i32), prefix, S=S, A=eng.A)
    b = rowpass.buffers(eng, N)
    lg, xin = b.lg, b.xin
    lg.view(B, K, V).copy_(p.first.unsqueeze(1).expand(B, K, V))
    ids2 = [p.ids.repeat_interleave(K, 0).contiguous(), torch.empty(N, S, dtype=torch.int64, device=dev)]
    pos = start.to(torch.int32)
    pos64 = start.clone()
    score = torch.full((B, K), float("-inf"), dtype=torch.float32, device=dev)
    score[:, 0] = 0.0                                       # slot 0 is the prompt, the others are empty
    done, n_gen = torch.zeros(N, **i32), torch.zeros(N, **i32)
    parents, tokens = torch.zeros(max_new_tokens, N, **i32), torch.full((max_new_tokens, N), -1, **i32)
    n_active, counter = torch.zeros(max_new_tokens, **i32), torch.zeros(1, **i32)
    if trie is not None:                                    # every slot starts at its sample's root
        dtrie = trie.to(dev)
        node = torch.as_tensor(trie.roots(B), dtype=torch.int32).repeat_interleave(K).to(dev).contiguous()
    attn = _one_row_attn(eng, p, cache["qkv"], vstart, pos64)
    stop = _LagOneStop(max_new_tokens, early_stop)
    steps, cur = 0, 0
    for t in range(max_new_tokens):
        if not stop.may_launch(t):
            break
        act = n_active[t:t + 1]
        if trie is not None:
            ops.beam_step_trie(lg, pk.emb, ids2[cur], ids2[1 - cur], pos, score.view(N), done, n_gen, pos64, parents[t],
                               tokens[t], xin, act, counter, node, dtrie, num_beams=K, eos_id=eos, stop_at_eos=stop_at_eos,
                               count_any_live=True)
        else:
            ops.beam_step(lg, pk.emb, ids2[cur], ids2[1 - cur], pos, score.view(N), done, n_gen, pos64, parents[t], tokens[t],
                          xin, act, counter, num_beams=K, eos_id=eos, stop_at_eos=stop_at_eos,
                          count_any_live=length_penalty != 0)
        cur = 1 - cur
        stop.queued(t, act)
        steps = t + 1
        if steps == max_new_tokens:
            break                                           # (the logits after the last token pick nothing)
        # the generated rows [prefix, pos) of every slot that changed its parent follow it, in all layers (a child writes
        # its own row `pos` in the layer pass below; a carried slot's frozen row is rewritten there and read by nobody)
        if K > 1:
            ops.kv_beam_move(cache["qkv"], cache["qkv"], parents[t], prefix, pos, S=S, A=eng.A, scratch=cache["scratch"],
                             window_rows=W, group=K)
        rowpass.head(eng, rowpass.layers(eng, b, attn), b.xn, lg)
    ids = ids2[cur].view(B, K, S)
    n_gen = n_gen.view(B, K).to(torch.int64)
    if length_penalty == 0:
        best = torch.zeros(B, dtype=torch.int64, device=dev)
    else:                                                   # (argmax returns the first of equal maxima: the lowest slot)
        best = (score / n_gen.clamp(min=1).to(torch.float32) ** float(length_penalty)).argmax(1)
    n_best = n_gen[rows, best]
    col = torch.arange(steps, device=dev).unsqueeze(0)
    tok_best, _ = _read_back(ids[rows, best], p.prefix, n_best, col)
    out = {"ids": ids[rows, best].contiguous(), "n_generated": n_best, "steps": steps, "tokens": tok_best,
           "score": score[rows, best].clone(),
           "beams": {"ids": ids.clone(), "score": score.clone(), "n_generated": n_gen, "done": done.view(B, K).clone()},
           "parents": parents[:steps].view(steps, B, K).clone(), "step_tokens": tokens[:steps].view(steps, B, K).clone()}
    if trie is not None:                                    # each slot's tokens, read back from its id row
        tok_all = ids.gather(2, (p.prefix.view(B, 1, 1) + col.unsqueeze(0)).clamp(max=S - 1).expand(B, K, steps))
        tok_all = torch.where(col.unsqueeze(0) < n_gen.unsqueeze(2), tok_all, torch.full_like(tok_all, -1))
        choice = torch.as_tensor(constrain.choice_of(trie, tok_all), device=dev)
        out["beams"]["choice"] = choice
        out["choice"] = choice[rows, best]
    return out



def _beam_cache(eng, N: int, S: int, W: int) -> dict:
    """The KV cache of N = B * K sequences in fvqa_attn_decode's layout (L, N * S + A, 3 * D) and the scratch window of the
    per-token move — kept on the engine for the next call of the same geometry. Not a second training arena: no activations."""
    key = (N, S, W, eng.dtype)
    c = getattr(eng, "_beam_kv", None)
    if c is None or c["key"] != key:
        eng._beam_kv = None                                 # (the old buffers go before the new ones come)
        c = {"key": key,
             "qkv": torch.zeros(eng.L, N * S + eng.A, 3 * eng.D, dtype=eng.dtype, device=eng.device),
             "scratch": torch.empty(ops.kv_beam_move_scratch(N, W, eng.D, eng.L, eng.dtype), dtype=torch.uint8,
                                    device=eng.device)}
        eng._beam_kv = c
    return c


_CHOICE = ("(A)", "(B)", "(C)", "(D)", "(E)")
_PLACEHOLDER = "x"          # the answer the prompt is cut in front of


def question_text(question: str, options=None) -> dict:
    """The prompt text of one question as dataloader/nextqa.py writes it (q_text, and o_text when the task is not a generation
    task): the question capitalised, stripped and closed by "?", the options lettered one per line under "Choices:"."""
    q = str(question).capitalize().strip()
    if not q.endswith("?"):
        q += "?"
    o = ""
    if options:
        if len(options) > len(_CHOICE):
            raise ValueError(f"at most {len(_CHOICE)} options")
        o = "Choices: \n" + "".join(f"{_CHOICE[i]} {opt}\n" for i, opt in enumerate(options))
    return {"q_text": f"Question: {q}\n", "o_text": o, "a_text": "Answer: The answer is "}


def _features(feats, B: int, max_feats: int, dim: int) -> torch.Tensor:
    """None | (B, n, dim) | a list of B (n_b, dim) -> (B, max_feats, dim) fp32, sub-sampled / zero-padded as the readers do."""
    from dataloader.nextqa import sample_frames
    if feats is None:
        return torch.zeros(B, max_feats, dim)
    rows = [torch.as_tensor(f).float() for f in feats]
    if len(rows) != B or any(r.dim() != 2 or r.shape[1] != dim for r in rows):
        raise ValueError(f"features: one (n, {dim}) array per question")
    return torch.stack([sample_frames(r, max_feats)[0] for r in rows])


def prompt_batch(tokenizer, questions, video=None, audio=None, options=None, *, max_seq_len: int, max_feats: int) -> dict:
    """questions (a list of strings) -> a batch dict `generate` accepts, with no gold answer anywhere. Per question: the sequence
    Tokenizer.encode_vqa emits in generation mode for a placeholder answer, cut at the prefix index it returns — text_id['vqa']
    (B, 1, max_seq_len) holds the prompt and 0 from prefix_index on; video_start / prefix_index are what the reader would give;
    label['vqa'] marks the one position after the prompt (the prefill needs a scored row; its loss is not used).
    video / audio: None (zero features), a (B, n, 768 / 1024) array or a list of per-question arrays; `options`: one list of
    answer options per question (or one list for all), written into the question text as the multiple-choice reader does.
    A prompt that does not leave room for one token inside max_seq_len is a ValueError."""
    questions = list(questions)
    B = len(questions)
    if B == 0:
        raise ValueError("prompt_batch: no question")
    if options is not None and (len(options) == 0 or isinstance(options[0], str)):
        options = [list(options)] * B
    ids = torch.zeros(B, 1, max_seq_len, dtype=torch.int64)
    label = torch.zeros(B, 1, max_seq_len, dtype=torch.int64)
    vstart, prefix = [], []
    for b, q in enumerate(questions):
        t = question_text(q, None if options is None else options[b])
        text = {"q_text": t["q_text"] + t["o_text"], "o_text": "", "a_text": t["a_text"]}
        seqs, p, vs = tokenizer.encode_vqa(text=text, max_feats=max_feats, split="val", answer_mapping={0: _PLACEHOLDER},
                                           answer=0, options=[_PLACEHOLDER])
        if p > max_seq_len - 1:
            raise ValueError(f"question {b}: the prompt takes {p} tokens, max_seq_len - 1 = {max_seq_len - 1} are available")
        ids[b, 0, :p] = torch.tensor(seqs[0][:p], dtype=torch.int64).clamp_min(0)      # (frame placeholders -2 -> 0)
        label[b, 0, p] = 1
        vstart.append(vs)
        prefix.append(p)
    out = {"text_id": {"vqa": ids}, "label": {"vqa": label}, "video_start": {"vqa": vstart}, "prefix_index": {"vqa": prefix},
           "text": questions, "vid": [None] * B}
    if video is not None or audio is None:
        out["video"] = _features(video, B, max_feats, 768)
    if audio is not None:
        out["audio"] = _features(audio, B, max_feats, 1024)
    return out
