"""Drop-in `llama.model` for the Flipped-VQA training path on MI355X.

Same public surface as the reference module (reference llama/model.py:17-29 ModelArgs,
:190-365 Transformer): `Transformer(params, args)`, `forward(data, inference=False) ->
(vqa_loss, vaq_loss, qav_loss)`, the same parameter names/shapes in `state_dict()` — but the
modules here are only parameter containers. No torch arithmetic happens in this file: the
forward/backward is the kernel schedule of fvqa/step.py over libfvqa_hip.so, attached to
autograd through a single Function whose backward writes the trainable gradients.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional

import torch
from torch import nn

from fvqa.step import FlatParams, StepEngine, audio_mode
from llama.tokenizer import Tokenizer


@dataclass
class ModelArgs:  # reference llama/model.py:17-29 (same fields and defaults)
    dim: int = 512
    n_layers: int = 8
    n_heads: int = 8
    vocab_size: int = -1
    multiple_of: int = 256
    norm_eps: float = 1e-5

    max_batch_size: int = 32
    max_seq_len: int = 2048
    adapter_len: int = 10
    adapter_layer: int = 30


def swiglu_hidden(dim: int, multiple_of: int) -> int:
    """SwiGLU width rule of reference llama/model.py:134-135 with hidden_dim = 4*dim (:179)."""
    h = int(2 * (4 * dim) / 3)
    return multiple_of * ((h + multiple_of - 1) // multiple_of)


class _Weight(nn.Module):
    """Holds one `.weight` parameter (stands in for nn.Linear / nn.Embedding / RMSNorm: the
    state-dict key is `<name>.weight`, exactly as in the reference)."""

    def __init__(self, *shape, init: str = "empty"):
        super().__init__()
        w = torch.empty(*shape)
        if init == "ones":
            w.fill_(1.0)
        elif init == "normal":
            w = torch.randn(*shape, dtype=torch.float32).to(w.dtype)
        elif init == "linear":                      # nn.Linear default: U(-1/sqrt(fan_in), 1/sqrt(fan_in))
            b = 1.0 / math.sqrt(shape[-1])
            w = ((torch.rand(*shape, dtype=torch.float32) * 2 - 1) * b).to(w.dtype)
        self.weight = nn.Parameter(w)


class _Attention(nn.Module):   # parameter layout of reference llama/model.py:77-85
    def __init__(self, dim: int, n_heads: int, bias: float):
        super().__init__()
        self.wq, self.wk, self.wv, self.wo = (_Weight(dim, dim) for _ in range(4))
        self.gate1 = nn.Parameter(torch.zeros(1, n_heads, 1, 1))
        self.gate2 = nn.Parameter(torch.ones(1, n_heads, 1, 1) * -bias)


class _FeedForward(nn.Module):  # reference llama/model.py:137-139
    def __init__(self, dim: int, hidden: int):
        super().__init__()
        self.w1, self.w2, self.w3 = _Weight(hidden, dim), _Weight(dim, hidden), _Weight(hidden, dim)


class _Block(nn.Module):        # reference llama/model.py:178-182
    def __init__(self, layer_id: int, p: ModelArgs, bias: float):
        super().__init__()
        self.layer_id = layer_id
        self.attention = _Attention(p.dim, p.n_heads, bias)
        self.feed_forward = _FeedForward(p.dim, swiglu_hidden(p.dim, p.multiple_of))
        self.attention_norm = _Weight(p.dim, init="ones")
        self.ffn_norm = _Weight(p.dim, init="ones")


VIDEO_DIM, AUDIO_DIM = 768, 1024       # CLIP frame / ImageBind audio feature widths (reference llama/model.py:209-223)


class _CrossAttention(nn.Module):     # parameter layout of reference llama/model.py:145-150 (fp32, :227)
    def __init__(self, dim: int):
        super().__init__()
        self.query, self.key, self.value = (nn.Linear(dim, dim, dtype=torch.float32) for _ in range(3))


class _StepFunction(torch.autograd.Function):
    """forward: losses (3,) from the kernel schedule; backward: launches the backward schedule.

    In 'flat' gradient mode (default) the backward accumulates directly into the flat gradient
    buffer that every trainable's .grad views, and returns no per-input gradients. In 'autograd'
    mode it returns ordinary gradient tensors (for third-party wrappers that hook AccumulateGrad,
    e.g. torch DDP)."""

    @staticmethod
    def forward(ctx, model, data, *trainables):
        ctx.model = model
        return model._engine.forward(data)

    @staticmethod
    def backward(ctx, g_losses):
        model = ctx.model
        flat: FlatParams = model._flat
        if model.grad_mode == "flat":
            if not flat.grads_attached():          # optimizer.zero_grad(set_to_none=True) happened
                flat.zero_grad()
                flat.attach_grads()
            model._engine.backward(g_losses.float().contiguous(), flat)
            return (None, None) + tuple(None for _ in flat.offsets)
        keep = flat.flat_grad.clone()
        flat.zero_grad()
        model._engine.backward(g_losses.float().contiguous(), flat)
        out = tuple(flat.grad_view(n).clone() for n in flat.offsets)
        flat.flat_grad.copy_(keep)
        return (None, None) + out


def _frame_attention_kw(args) -> dict:
    """--gen_frame_attention as generate's keyword ({} without the flag: the call made before it existed)."""
    return {"frame_attention": True} if getattr(args, "gen_frame_attention", False) else {}


def _pick_rules_kw(args) -> dict:
    """--gen_no_repeat_ngram / --gen_min_new_tokens as generate's keywords ({} without them: the call made before they existed)."""
    n, m = int(getattr(args, "gen_no_repeat_ngram", 0) or 0), int(getattr(args, "gen_min_new_tokens", 0) or 0)
    return {"no_repeat_ngram_size": n, "min_new_tokens": m} if n or m else {}


def _vote_kw(args) -> dict:
    """--gen_vote N [--gen_vote_temperature T --gen_vote_top_p P] as generate's keywords ({} without the flag)."""
    n = int(getattr(args, "gen_vote", 0) or 0)
    if n < 2:
        return {}
    return {"num_return_sequences": n, "vote": True, "temperature": float(getattr(args, "gen_vote_temperature", 1.0)),
            "top_p": float(getattr(args, "gen_vote_top_p", 1.0)), "seed": int(getattr(args, "seed", 0) or 0)}


def _winner_rows(out: dict, key: str):
    """A voted result's `key` (B, n, ...) -> (B, ...): each row's winning sample."""
    t = out[key]
    w = out["vote"]["winner"].to(torch.int64).view(-1, *([1] * (t.dim() - 1))).expand(-1, 1, *t.shape[2:])
    return t.gather(1, w).squeeze(1)


def _report_frame_attention(model, out: dict, extracted) -> None:
    """A result of generate with "frame_attention": the model's `last_generation` gains it, "tokens" and attribution.summarize's
    "frame_share" / "video_mass"; every extracted answer gains its "frame_share" (F numbers) and "video_mass"."""
    if "frame_attention" not in out:
        return
    from fvqa import attribution
    s = attribution.summarize(out)
    model.last_generation.update(frame_attention=out["frame_attention"], tokens=out["tokens"], **s)
    share, total = s["frame_share"].cpu().tolist(), s["video_mass"].cpu().tolist()
    for e, f, v in zip(extracted, share, total):
        e["frame_share"], e["video_mass"] = f, v


class Transformer(nn.Module):
    def __init__(self, params: ModelArgs, args):
        super().__init__()
        params.max_feats = args.max_feats          # reference llama/model.py:193-194
        params.bias = args.bias
        self.args = args
        self.params = params
        self.vocab_size = params.vocab_size
        self.n_layers = params.n_layers
        self.max_feats = args.max_feats
        self.audio_mode = audio_mode(args)         # none | only | concat | sum | attention (reference llama/model.py:209-227)
        # --train_audio: audio_proj and the cross-attention train, ride in the flat buffer and travel with the checkpoint
        # (`concat` and the video-only model have no frozen audio part: nothing changes there)
        self.train_audio = bool(getattr(args, "train_audio", False)) and self.audio_mode in ("only", "sum", "attention")

        # --train_norm: the RMSNorm weights of the walked layers and the final norm train: fp32 masters in the flat buffer, the
        # kernels read a storage-dtype working block the step engine refreshes after every update (fvqa/step.py)
        self.train_norm = bool(getattr(args, "train_norm", False))

        self.tokenizer = Tokenizer(model_path=f"{args.llama_model_path}./tokenizer.model", args=args)
        self.eos_id = self.tokenizer.eos_id
        self.answer_token_id = self.tokenizer.a_token_id
        self.q_token_id = self.tokenizer.q_token_id

        self.tok_embeddings = _Weight(params.vocab_size, params.dim)
        self.adapter_query = _Weight(params.adapter_len * params.adapter_layer, params.dim, init="normal")
        # The front end's projections, registered in the reference's order (llama/model.py:209-227). audio_proj and the
        # cross-attention are outside the freeze policy's filter (llama_vqa.py:72): without --train_audio they stay at this
        # initialisation — nn.Linear's own rule, drawn from torch's seeded generator — in every mode, and no checkpoint of
        # trainables holds them. They are kept in fp32 whatever the storage type: the front end is fp32 arithmetic.
        f32 = dict(dtype=torch.float32)
        am = self.audio_mode
        if am in ("only", "sum"):
            self.audio_proj = nn.Linear(AUDIO_DIM, params.dim, bias=False, **f32)
        elif am == "attention":
            self.audio_proj = nn.Linear(AUDIO_DIM, VIDEO_DIM, bias=False, **f32)
        if am != "only":
            self.visual_proj = _Weight(params.dim, VIDEO_DIM + AUDIO_DIM if am == "concat" else VIDEO_DIM, init="linear")
        if am == "attention":
            self.video_audio_cross_attn = _CrossAttention(VIDEO_DIM)
        self.temporal_emb = _Weight(self.max_feats, params.dim, init="normal")
        self.adapter_len = params.adapter_len
        self.adapter_layer = params.adapter_layer
        self.layers = nn.ModuleList(_Block(i, params, args.bias) for i in range(params.n_layers))
        self.norm = _Weight(params.dim, init="ones")
        self.output = _Weight(params.vocab_size, params.dim)
        self.tau = args.tau

        self.grad_mode = "flat"
        self._engine: Optional[StepEngine] = None
        self._flat: Optional[FlatParams] = None
        self._engine_key = None

    # ---- helpers used by the step engine ----------------------------------------------------
    def rope_tables(self):
        """cos/sin of reference precompute_freqs_cis (llama/model.py:45-50,245): fp32 angles
        p * 10000^(-2i/Dh) for p < 2*max_seq_len."""
        dh = self.params.dim // self.params.n_heads
        inv = 1.0 / (10000.0 ** (torch.arange(0, dh, 2)[: dh // 2].float() / dh))
        ang = torch.outer(torch.arange(self.params.max_seq_len * 2).float(), inv).float()
        return torch.cos(ang), torch.sin(ang)

    def engine_layer_ids(self):
        return list(range(self.params.n_layers))[-self.adapter_layer:]    # llama/model.py:338

    def gate_views(self, i: int):
        li = self.engine_layer_ids()[i]
        g = self._flat.gates
        return g[li, 0], g[li, 1]

    def is_trainable(self, name: str) -> bool:
        """The freeze policy of THIS model: the reference's name filter, widened by --train_audio and --train_norm."""
        from fvqa import synth
        return synth.is_trainable(name, self.train_audio, self.engine_layer_ids() if self.train_norm else None)

    def flat_trainable_names(self):
        """The trainables FlatParams lays out ahead of the gates, in buffer order (no visual_proj in the audio-only model). With
        --train_audio the audio front end follows temporal_emb: audio_proj, then the cross-attention's query | key | value weights
        adjacent and its three biases adjacent — the fused operands of the step engine are then single ranges of the buffer."""
        names = ["adapter_query.weight"] + (["visual_proj.weight"] if hasattr(self, "visual_proj") else []) + \
            ["temporal_emb.weight"]
        if self.train_audio:
            names.append("audio_proj.weight")
            if self.audio_mode == "attention":
                names += [f"video_audio_cross_attn.{m}.{w}" for w in ("weight", "bias") for m in ("query", "key", "value")]
        if self.train_norm:         # last ahead of the gates: one contiguous (2L + 1, D) block, an | fn | the final norm
            from fvqa import synth
            names += synth.norm_train_names(self.engine_layer_ids())
        return names

    def refresh_norm_working(self):
        """--train_norm: the storage-dtype working copies of the norm weights <- their fp32 masters. Called wherever the masters
        are written: the optimizer step, a checkpoint load, the data-parallel broadcast (a no-op without the flag or before the
        engine exists — its construction makes the first copies)."""
        if self.train_norm and self._engine is not None:
            self._engine.refresh_norm()

    def trainable_parameters(self):
        return [p for p in self.parameters() if p.requires_grad]

    def ensure_engine(self):
        """Pack weights / flatten trainables on first use (after load_state_dict + .to(device))."""
        w = self.tok_embeddings.weight
        key = (w.data_ptr(), w.dtype, str(w.device), self.adapter_query.weight.data_ptr())
        if self._engine is None or self._engine_key is None or key[:3] != self._engine_key[:3]:
            # fp16 frozen weights — the reference's own storage type (llama_vqa.py:63) — stay fp16: the fp16 build of the kernels
            # (libfvqa_hip_f16.so, v_mfma_f32_16x16x32_f16) takes them as they are. (Rounds 2-4 re-rounded them to bf16 here.)
            self._flat = FlatParams(self)
            self._engine = StepEngine(self)
            w = self.tok_embeddings.weight
            self._engine_key = (w.data_ptr(), w.dtype, str(w.device), self.adapter_query.weight.data_ptr())
        return self._engine

    def flat_params(self) -> FlatParams:
        self.ensure_engine()
        return self._flat

    # ---- reference forward signature --------------------------------------------------------
    @torch.no_grad()
    def inference(self, data):
        """Greedy generation of the answer + nearest-choice matching (reference llama/model.py:367-546):
        -> (most_similar_indices (B,), extracted_answers list of dicts). KV-cached, batched: fvqa/generate.py."""
        from fvqa import generate
        eng = self.ensure_engine()
        mode = getattr(self.args, "gen_constrain", None)
        if int(getattr(self.args, "lookahead", 0) or 0) > 1 and (mode or getattr(self.args, "contrast", None)):
            raise ValueError("--lookahead verifies drafts against the greedy choice: not with --gen_constrain or --contrast")
        if getattr(self.args, "gen_frame_attention", False) and not (mode or getattr(self.args, "gen_stop_eos", False)):
            raise ValueError("--gen_frame_attention is reported by generate: it needs --gen_stop_eos or --gen_constrain")
        if getattr(self.args, "gen_frame_attention", False) and (
                int(getattr(self.args, "num_beams", 1) or 1) > 1 or getattr(self.args, "contrast", None)
                or int(getattr(self.args, "lookahead", 0) or 0) > 1 or int(getattr(self.args, "gen_jump_forward", 0) or 0) > 1):
            raise ValueError("--gen_frame_attention is served by the plain token loop: not with --num_beams > 1, --contrast, "
                             "--lookahead > 1 or --gen_jump_forward > 1")
        draft = getattr(self.args, "gen_draft", None)
        if draft:                                           # --gen_draft: greedy's tokens, a trie of likely answers as the draft
            if (mode or getattr(self.args, "contrast", None) or int(getattr(self.args, "num_beams", 1) or 1) > 1
                    or int(getattr(self.args, "gen_jump_forward", 0) or 0) > 1 or getattr(self.args, "gen_frame_attention", False)):
                raise ValueError("--gen_draft verifies a draft trie against the greedy choice: not with --gen_constrain, "
                                 "--contrast, --num_beams > 1, --gen_jump_forward > 1 or --gen_frame_attention")
            return self._drafted_inference(data, draft)
        if int(getattr(self.args, "gen_vote", 0) or 0) > 1 and (
                int(getattr(self.args, "num_beams", 1) or 1) > 1 or int(getattr(self.args, "lookahead", 0) or 0) > 1
                or int(getattr(self.args, "gen_jump_forward", 0) or 0) > 1 or getattr(self.args, "gen_frame_attention", False)):
            raise ValueError("--gen_vote draws samples in the plain token loop: not with --num_beams > 1, --lookahead > 1, "
                             "--gen_jump_forward > 1 or --gen_frame_attention")
        if mode:                                            # --gen_constrain: decode under the allowed answers
            return self._constrained_inference(data, mode)
        if int(getattr(self.args, "gen_vote", 0) or 0) > 1:     # --gen_vote N: N samples per row, the largest group's answer
            return self._voted_inference(data)
        if getattr(self.args, "contrast", None):            # --contrast blind: each token from the difference to the blind twin
            out = generate.generate(eng, data, max_new_tokens=generate.N_NEW, temperature=0.0, stop_at_eos=True,
                                    **self._contrast_kw())
            ids = out["ids"]
            best, sims, extracted = generate.match_answers(self, data, ids)
            self.last_generation = {"ids": ids, "similarities": sims, "n_plausible": out["n_plausible"]}
            return best, extracted
        if int(getattr(self.args, "lookahead", 0) or 0) > 1:    # --lookahead T: greedy's tokens, several per pass
            out = generate.generate(eng, data, max_new_tokens=generate.N_NEW, temperature=0.0, stop_at_eos=True,
                                    num_beams=int(getattr(self.args, "num_beams", 1) or 1), lookahead=int(self.args.lookahead),
                                    lookup_ngram=int(getattr(self.args, "lookup_ngram", 2) or 2))
            ids = out["ids"]
            best, sims, extracted = generate.match_answers(self, data, ids)
            self.last_generation = {"ids": ids, "similarities": sims, "n_committed": out["n_committed"],
                                    "n_drafted": out["n_drafted"]}
            return best, extracted
        out = {}
        if int(getattr(self.args, "num_beams", 1) or 1) > 1:    # --num_beams N: the most likely answer under the model
            out = generate.generate(eng, data, max_new_tokens=generate.N_NEW, temperature=0.0, stop_at_eos=True,
                                    num_beams=int(self.args.num_beams))
            ids = out["ids"]
        elif getattr(self.args, "gen_stop_eos", False):     # --gen_stop_eos: the same tokens up to each row's EOS, which is
            out = generate.generate(eng, data, max_new_tokens=generate.N_NEW, temperature=0.0, stop_at_eos=True,
                                    **_frame_attention_kw(self.args), **_pick_rules_kw(self.args))
            ids = out["ids"]                                # where both readers of the ids cut them (match_answers, engine)
        else:
            ids = generate.greedy_decode(eng, data)
        best, sims, extracted = generate.match_answers(self, data, ids)
        self.last_generation = {"ids": ids, "similarities": sims}
        _report_frame_attention(self, out, extracted)
        return best, extracted

    @torch.no_grad()
    def inference_stream(self, batches, slots, admit=None):
        """`inference` over a list of validation batches with in-flight batching (--gen_stream SLOTS; fvqa/stream.py): every row of
        every batch is a request of ONE stream of `slots` rows — plain greedy with EOS stop (--gen_stop_eos's tokens), or
        --gen_constrain options | vocab with one trie over all requests —, then `match_answers` per batch.
        -> [(most_similar_indices, extracted_answers)] per batch. `last_generation`: the last batch's, plus "steps", "n_prefills"
        and "occupancy" of the stream."""
        from fvqa import constrain, generate, stream
        eng = self.ensure_engine()
        batches = list(batches)
        for k, what in (("num_beams", 1), ("lookahead", 1), ("gen_jump_forward", 1)):
            if int(getattr(self.args, k, 0) or 0) > what:
                raise ValueError(f"--gen_stream decodes one token per row and pass: not with --{k} > {what}")
        if getattr(self.args, "contrast", None):
            raise ValueError("--gen_stream is not built for --contrast")
        mode = getattr(self.args, "gen_constrain", None)
        trie, n_new = None, generate.N_NEW
        if mode == "options":
            cons = []
            for data in batches:
                S = data["text_id"]["vqa"].shape[2]
                cons += [[o[: max(S - int(p) - 1, 0)] for o in opts]
                         for opts, p in zip(constrain.options_of(data, self.tokenizer), data["prefix_index"]["vqa"])]
            trie = constrain.TokenTrie.from_sequences(cons, self.tokenizer.eos_id, eng.V)
        elif mode == "vocab":
            path = getattr(self.args, "answer_vocab", None)
            if not path:
                raise ValueError("--gen_constrain vocab needs --answer_vocab FILE")
            trie = constrain.TokenTrie.from_sequences(constrain.encode_answers(self.tokenizer, constrain.read_answer_vocab(path)),
                                                      self.tokenizer.eos_id, eng.V)
        elif mode:
            raise ValueError(f"gen_constrain: 'options' or 'vocab', not {mode!r}")
        if trie is not None:
            n_new = max(n_new, max(trie.max_len))
        out = stream.generate_stream(eng, batches, slots=slots, admit=admit, max_new_tokens=n_new, temperature=0.0,
                                     stop_at_eos=True, constraints=trie)
        results, lo = [], 0
        for data in batches:
            hi = lo + data["text_id"]["vqa"].shape[0]
            ids = out["ids"][lo:hi].contiguous()
            best, sims, extracted = generate.match_answers(self, data, ids)
            self.last_generation = {"ids": ids, "similarities": sims}
            if trie is not None:
                choice = out["choice"][lo:hi]
                if mode == "options":
                    best = torch.where(choice >= 0, choice.to(best.dtype), best)
                self.last_generation["choice"] = choice
            results.append((best, extracted))
            lo = hi
        self.last_generation.update(steps=out["steps"], n_prefills=out["n_prefills"], occupancy=out["occupancy"])
        return results

    def _voted_inference(self, data):
        """--gen_vote N: every row decodes N samples from one prefill (seed = --seed), the vote's winner goes through the unchanged
        `match_answers`. `last_generation` gains "vote" and "vote_share" (B,), the meter validation reads with its predictions.
        With --contrast the samples are contrastive ones; --gen_constrain is `_constrained_inference`'s."""
        from fvqa import generate
        out = generate.generate(self.ensure_engine(), data, max_new_tokens=generate.N_NEW, stop_at_eos=True, **_vote_kw(self.args),
                                **self._contrast_kw(), **_pick_rules_kw(self.args))
        ids = _winner_rows(out, "ids").contiguous()
        best, sims, extracted = generate.match_answers(self, data, ids)
        self.last_generation = {"ids": ids, "similarities": sims, "vote": out["vote"], "vote_share": out["vote"]["share"]}
        return best, extracted

    def _contrast_kw(self) -> dict:
        """--contrast / --contrast_alpha / --contrast_beta as generate's keywords ({} without --contrast)."""
        c = getattr(self.args, "contrast", None)
        if not c:
            return {}
        return {"contrast": c, "contrast_alpha": float(getattr(self.args, "contrast_alpha", 1.0)),
                "contrast_beta": float(getattr(self.args, "contrast_beta", 0.1))}

    def _answer_sets(self, data, mode, eng):
        """'options': each sample's own option token sequences (an option cut off by the end of the row keeps room for its EOS);
        'vocab': the encoded answers of --answer_vocab, one list for the batch."""
        from fvqa import constrain
        if mode == "options":
            S = data["text_id"]["vqa"].shape[2]
            return [[o[: max(S - int(p) - 1, 0)] for o in opts]
                    for opts, p in zip(constrain.options_of(data, self.tokenizer), data["prefix_index"]["vqa"])]
        if mode == "vocab":
            path = getattr(self.args, "answer_vocab", None)
            if not path:
                raise ValueError("--gen_draft vocab needs --answer_vocab FILE")
            return constrain.encode_answers(self.tokenizer, constrain.read_answer_vocab(path))
        raise ValueError(f"gen_draft: 'options' or 'vocab', not {mode!r}")

    def _drafted_inference(self, data, mode):
        """--gen_draft options | vocab with --lookahead R: the validation protocol as it stands — the plain greedy tokens (up to
        each row's EOS with --gen_stop_eos, else all N_NEW), `match_answers` — with the sample's options or the answer vocabulary
        as a draft trie (generate(lookahead=R, draft_answers=...)): fewer passes, the same answers file."""
        from fvqa import constrain, generate
        eng = self.ensure_engine()
        trie = getattr(self, "_draft_vocab_trie", None) if mode == "vocab" else None
        if trie is None:
            sets = [[o for o in opts if o] for opts in self._answer_sets(data, mode, eng)] if mode == "options" else \
                self._answer_sets(data, mode, eng)
            trie = constrain.TokenTrie.from_sequences(sets, self.tokenizer.eos_id, eng.V)
            if mode == "vocab":
                self._draft_vocab_trie = trie
        out = generate.generate(eng, data, max_new_tokens=generate.N_NEW, temperature=0.0,
                                stop_at_eos=bool(getattr(self.args, "gen_stop_eos", False)), lookahead=int(self.args.lookahead),
                                draft_answers=trie)
        ids = out["ids"]
        best, sims, extracted = generate.match_answers(self, data, ids)
        self.last_generation = {"ids": ids, "similarities": sims, "n_committed": out["n_committed"],
                                "n_drafted": out["n_drafted"], "rows_per_pass": out["rows_per_pass"], "steps": out["steps"]}
        return best, extracted

    def _constrained_inference(self, data, mode):
        """--gen_constrain options | vocab: every sample decodes under its own answer options (-> best = the index of the option
        generated; a row that completed none falls back to the cosine pick) or under the shared answers of --answer_vocab (the
        cosine pick then ranks the options against an answer of that vocabulary). --num_beams applies as before; each row ends
        at its EOS. `last_generation` gains "choice". With --contrast the constrained pick is the contrastive one."""
        from fvqa import constrain, generate
        eng = self.ensure_engine()
        if mode == "options":
            S = data["text_id"]["vqa"].shape[2]             # (an option cut off by the end of the row keeps room for its EOS)
            cons = [[o[: max(S - int(p) - 1, 0)] for o in opts]
                    for opts, p in zip(constrain.options_of(data, self.tokenizer), data["prefix_index"]["vqa"])]
            trie = constrain.TokenTrie.from_sequences(cons, self.tokenizer.eos_id, eng.V)
        elif mode == "vocab":
            trie = getattr(self, "_answer_vocab_trie", None)
            if trie is None:
                path = getattr(self.args, "answer_vocab", None)
                if not path:
                    raise ValueError("--gen_constrain vocab needs --answer_vocab FILE")
                answers = constrain.read_answer_vocab(path)
                trie = constrain.TokenTrie.from_sequences(constrain.encode_answers(self.tokenizer, answers),
                                                          self.tokenizer.eos_id, eng.V)
                self._answer_vocab_trie = trie
        else:
            raise ValueError(f"gen_constrain: 'options' or 'vocab', not {mode!r}")
        jump = int(getattr(self.args, "gen_jump_forward", 0) or 0)      # --gen_jump_forward T: forced tokens without a pass of
        kw = {"jump_forward": jump} if jump > 1 else {}                 # their own (0, 1: the call made before the flag existed)
        vote = _vote_kw(self.args)                                      # --gen_vote N: the winner's choice is the prediction
        out = generate.generate(eng, data, max_new_tokens=max(generate.N_NEW, max(trie.max_len)),
                                stop_at_eos=True, num_beams=int(getattr(self.args, "num_beams", 1) or 1), constraints=trie,
                                **self._contrast_kw(), **_frame_attention_kw(self.args), **kw, **(vote or {"temperature": 0.0}))
        ids, choice = out["ids"], out["choice"]
        if vote:
            ids, choice = _winner_rows(out, "ids").contiguous(), _winner_rows(out, "choice")
        best, sims, extracted = generate.match_answers(self, data, ids)
        if mode == "options":
            best = torch.where(choice >= 0, choice.to(best.dtype), best)
        self.last_generation = {"ids": ids, "similarities": sims, "choice": choice}
        if vote:
            self.last_generation.update(vote=out["vote"], vote_share=out["vote"]["share"])
        if jump > 1:
            self.last_generation["n_committed"] = out["n_committed"]
        _report_frame_attention(self, out, extracted)
        return best, extracted

    @torch.no_grad()
    def generate(self, data, **kw):
        """The generation API on a batch of `fvqa.generate.prompt_batch` (or a validation batch): fvqa.generate.generate's
        keywords (max_new_tokens, temperature, top_p, stop_at_eos, seed, num_beams, length_penalty, top_k, repetition_penalty,
        return_logprobs, num_return_sequences, constraints, contrast, contrast_alpha, contrast_beta, lookahead, lookup_ngram,
        draft_tokens, draft_answers, jump_forward, frame_attention, min_p, no_repeat_ngram_size, min_new_tokens, vote) -> one answer per row, the
        generated tokens up to (not including) the EOS: decoded text when the tokenizer has a vocabulary, else the list of token ids. The id matrix, the
        per-row counts and the number of token steps launched are left in `last_generation` (with num_beams > 1 the best
        hypothesis' and, under "score", the sum of its tokens' log-probabilities; with return_logprobs "logprobs" and
        "sum_logprob"; with constraints "choice", the index of each answer in the allowed set; with contrast "n_plausible", the
        size of the plausible set at every token step; with lookahead >= 2 "n_committed" and "n_drafted", per token step, and with draft_answers "rows_per_pass"; with jump_forward >= 2 "n_committed"; with frame_attention "frame_attention" and "tokens", what fvqa.attribution.summarize reads). num_return_sequences = n > 1: a list of n answers per row, and `last_generation` with the sample axis; with vote=True the answer of the vote's winner per row (one answer, not a list), and "vote" and "answers" (every sample's, the list above) in `last_generation`."""
        from fvqa import generate
        out = generate.generate(self.ensure_engine(), data, **kw)
        self.last_generation = {k: out[k] for k in ("ids", "n_generated", "steps", "score", "logprobs", "sum_logprob", "choice",
                                                     "n_plausible", "n_committed", "n_drafted", "rows_per_pass",
                                                     "frame_attention", "vote")
                                if k in out}
        if "frame_attention" in out:
            self.last_generation["tokens"] = out["tokens"]
        ids, n = out["ids"].cpu(), out["n_generated"].cpu()

        def answer(row):
            if self.tokenizer.eos_id in row:
                row = row[: row.index(self.tokenizer.eos_id)]
            return self.tokenizer.decode(row) if self.tokenizer.sp_model is not None else row

        answers = []
        for b, p in enumerate(data["prefix_index"]["vqa"]):
            if ids.dim() == 3:
                answers.append([answer(ids[b, k, int(p): int(p) + int(n[b, k])].tolist()) for k in range(ids.shape[1])])
            else:
                answers.append(answer(ids[b, int(p): int(p) + int(n[b])].tolist()))
        if "vote" in out:                                   # the winner's answer per row; every sample's stays in "answers"
            self.last_generation["answers"] = answers
            answers = [row[int(k)] for row, k in zip(answers, out["vote"]["winner"].cpu())]
        return answers

    @torch.no_grad()
    def generate_stream(self, batches, **kw):
        """`generate` over many requests with in-flight batching (fvqa.stream.generate_stream's keywords: slots, admit,
        max_new_tokens — an int or one per request —, temperature, top_p, top_k, repetition_penalty, return_logprobs, constraints,
        stop_at_eos, seed): `batches` is one batch of `prompt_batch` / a validation batch or a list of them, their rows are the
        requests, and a finished row hands its slot of the decode batch to the next request. -> one answer per request, formed as
        `generate` forms them. `last_generation`: "ids", "n_generated", "tokens", "steps", "n_prefills", "occupancy", "seated"
        (and "logprobs", "sum_logprob", "choice" where asked). ValueError: num_beams, contrast, lookahead, draft_answers,
        jump_forward and num_return_sequences are not built into the stream."""
        from fvqa import stream
        for k in ("num_beams", "contrast", "lookahead", "draft_answers", "jump_forward", "num_return_sequences"):
            if k in kw:
                raise ValueError(f"generate_stream: {k} is not built into the stream (beams, contrast, lookahead, tree drafts, "
                                 "jump-forward and several samples per prompt run through generate())")
        out = stream.generate_stream(self.ensure_engine(), batches, **kw)
        self.last_generation = {k: out[k] for k in ("ids", "n_generated", "tokens", "steps", "n_prefills", "occupancy", "seated",
                                                     "logprobs", "sum_logprob", "choice") if k in out}
        tokens, n = out["tokens"].cpu(), out["n_generated"].cpu()
        answers = []
        for r in range(tokens.shape[0]):
            row = tokens[r, : int(n[r])].tolist()
            if self.tokenizer.eos_id in row:
                row = row[: row.index(self.tokenizer.eos_id)]
            answers.append(self.tokenizer.decode(row) if self.tokenizer.sp_model is not None else row)
        return answers

    @torch.no_grad()
    def score_options(self, data, contrast=None, contrast_alpha: float = 1.0, frame_attention: bool = False):
        """The multiple-choice protocol's model half (reference llama/model_my_original_mod.py:332-377,506 with
        `inference=True`, not a generation task): -> individual_losses (B, n_options, S-1) fp32 on the device, the per-token
        cross-entropy (ignore_index 0) of every option, zero wherever a row is not scored. The reduction engine.py:86-93 makes of
        it is done on the device as well and left in `last_scoring`: prediction (B,), per-option mean and count, and the route
        that ran ("shared": the prompt once + each option's last rows; "dense": every option in full — fvqa/score.py).
        contrast ("blind", or a dict of replacement features; None: nothing changes), contrast_alpha: the batch's twin is scored
        too and the prediction is the argmin of mean+ + alpha * (mean+ - mean-); `last_scoring` gains "mean_blind",
        "prediction_blind" and "prediction_plain" (fvqa/score.py: score_options). The returned losses stay the batch's own.
        frame_attention (not with contrast): `last_scoring` gains "frame_attention" (B, n_options, T, L, H, F + 2) — where every
        suffix row of every option looked — and fvqa.attribution.summarize_options' "frame_share" (B, n_options, F) and
        "video_mass" (B, n_options)."""
        from fvqa import attribution, score
        kw = {} if contrast is None else {"contrast": contrast, "contrast_alpha": contrast_alpha}
        if frame_attention:
            kw["frame_attention"] = True
        r = score.score_options(self.ensure_engine(), data, **kw)
        self.last_scoring = {k: r[k] for k in ("prediction", "mean", "count", "route", "mean_blind", "prediction_blind",
                                               "prediction_plain", "frame_attention") if k in r}
        if "frame_attention" in r:
            self.last_scoring.update(attribution.summarize_options(r))
        return r["individual_losses"]

    @torch.no_grad()
    def score_flipped(self, data, **kw):
        """The answer options ranked by all three flipped tasks (fvqa/flipped.py: score_flipped, whose keywords these are — tasks,
        weights, route, answer, events): -> its result dict, all tensors on the device, also left in `last_scoring`: per task
        mean_t / sum_t / count_t (B, n_options) and prediction_t, total = sum_t w_t * mean_t, prediction, gold_loss (B, 3) when
        `answer` is given, route and plan per task. The token ids of "Question" / "Video" come from the model's tokenizer."""
        from fvqa import flipped
        tok = getattr(self, "tokenizer", None)
        for k, attr in (("q_token_id", "q_token_id"), ("v_token_id", "v_token_id")):
            if k not in kw and tok is not None and hasattr(tok, attr):
                kw[k] = int(getattr(tok, attr))
        self.last_scoring = flipped.score_flipped(self.ensure_engine(), data, **kw)
        return self.last_scoring

    def answer_vocab(self):
        """--answer_vocab FILE, read once: -> (the answers as text, their token sequences as they stand behind a prompt)."""
        from fvqa import constrain
        if getattr(self, "_answer_vocab", None) is None:
            path = getattr(self.args, "answer_vocab", None)
            if not path:
                raise ValueError("--val_vocab needs --answer_vocab FILE")
            answers = constrain.read_answer_vocab(path)
            self._answer_vocab = (answers, constrain.encode_answers(self.tokenizer, answers))
        return self._answer_vocab

    @torch.no_grad()
    def score_vocab(self, data, constraints, **kw):
        """Every allowed answer's exact log-probability behind the prompts of a generation batch, in one pass over the trie of
        `constraints` (fvqa/vocab.py: score_vocab, whose keywords these are — route, top, length_penalty, contrast,
        contrast_alpha, events): -> its result dict, all tensors on the device; the reductions — logprob_sum, count, mean,
        log_posterior (B, M), ranking (B, top), prediction (B,), route and, under `contrast`, mean_blind / prediction_blind /
        prediction_plain — are left in `last_scoring`."""
        from fvqa import vocab
        r = vocab.score_vocab(self.ensure_engine(), data, constraints, **kw)
        self.last_scoring = {k: v for k, v in r.items() if k not in ("edge_logprob", "plan")}
        return r

    def forward(self, data, inference=False):
        if inference:
            return self.inference(data)
        eng = self.ensure_engine()
        flat = self._flat
        named = dict(self.named_parameters())
        trainables = [named[n] for n in flat.offsets]
        if torch.is_grad_enabled() and any(p.requires_grad for p in trainables):
            losses = _StepFunction.apply(self, data, *trainables)
        else:
            losses = eng.forward(data)
        vqa_loss = losses[0]
        # tensor([0]) of a switched-off loss (llama/model.py:302), made ON the device: torch.tensor([0], device=...) is a
        # pageable host-to-device copy, which blocks the host until the stream reaches it — i.e. until the whole forward
        # has run — and the backward then starts late (C2 step: 29.7 -> 28.7 ms, profiles/r02_gemm_partition_probe.log section 7)
        zero = lambda: torch.zeros(1, dtype=torch.int64, device=losses.device)      # noqa: E731
        vaq_loss = losses[1] if self.args.vaq else zero()
        qav_loss = losses[2] if self.args.qav else zero()
        return vqa_loss, vaq_loss, qav_loss
