"""Ask a trained model one question about one clip and print its answer (the generation API: fvqa.generate.prompt_batch ->
Transformer.generate; KV-cached decode, greedy or temperature / nucleus sampling, ended by EOS).

    python answer.py --model 7B --llama_model_path ... --resume ckpt.pth --features clip.pth|.npy [--audio_features ...] \
        --question "..." [--options a b c] [--max_new_tokens 31 --temperature 0 --top_p 1 --seed 0] \
        [--num_beams N --length_penalty A] [--top_k K --repetition_penalty R --num_samples N --logprobs] \
        [--constrain | --answer_vocab FILE] [--contrast blind --contrast_alpha A --contrast_beta B] \
        [--lookahead T --lookup_ngram G] [--draft options|vocab --lookahead R] [--jump_forward T] [--frame_attention] [--json FILE]
    python answer.py ... --features clip.pth --questions FILE --slots N [--admit M]
    python answer.py ... --question "..." --answer_vocab FILE --rank N [--contrast blind]

`--answer_vocab FILE --rank N` decodes nothing: every answer of the file is scored exactly in one pass over their trie
(fvqa.vocab.score_vocab) and the N best (1 .. 8, by the mean log-probability of their tokens) are printed with their posterior.
`--constrain` (with --options) makes the answer one of the options and prints its index; `--answer_vocab FILE` (one answer per
line) makes it one of the file's answers (fvqa.generate.generate(constraints=...): decoding over a trie of the allowed answers).
`--contrast blind` (train.py's flag) picks every token from the difference to the prompt's video-blind twin — the same text with
zero features — and prints how many tokens were plausible per step (fvqa.generate.generate(contrast="blind")).
`--lookahead T` (train.py's flag) verifies a prompt-lookup draft of up to T - 1 tokens per pass and prints how many
tokens each token step committed (fvqa.generate.generate(lookahead=T)): the same answer in fewer passes.
`--draft options|vocab --lookahead R` drafts the --options, or the answers of --answer_vocab FILE, as a trie and
verifies it in one tree pass of up to R rows (fvqa.generate.generate(lookahead=R, draft_answers=...)): the plain answer,
whatever the model says, in about three passes where it is one of the drafted answers.
Both take --temperature, --top_p, --top_k and --repetition_penalty together with a --seed (required: without one they stay
refused): the answer is then the plain SAMPLED call's for the same seed, token for token (a draft is kept iff it is the token the plain sampler draws there). Not with --num_samples > 1.
`--jump_forward T` (with --constrain or --answer_vocab; greedy only) commits the tokens the trie of allowed answers fixes without
a pass of their own, up to T per step, and prints the tokens committed per step (fvqa.generate.generate(jump_forward=T)).
`--frame_attention` prints, under each answer, the weight its tokens' text softmax put on each of the clip's frame keys and their
sum, the video mass (fvqa.generate.generate(frame_attention=True), fvqa.attribution.summarize: mean over the answer's tokens, the
layers and the heads); `--json FILE` writes the answers — and those numbers — as a JSON list. Not with beams, --contrast,
--lookahead, --jump_forward or --slots.
`--min_p P`, `--no_repeat_ngram N`, `--min_new_tokens M`: three more pick rules (fvqa.generate.generate(min_p=, no_repeat_ngram_size=,
min_new_tokens=)) — sample only tokens at least P times as likely as the most likely one, never repeat an N-gram among the
generated tokens, no EOS before the M-th token. Not with beams, --constrain / --answer_vocab, --contrast, --lookahead,
--jump_forward or --slots.
`--vote` with `--num_samples N --temperature T`: self-consistency — the N samples with equal tokens form a group; each group, its
count and the winner are printed (fvqa.generate.generate(vote=True)).
`--questions FILE --slots N [--admit M]`: one question per line about the given clip, one answer per line, through in-flight
batching (fvqa.stream.generate_stream): a decode batch of N rows in which a finished answer hands its slot to the next question.
The sampling flags and --constrain / --answer_vocab apply; beams, --contrast, --lookahead, --jump_forward and --num_samples do not.

The model, audio and dtype flags are train.py's (`train.get_args_parser()`, `validate_args`). `--random_init --synthetic` runs
without LLaMA assets: the weights are closed-form, the prompt is made with a word-hash stand-in vocabulary, and the answer is
printed as token ids (a synthetic tokenizer has no vocabulary to decode with).
"""
import argparse
import copy
import re
import zlib

import numpy as np
import torch

import train
import util.misc as misc
from fvqa import constrain, generate
from llama_vqa import LLaMA_VQA


def get_args_parser():
    p = train.ArgumentParser("Flipped-VQA: answer one question (MI355X)", parents=[train.get_args_parser()])
    p.add_argument("--question", type=str, default=None)
    p.add_argument("--questions", type=str, default=None, metavar="FILE",
                   help="a file with one question per line about the given clip: answered through --slots, one answer per line")
    p.add_argument("--slots", type=int, default=0, help="with --questions: the rows of the decode batch (in-flight batching)")
    p.add_argument("--admit", type=int, default=None, help="with --slots: questions admitted per prefill, 1 .. SLOTS")
    p.add_argument("--options", type=str, nargs="*", default=None, help="answer options of a multiple-choice question")
    p.add_argument("--features", type=str, default=None, help="frame features of the clip, (n, 768): .pth or .npy")
    p.add_argument("--audio_features", type=str, default=None, help="audio features of the clip, (n, 1024): .pth or .npy")
    p.add_argument("--max_new_tokens", type=int, default=generate.N_NEW)
    p.add_argument("--temperature", type=float, default=0.0)
    p.add_argument("--top_p", type=float, default=1.0)
    p.add_argument("--length_penalty", type=float, default=0.0,
                   help="with --num_beams > 1: the final hypotheses are ranked by score / n_generated ** A (0: by score)")
    p.add_argument("--top_k", type=int, default=0, help="sample from the K most likely tokens only (0: off)")
    p.add_argument("--repetition_penalty", type=float, default=1.0,
                   help=">= 1: the logits of the tokens generated so far are divided (positive) or multiplied (negative) by it; "
                        "the prompt's tokens are not penalised")
    p.add_argument("--num_samples", type=int, default=1,
                   help="answers drawn per question from one prefill (needs --temperature > 0)")
    p.add_argument("--logprobs", action="store_true",
                   help="print each answer's log-probability under the model and its per-token geometric mean probability")
    p.add_argument("--min_p", type=float, default=0.0,
                   help="sample only tokens whose probability is at least P times the most likely token's (0: off; in [0, 1))")
    p.add_argument("--no_repeat_ngram", type=int, default=0, metavar="N",
                   help="no N-gram occurs twice among the generated tokens (0: off); the prompt is not scanned")
    p.add_argument("--min_new_tokens", type=int, default=0, metavar="M", help="the EOS is banned before the M-th token (0: off)")
    p.add_argument("--vote", action="store_true",
                   help="with --num_samples N (2 .. 64): group the samples by their tokens and print each group, its count and "
                        "the winner — the largest group, ties by the mean log-probability per token")
    p.add_argument("--constrain", action="store_true",
                   help="with --options: the answer is one of the options (constrained decoding); its index is printed")
    p.add_argument("--jump_forward", type=int, default=0,
                   help="with --constrain / --answer_vocab: up to T tokens per pass where the allowed answers leave no choice "
                        "(0, 1: off)")
    p.add_argument("--draft", type=str, choices=["options", "vocab"], default=None,
                   help="with --lookahead R (2 .. 64): draft a trie of likely answers — the --options, or the answers of "
                        "--answer_vocab — and verify it in one tree pass: the plain call's own answer, whatever it is, in fewer passes")
    p.add_argument("--frame_attention", action="store_true",
                   help="print the share of attention each frame of the clip received from the answer's tokens, and their sum")
    p.add_argument("--rank", type=int, default=0, metavar="N",
                   help="with --answer_vocab: print the N best answers of the vocabulary (1 .. 8) with their posterior — every "
                        "allowed answer is scored exactly in one pass (fvqa.vocab.score_vocab), nothing is decoded")
    p.add_argument("--json", type=str, default=None, metavar="FILE",
                   help="write the answers (with --frame_attention: frame_share and video_mass too) as a JSON list")
    p.set_defaults(max_seq_len=128, seed=None)
    return p


class WordHashVocabulary:
    """The stand-in `sp_model` of a synthetic run: words and punctuation marks hashed into the vocabulary, the prompt markers the
    layouts look for ("Video", "Question", "Answer", newline) at LLaMA's ids."""
    FIXED = {"Video": 15167, "Question": 16492, "Answer": 22550, "\n": 13}

    def __init__(self, n_words: int):
        self.n_words = n_words

    def encode(self, s: str):
        out = []
        for w in re.findall(r"\w+|[^\w\s]|\n", s):
            t = self.FIXED.get(w)
            if t is None or t >= self.n_words:
                t = 3 + zlib.crc32(w.encode()) % (self.n_words - 3)
                while t in self.FIXED.values():
                    t = 3 + (t - 2) % (self.n_words - 3)
            out.append(t)
        return out


def load_features(path, dim: int):
    """(n, dim) fp32 from a .npy array or a torch file holding a tensor."""
    if path is None:
        return None
    feats = torch.from_numpy(np.load(path)) if str(path).endswith(".npy") else torch.load(path, map_location="cpu")
    feats = torch.as_tensor(feats).float()
    if feats.dim() != 2 or feats.shape[1] != dim:
        raise ValueError(f"{path}: expected (n, {dim}) features, got {tuple(feats.shape)}")
    return feats


def main(args):
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    model = LLaMA_VQA(args).to(dev).eval()
    args.eval = True
    misc.load_model(args=args, model_without_ddp=model, optimizer=None, loss_scaler=None)
    tok = model.tokenizer
    if tok.sp_model is None:                      # synthetic: no vocabulary — a stand-in makes the prompt, ids are printed
        tok = copy.copy(tok)
        tok.sp_model = WordHashVocabulary(tok.n_words)
    video = load_features(args.features, 768)
    audio = load_features(args.audio_features, 1024)
    if args.audio and audio is None:
        raise SystemExit("--audio needs --audio_features")
    questions = [args.question]
    if args.questions:
        questions = [q.strip() for q in open(args.questions) if q.strip()]
    n_q = len(questions)
    batch = generate.prompt_batch(tok, questions, video=None if video is None else [video] * n_q,
                                  audio=None if audio is None else [audio] * n_q,
                                  options=[args.options] * n_q if args.options else None,
                                  max_seq_len=args.max_seq_len, max_feats=args.max_feats)
    if args.audio_only:
        batch.pop("video", None)
    allowed = None                                # --constrain / --answer_vocab: the allowed answers, as text
    drafted = None                                # --draft: likely answers, as text (a draft, not a rule)
    if args.draft:
        drafted = list(args.options) if args.draft == "options" else constrain.read_answer_vocab(args.answer_vocab)
    elif args.constrain:
        if not args.options:
            raise SystemExit("--constrain needs --options")
        allowed = list(args.options)
    elif args.answer_vocab:
        allowed = constrain.read_answer_vocab(args.answer_vocab)
    if args.rank:                                 # the classifier over the vocabulary: the N best members with their posterior
        kw = {"contrast": args.contrast, "contrast_alpha": args.contrast_alpha} if args.contrast else {}
        r = model.score_vocab(batch, constrain.encode_answers(tok, allowed), top=args.rank, **kw)
        rank, post, mean = r["ranking"].cpu(), r["log_posterior"].exp().cpu(), r["mean"].cpu()
        records = []
        for b, q in enumerate(questions):
            best = [(int(c), float(post[b, c]), float(mean[b, c])) for c in rank[b].tolist() if c >= 0]
            if n_q > 1:
                print(q)
            for c, p, m in best:
                print(f"{p:.4f}\t{allowed[c]}\t[member {c}, mean log-probability {m:.4f}]")
            records.append({"ranking": [{"answer": allowed[c], "posterior": p} for c, p, _ in best]})
        if args.json:
            import json
            with open(args.json, "w") as f:
                json.dump(records, f)
        return records
    kw = {} if allowed is None else {"constraints": constrain.encode_answers(tok, allowed)}
    if args.contrast:
        kw.update(contrast=args.contrast, contrast_alpha=args.contrast_alpha, contrast_beta=args.contrast_beta)
    if args.questions:                            # every question of the file through one stream of --slots rows
        answers = model.generate_stream(batch, slots=args.slots, admit=args.admit, max_new_tokens=args.max_new_tokens,
                                        temperature=args.temperature, top_p=args.top_p, seed=args.seed, top_k=args.top_k,
                                        repetition_penalty=args.repetition_penalty, return_logprobs=args.logprobs, **kw)
        g = model.last_generation
        print(f"[{n_q} questions, {g['steps']} token steps, {g['n_prefills']} prefills, occupancy {g['occupancy']:.2f}]")
        for r, a in enumerate(answers):
            line = a if isinstance(a, str) else " ".join(str(t) for t in a)
            if "sum_logprob" in g:
                line += f"\t[log-probability {float(g['sum_logprob'][r]):.4f}]"
            if allowed is not None:
                c = int(g["choice"][r])
                line += f"\t[choice {c}: {allowed[c]}]" if c >= 0 else "\t[choice -1]"
            print(line)
        return answers
    if drafted is not None:
        kw.update(lookahead=args.lookahead, draft_answers=constrain.encode_answers(tok, drafted))
    elif args.lookahead > 1:
        kw.update(lookahead=args.lookahead, lookup_ngram=args.lookup_ngram)
    if args.jump_forward > 1:
        kw.update(jump_forward=args.jump_forward)
    if args.frame_attention:
        kw.update(frame_attention=True)
    if args.min_p or args.no_repeat_ngram or args.min_new_tokens:
        kw.update(min_p=args.min_p, no_repeat_ngram_size=args.no_repeat_ngram, min_new_tokens=args.min_new_tokens)
    if args.vote:
        return vote_report(model, batch, allowed, args, kw)
    answer = model.generate(batch, max_new_tokens=args.max_new_tokens, temperature=args.temperature, top_p=args.top_p,
                            seed=args.seed, num_beams=args.num_beams, length_penalty=args.length_penalty, top_k=args.top_k,
                            repetition_penalty=args.repetition_penalty, return_logprobs=args.logprobs,
                            num_return_sequences=args.num_samples, **kw)[0]
    g = model.last_generation
    many = args.num_samples > 1
    share = None
    if args.frame_attention:                      # (1[, n], F) and (1[, n]): the one question's answers
        from fvqa import attribution
        s = attribution.summarize(g)
        share, mass = s["frame_share"][0].cpu().reshape(-1, s["frame_share"].shape[-1]), s["video_mass"][0].cpu().reshape(-1)
    records = []
    for k, a in enumerate(answer if many else [answer]):
        n = int(g["n_generated"][0, k] if many else g["n_generated"][0])
        head = f"[{n} tokens, {g['steps']} steps"
        if "score" in g:
            head += f", log-probability {float(g['score'][0]):.4f}"
        if "sum_logprob" in g:
            lp = float(g["sum_logprob"][0, k] if many else g["sum_logprob"][0])
            head += f", log-probability {lp:.4f}, per-token probability {np.exp(lp / max(n, 1)):.4f}"
        if "n_plausible" in g:
            npl = (g["n_plausible"][0, k] if many else g["n_plausible"][0])[:n]
            head += f", plausible tokens per step {float(npl.float().mean()) if n else 0.0:.1f}"
        if "n_committed" in g:
            head += ", committed per step " + " ".join(str(int(c)) for c in g["n_committed"][0])
        print(head + "]")
        print(a if isinstance(a, str) else " ".join(str(t) for t in a))
        if allowed is not None:
            c = int(g["choice"][0, k] if many else g["choice"][0])
            print(f"choice {c}: {allowed[c]}" if c >= 0 else "choice -1: no allowed answer was completed")
        records.append({"answer": a})
        if share is not None:
            print("frame shares " + " ".join(f"{float(x):.4f}" for x in share[k]) + f" | video mass {float(mass[k]):.4f}")
            records[-1].update(frame_share=[float(x) for x in share[k]], video_mass=float(mass[k]))
    if args.json:
        import json
        with open(args.json, "w") as f:
            json.dump(records, f)
    return answer


def vote_report(model, batch, allowed, args, kw):
    """--vote: the samples of the one question, grouped by their tokens — each group with its count, the winner marked."""
    best = model.generate(batch, max_new_tokens=args.max_new_tokens, temperature=args.temperature, top_p=args.top_p,
                          seed=args.seed, top_k=args.top_k, repetition_penalty=args.repetition_penalty,
                          num_return_sequences=args.num_samples, vote=True, **kw)[0]
    g = model.last_generation
    v = {k: t[0].cpu() for k, t in g["vote"].items()}
    win = int(v["winner"])
    print(f"[{args.num_samples} samples, {int(v['n_groups'])} groups, {g['steps']} steps, winner's share {float(v['share']):.2f}]")
    records = []
    for k, a in enumerate(g["answers"][0]):       # a group is printed at its first sample
        if int(v["votes"][k]) == 0:
            continue
        line = f"{int(v['votes'][k])}\t" + (a if isinstance(a, str) else " ".join(str(t) for t in a))
        if allowed is not None:
            c = int(g["choice"][0, k])
            line += f"\t[choice {c}: {allowed[c]}]" if c >= 0 else "\t[choice -1]"
        print(line + ("\t<- winner" if k == win else ""))
        records.append({"answer": a, "votes": int(v["votes"][k]), "winner": k == win})
    if args.json:
        import json
        with open(args.json, "w") as f:
            json.dump(records, f)
    return best


if __name__ == "__main__":
    parser = get_args_parser()
    a = parser.parse_args()
    if (a.question is None) == (a.questions is None):
        parser.error("one of --question TEXT and --questions FILE")
    if (a.questions is not None) != (a.slots >= 1):
        parser.error("--questions FILE and --slots N come together")
    if a.rank and (not a.answer_vocab or a.constrain or not 1 <= a.rank <= 8 or a.slots >= 1):
        parser.error("--rank N (1 .. 8) ranks the answers of --answer_vocab FILE: not with --constrain or --slots")
    train.validate_args(a)
    main(a)
