#!/usr/bin/env python3
"""Generation/eval path measurement on the MI355X box: greedy decode of 31 answer tokens for
a batch of B samples with the KV-cached row-wise decode, against the same decode done the reference's way on
the same kernels (one full forward of the batch per generated token; the reference additionally runs its
forwards one sample at a time).

The generation API (fvqa.generate.generate) is measured with --generate (full length, stop_at_eos=False) or --stop_eos
(each row stops at its EOS, the batch when every row has); --val_batch_size N decodes N rows per token step; --eos_at K
puts the first EOS of every row at generated token K: the weights are the `peakedperm` closed form (token t is followed
by pi(t), fvqa.synth.vocab_permutation) and the prompt's last token is pi^{-K}(EOS) — the trajectory of
tests/test_generate_gpu.py. The rows' generated counts and the token steps launched are printed with the timing.
--num_beams N [N ...] times beam search (generate(num_beams=N, stop_at_eos=False): all 31 steps) interleaved with the greedy
`generate` of the same batch; for N > 1 also the greedy `generate` of a batch of B * N rows — the like-for-like figure, the
layer pass is the same size — and, with device events, one fvqa_beam_step and one fvqa_kv_beam_move of the loop's shapes (every
slot moving 15 generated rows: the worst case half way through an answer).
--top_k K [K ...] / --samples N [N ...] time sampling `generate(temperature=0.8, stop_at_eos=False)` with a top-k cut (and the
log-probabilities: the fvqa_decode_next_ex token step) / with N samples per prompt from one prefill, each interleaved with the
plain sampling `generate` of the same batch — for N > 1 also N calls of it, which is what the fan-out replaces.
--contrast times greedy `generate(contrast="blind", stop_at_eos=False)` — contrastive decoding runs twice the rows — interleaved
(--pairs N times, default 3) with its two comparison points: the plain greedy `generate` of the same batch (B rows) and of a
batch of 2 * B rows (the same layer pass as the pairs).
--tree_draft R [R ...] times tree-shaped draft verification, generate(lookahead=R, draft_answers=...), four arms interleaved with
the plain call in three pairs each (tree_draft_lines states them).
--temperature T [--top_p P] with --lookahead or --tree_draft times the SAMPLED arms: every call, the plain one too, samples with
seed 0, the drafts are built around the plain sampled answer, and each arm is interleaved with the plain sampled call.
--lookahead T [T ...] times draft-and-verify greedy decoding, generate(lookahead=T, stop_at_eos=False), each arm interleaved
(--pairs N times, default 3) with the same call without the keyword: the run's own answer as draft (full acceptance: the upper
bound), drafts that are all wrong (the price of the wasted rows) and prompt lookup (--lookup_ngram G) on the synthetic batch as it
is and with the first 12 answer tokens listed in the prompt, as a multiple-choice prompt lists its options. The weights are the
`peakedperm` closed form of --eos_at: the greedy tokens are decided, whatever the number of rows in a pass. Per line: ms per
batch, ms per committed token of a row, committed tokens per pass, and whether the ids are the plain call's.
--jump_forward T [T ...] times jump-forward constrained decoding, generate(constraints=C, jump_forward=T), interleaved (--pairs N
times, default 3) with the plain constrained call generate(constraints=C) on the same trie, for two kinds of C: five options per
sample (8 to 12 tokens each, two of them sharing their first two tokens and two more their first token: the options part within
their first tokens and are then fixed up to their EOS) and one shared vocabulary of 400 answers of one to three words from a
list of 60 (a trie that branches at its first depths and nowhere else). Per line: ms per batch and passes (the token steps that
committed something) of each arm, and whether the ids are the plain call's.
--stream SLOTS --admit M [M ...] times in-flight batching, fvqa.stream.generate_stream(slots=SLOTS, admit=M), on --requests N
requests (default 64) with stop_at_eos=False and per-request budgets cycling 3, 6, 12, 24 tokens, each arm interleaved (--pairs N
times, default 3) with the plain arm: generate() over the same requests in batches of SLOTS, each at its batch's largest budget —
what a rectangular batch must run. Prefills are included on both sides. Per line: ms per request, token steps, prefills and
occupancy of each arm, beside what fvqa.stream.simulate predicts, and whether every request's tokens are the plain call's.
--frame_attention times greedy generate(frame_attention=True, stop_at_eos=False) — the decode attention also writes each row's
frame-attention summary, and the prefill's rows are summarised once per call — interleaved (--pairs N times, default 3) with the
same call without the keyword; per round both arms, their ratio, and whether the ids are the same."""
import argparse
import os
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "flipped-vqa_amd"))
import torch  # noqa: E402

from fvqa import generate, synth  # noqa: E402
from llama_vqa import LLaMA_VQA  # noqa: E402


def pick_rules_lines(a, eng, b, model, timed):
    """--pick_rules: end to end, then the pick and the vote alone."""
    from fvqa import ops
    B, T, V = a.batch_size, generate.N_NEW, model.vocab_size
    tag = f"{a.model} L={eng.L} B={B} S=128 V={V} temperature=0.8 top_p=0.9"
    rules = dict(min_p=0.05, no_repeat_ngram_size=3, min_new_tokens=4)
    runs = (("plain sampled", lambda: generate.generate(eng, b, temperature=0.8, top_p=0.9, stop_at_eos=True, seed=0)),
            ("min_p=0.05 no_repeat_ngram_size=3 min_new_tokens=4",
             lambda: generate.generate(eng, b, temperature=0.8, top_p=0.9, stop_at_eos=True, seed=0, **rules)))
    for _, fn in runs:
        timed(fn, reps=1)
    for k in range(a.pairs or 3):
        t = [timed(fn, warm=0) for _, fn in runs]
        print(f"{tag} round {k}: " + " | ".join(f"{name}: {x * 1e3:7.1f} ms/batch" for (name, _), x in zip(runs, t))
              + f" | rules / plain {t[1] / t[0]:6.3f}", flush=True)
    dev, S = eng.device, 128
    gen = torch.Generator(device=dev).manual_seed(0)
    lg = 6.0 * torch.randn(B, V, device=dev, generator=gen)
    u = torch.rand(B, device=dev, generator=gen)
    ids0 = torch.randint(3, V, (B, S), device=dev, generator=gen)
    i32 = lambda *s, v=0: torch.full(s, v, dtype=torch.int32, device=dev)   # noqa: E731
    emb = eng.pack.emb

    def event_timed(fn, n=50):
        for _ in range(5):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n * 1e3

    st = dict(ids=ids0.clone(), pos=i32(B, v=90), done=i32(B), gs=i32(B, v=60), x=torch.empty(B, emb.shape[1], dtype=emb.dtype, device=dev),
              tok=i32(B), kept=i32(B), lp=torch.zeros(B, device=dev), act=i32(1), cnt=i32(1))

    def step(entry, **kw):
        def fn():
            st["pos"].fill_(90)
            st["done"].zero_()
            entry(lg, emb, st["ids"], st["pos"], st["done"], st["gs"], st["x"], st["tok"], st["kept"], st["lp"], st["act"], st["cnt"],
                  u=u, temperature=0.8, **kw)
        return fn
    for name, kw in (("top_p 0.9", dict(top_p=0.9)), ("top_k 40 penalty 1.3", dict(top_p=1.0, top_k=40, repetition_penalty=1.3))):
        t_ex = event_timed(step(ops.decode_next_ex, **kw))
        t_ru = event_timed(step(ops.decode_next_rules, min_p=0.05, no_repeat_ngram=3, min_new_tokens=4, **kw))
        t_mp = event_timed(step(ops.decode_next_rules, min_p=0.05, **kw))
        print(f"pick alone, B={B} V={V}, 31 generated ids, {name} (with two position resets per launch): decode_next_ex {t_ex:7.1f} us | "
              f"decode_next_rules min_p + n-gram 3 + minimum length {t_ru:7.1f} us | decode_next_rules min_p alone {t_mp:7.1f} us",
              flush=True)
    for n in (5, 64):
        tokens = torch.randint(3, 6, (B, n, T), device=dev, generator=gen, dtype=torch.int32)
        score = -torch.rand(B, n, device=dev, generator=gen)
        t_v = event_timed(lambda: ops.sample_vote(tokens, score))
        print(f"sample_vote, B={B} n={n} steps={T} (with its five output allocations): {t_v:7.1f} us", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="7B")
    ap.add_argument("--batch_size", type=int, default=8)
    ap.add_argument("--n_layers", type=int, default=0)
    ap.add_argument("--generate", action="store_true", help="decode through generate(stop_at_eos=False)")
    ap.add_argument("--stop_eos", action="store_true", help="decode through generate(stop_at_eos=True)")
    ap.add_argument("--val_batch_size", type=int, default=0, help="rows per token step (default: --batch_size)")
    ap.add_argument("--eos_at", type=int, nargs="*", default=[],
                    help="first EOS of every row at generated token K (peakedperm weights); several K: one line each, then the "
                         "full-length decode of the same model")
    ap.add_argument("--pairs", type=int, default=0, help="N interleaved pairs greedy_decode / generate(stop_at_eos=False)")
    ap.add_argument("--num_beams", type=int, nargs="*", default=[], help="beam search with N slots per sample; several N: a "
                                                                         "line each, interleaved with greedy generate")
    ap.add_argument("--top_k", type=int, nargs="*", default=[], help="sampling with a top-k cut; several K: a line each")
    ap.add_argument("--samples", type=int, nargs="*", default=[], help="N samples per prompt from one prefill; several N: a line "
                                                                       "each")
    ap.add_argument("--contrast", action="store_true", help="contrastive decoding against the blind twin, interleaved with greedy "
                                                            "generate at B and at 2 * B rows (--pairs rounds, default 3)")
    ap.add_argument("--lookahead", type=int, nargs="*", default=[], help="draft-and-verify decoding with up to T rows per pass; "
                                                                         "several T: three arms each, interleaved with plain generate")
    ap.add_argument("--lookup_ngram", type=int, default=2, help="--lookahead: the prompt-lookup arm's longest n-gram")
    ap.add_argument("--temperature", type=float, default=0.0, help="--lookahead / --tree_draft: > 0 times the SAMPLED arms — every "
                    "call, the plain one too, draws with this temperature, --top_p and seed 0, and the drafts are built around the "
                    "plain sampled answer")
    ap.add_argument("--top_p", type=float, default=1.0, help="--temperature: the nucleus bound")
    ap.add_argument("--tree_draft", type=int, nargs="*", default=[], help="tree-shaped draft verification with up to R rows per "
                    "pass (generate(lookahead=R, draft_answers=...)); several R: the four arms for each")
    ap.add_argument("--jump_forward", type=int, nargs="*", default=[], help="jump-forward constrained decoding with up to T rows "
                    "per pass; several T: a line per round each, interleaved with the plain constrained call")
    ap.add_argument("--stream", type=int, default=0, metavar="SLOTS", help="in-flight batching through SLOTS rows, interleaved "
                    "with generate() over batches of SLOTS")
    ap.add_argument("--admit", type=int, nargs="*", default=[], help="--stream: requests admitted per prefill; several M: an arm each")
    ap.add_argument("--requests", type=int, default=64, help="--stream: the number of requests")
    ap.add_argument("--frame_attention", action="store_true", help="generate(frame_attention=True) against the call without "
                                                                   "the keyword, interleaved (--pairs rounds, default 3)")
    ap.add_argument("--pick_rules", action="store_true", help="the plain sampled call against the same call with min_p, "
                    "no_repeat_ngram_size and min_new_tokens, interleaved (--pairs, default 3); then the pick alone — "
                    "fvqa_decode_next_rules against fvqa_decode_next_ex on B rows of the model's vocabulary — and fvqa_sample_vote "
                    "at 5 and 64 samples per prompt, event-timed")
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    if a.val_batch_size:
        a.batch_size = a.val_batch_size
    if a.stream:
        a.batch_size = a.stream
    dev = torch.device("cuda", 0)
    margs = types.SimpleNamespace(
        llama_model_path="/nonexistent/", model=a.model, max_seq_len=128, adapter_len=10, adapter_layer=32,
        max_feats=10, bias=3.5, tau=100.0, vaq=False, qav=False, audio=False, audio_only=False, audio_merge="none",
        debug=False, synthetic=True, random_init=True, dtype="bf16", accum_iter=1, weight_decay=0.14)
    kw = {}
    if a.n_layers:
        kw["n_layers"] = a.n_layers
        margs.adapter_layer = a.n_layers
    model = LLaMA_VQA(margs, **kw).to(dev).eval()
    p = model.params
    cfg = synth.SynthConfig(dim=p.dim, n_heads=p.n_heads, n_layers=p.n_layers, vocab_size=model.vocab_size,
                            max_seq_len=128, batch_size=a.batch_size, vaq=False, qav=False)
    b = synth.make_batch(cfg, seed=5)
    B = a.batch_size
    b["prefix_index"] = {"vqa": [60 + i % 32 for i in range(B)]}
    if a.eos_at or a.lookahead or a.jump_forward or a.stream or a.tree_draft:   # decided tokens: what a draft is verified against must not hang on a near tie
        import dataclasses
        from llama_vqa import fill_closed_form
        fill_closed_form(model, dataclasses.replace(cfg, max_feats=margs.max_feats, bias=margs.bias, tau=margs.tau,
                                                    adapter_len=p.adapter_len, adapter_layer=p.adapter_layer,
                                                    multiple_of=p.multiple_of, norm_eps=p.norm_eps, peaked_perm=True))
    eng = model.ensure_engine()
    last = {}

    def timed(decode, reps=a.reps, warm=2):
        for _ in range(warm):
            decode()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            decode()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / reps

    def greedy():
        generate.greedy_decode(eng, b)

    def gen(stop):
        return lambda: last.update(generate.generate(eng, b, stop_at_eos=stop))

    def line(what, t):
        ng = last["n_generated"].tolist() if last else None
        print(f"{a.model} L={p.n_layers} B={B} S=128 {what}: {t * 1e3:7.1f} ms/batch ({B / t:6.1f} samples/s)"
              + (f"; steps {last['steps']}, generated per row min {min(ng)} max {max(ng)}" if last else ""), flush=True)
        last.clear()

    if a.num_beams:
        beam_lines(a, eng, b, cfg, timed)
        return
    if a.lookahead:
        lookahead_lines(a, eng, b, timed)
        return
    if a.tree_draft:
        tree_draft_lines(a, eng, b, model, timed)
        return
    if a.jump_forward:
        jump_lines(a, eng, b, timed)
        return
    if a.stream:
        stream_lines(a, eng, cfg, timed)
        return
    if a.frame_attention:
        tag = f"{a.model} L={eng.L} B={B} S=128 greedy, {generate.N_NEW} tokens"
        out = {}
        runs = (("off", lambda: out.update(off=generate.generate(eng, b, stop_at_eos=False))),
                ("frame_attention=True", lambda: out.update(on=generate.generate(eng, b, stop_at_eos=False, frame_attention=True))))
        for _, fn in runs:
            timed(fn, reps=1)
        for k in range(a.pairs or 3):
            t = [timed(fn, warm=0) for _, fn in runs]
            print(f"{tag} round {k}: " + " | ".join(f"{name}: {x * 1e3:7.1f} ms/batch" for (name, _), x in zip(runs, t))
                  + f" | on / off {t[1] / t[0]:6.3f}, same ids: {bool(torch.equal(out['on']['ids'], out['off']['ids']))}",
                  flush=True)
        return
    if a.contrast:
        import dataclasses
        T = generate.N_NEW
        tag = f"{a.model} L={eng.L} B={B} S=128 greedy"
        wide = synth.make_batch(dataclasses.replace(cfg, batch_size=2 * B), seed=5)
        wide["prefix_index"] = {"vqa": [60 + i % 32 for i in range(2 * B)]}
        runs = (("generate, B rows", lambda: generate.generate(eng, b, stop_at_eos=False)),
                ("generate, 2B rows", lambda: generate.generate(eng, wide, stop_at_eos=False)),
                ("generate(contrast='blind'), B pairs", lambda: generate.generate(eng, b, stop_at_eos=False, contrast="blind")))
        for _, fn in runs:
            timed(fn, reps=1)
        for k in range(a.pairs or 3):
            t = [timed(fn, warm=0) for _, fn in runs]
            print(f"{tag} round {k}: " + " | ".join(f"{name}: {x * 1e3:7.1f} ms/batch" for (name, _), x in zip(runs, t))
                  + f" | contrast: {B * T / t[2]:8.1f} answer tokens/s, {t[2] / t[0]:5.2f}x B rows, {t[2] / t[1]:5.2f}x 2B rows",
                  flush=True)
        return
    if a.pick_rules:
        pick_rules_lines(a, eng, b, model, timed)
        return
    if a.top_k or a.samples:
        T = generate.N_NEW
        tag = f"{a.model} L={eng.L} B={B} S=128 temperature=0.8"
        plain = lambda **kw: generate.generate(eng, b, temperature=0.8, stop_at_eos=False, seed=0, **kw)   # noqa: E731
        for K in a.top_k:
            t_p, t_k = timed(plain), timed(lambda: plain(top_k=K, return_logprobs=True))
            print(f"{tag} sampling generate: {t_p * 1e3:7.1f} ms/batch, {B * T / t_p:8.1f} tokens/s | top_k={K} with "
                  f"log-probabilities: {t_k * 1e3:7.1f} ms/batch, {B * T / t_k:8.1f} tokens/s", flush=True)
        for N in a.samples:
            t_p, t_n = timed(plain), timed(lambda: plain(num_return_sequences=N))
            print(f"{tag} sampling generate: {t_p * 1e3:7.1f} ms/batch | {N} samples per prompt from one prefill: "
                  f"{t_n * 1e3:7.1f} ms/batch, {B * N * T / t_n:8.1f} tokens/s ({N * t_p / t_n:5.2f}x {N} calls)", flush=True)
        return
    if a.pairs:
        timed(greedy, reps=1)
        timed(gen(False), reps=1)
        for k in range(a.pairs):
            line(f"pair {k} greedy_decode", timed(greedy, warm=0))
            line(f"pair {k} generate(stop_at_eos=False)", timed(gen(False), warm=0))
        return
    if a.eos_at:
        V = model.vocab_size
        pi = synth.vocab_permutation(V)
        mul, add = int((pi[1] - pi[0]) % V), int(pi[0])
        for K in a.eos_at:
            t = model.tokenizer.eos_id
            for _ in range(K):
                t = ((t - add) * pow(mul, -1, V)) % V
            for i, pre in enumerate(b["prefix_index"]["vqa"]):
                b["text_id"]["vqa"][i, :, pre - 1] = t
            line(f"eos_at {K} generate(stop_at_eos=True)", timed(gen(True)))
        line("same model, generate(stop_at_eos=False)", timed(gen(False)))
        line("same model, greedy_decode", timed(greedy))
        return
    if a.generate or a.stop_eos:
        line(f"generate(stop_at_eos={a.stop_eos})", timed(gen(a.stop_eos)))
        return
    t_kv = timed(greedy)
    eng.lm_head_rows = "all"        # the reference's re-forward evaluates the head at every position (llama/model.py:439-447)
    with torch.no_grad():
        for _ in range(2):
            eng.forward(b)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(generate.N_NEW):
            eng.forward(b)
        torch.cuda.synchronize()
        t_full = time.perf_counter() - t0
    print(f"{a.model} B={B} S=128: 31 greedy tokens — KV-cached rows {t_kv * 1e3:7.1f} ms/batch "
          f"({B / t_kv:6.1f} samples/s); one full batched forward per token {t_full * 1e3:7.1f} ms/batch "
          f"({B / t_full:6.1f} samples/s); ratio {t_full / t_kv:.2f}x")


def device_us(fn, reps=20):
    for _ in range(3):
        fn()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(reps):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) * 1e3 / reps


def sampling_of(a):
    """--temperature / --top_p -> (the keywords every call of a sampled arm gets — the plain one too: the same seed, so the same
    draws —, the word for the lines)."""
    if not a.temperature > 0:
        return {}, "greedy"
    return dict(temperature=a.temperature, top_p=a.top_p, seed=0), f"sampled temperature={a.temperature} top_p={a.top_p} seed=0"


def lookahead_lines(a, eng, b, timed):
    B, N = a.batch_size, generate.N_NEW
    smp, word = sampling_of(a)
    tag = f"{a.model} L={eng.L} B={B} S=128 {word}"
    ref = generate.generate(eng, b, stop_at_eos=False, **smp)
    answer = ref["tokens"].to(torch.int32)
    listed = dict(b, text_id={"vqa": b["text_id"]["vqa"].clone()})              # the prompt lists the answer: last token, 12 answer
    for i, pre in enumerate(b["prefix_index"]["vqa"]):                          # tokens, one other token, then the prompt's end
        listed["text_id"]["vqa"][i, :, pre - 15] = b["text_id"]["vqa"][i, 0, pre - 1]
        listed["text_id"]["vqa"][i, :, pre - 14:pre - 2] = answer[i, :12].cpu().to(torch.int64)
        listed["text_id"]["vqa"][i, :, pre - 2] = 5
    arms = (("the answer as draft", b, dict(draft_tokens=answer)),
            ("drafts all wrong", b, dict(draft_tokens=(answer + 1) % eng.V)),
            (f"prompt lookup, n-grams up to {a.lookup_ngram}", b, dict(lookup_ngram=a.lookup_ngram)),
            (f"prompt lookup, n-grams up to {a.lookup_ngram}, 12 answer tokens listed in the prompt", listed,
             dict(lookup_ngram=a.lookup_ngram)))
    for T in a.lookahead:
        for name, data, kw in arms:
            out, base = {}, {}
            plain = lambda: base.update(generate.generate(eng, data, stop_at_eos=False, **smp))        # noqa: E731
            fn = lambda: out.update(generate.generate(eng, data, stop_at_eos=False, lookahead=T, **smp, **kw))   # noqa: E731
            timed(plain, reps=1)
            timed(fn, reps=1)
            same = bool(torch.equal(out["ids"], base["ids"]))
            passes = int((out["n_committed"].sum(0) > 0).sum())                  # (the steps that committed something)
            for k in range(a.pairs or 3):
                t_p, t_l = timed(plain, warm=0), timed(fn, warm=0)
                print(f"{tag} round {k}: generate: {t_p * 1e3:7.1f} ms/batch, {t_p / N * 1e3:6.3f} ms per committed token | "
                      f"lookahead={T}, {name}: {t_l * 1e3:7.1f} ms/batch, {t_l / N * 1e3:6.3f} ms per committed token, "
                      f"{N / passes:5.2f} tokens per pass ({passes} passes, {out['steps']} steps launched), {t_p / t_l:5.2f}x; "
                      f"ids {'equal' if same else 'DIFFER from'} the plain call's", flush=True)


def tree_draft_lines(a, eng, b, model, timed):
    """Four arms against the plain generate(stop_at_eos=True), interleaved: the model answers with ANSWER tokens and its EOS (the
    prompt's last token is set as --eos_at sets it); the drafts are five options of 8 to 12 tokens with the answer among them,
    a 329-answer vocabulary with the answer in it, five options without it, and — the yardstick — the chain lookahead=16 with
    the answer as draft_tokens."""
    import numpy as np
    ANSWER = 10
    B, V, eos = a.batch_size, eng.V, model.tokenizer.eos_id
    smp, word = sampling_of(a)
    tag = f"{a.model} L={eng.L} B={B} S=128 {word} to the EOS"
    pi = synth.vocab_permutation(V)
    mul, add = int((pi[1] - pi[0]) % V), int(pi[0])
    t = eos
    for _ in range(ANSWER + 1):                                                 # the EOS is token ANSWER + 1 of every row
        t = ((t - add) * pow(mul, -1, V)) % V
    for i, pre in enumerate(b["prefix_index"]["vqa"]):
        b["text_id"]["vqa"][i, :, pre - 1] = t
    ref = generate.generate(eng, b, stop_at_eos=True, **smp)
    rows = [[x for x in r if x >= 0 and x != eos] for r in ref["tokens"].cpu().tolist()]
    rng = np.random.default_rng(3)
    other = lambda n: [int(x) for x in rng.integers(3, V, n)]                   # noqa: E731
    options = [[r] + [other(int(rng.integers(8, 13))) for _ in range(4)] for r in rows]
    wrong = [[other(int(rng.integers(8, 13))) for _ in range(5)] for _ in rows]
    vocab329 = [[r] + [other(int(rng.integers(1, 4))) for _ in range(328)] for r in rows]
    from fvqa import constrain
    options, wrong, vocab329 = (constrain.TokenTrie.from_sequences(c, eos, V) for c in (options, wrong, vocab329))   # compiled once
    chain = torch.full((B, generate.N_NEW), -1, dtype=torch.int32)
    for i, r in enumerate(rows):
        chain[i, :len(r) + 1] = torch.tensor(r + [eos], dtype=torch.int32)
    for R in a.tree_draft:
        arms = ((f"tree R={R}, the answer among five options", dict(lookahead=R, draft_answers=options)),
                (f"tree R={R}, the answer in a vocabulary of 329", dict(lookahead=R, draft_answers=vocab329)),
                (f"tree R={R}, five options without the answer", dict(lookahead=R, draft_answers=wrong)),
                ("chain lookahead=16, the answer as draft", dict(lookahead=16, draft_tokens=chain)))
        for name, kw in arms:
            out, base = {}, {}
            plain = lambda: base.update(generate.generate(eng, b, stop_at_eos=True, **smp))            # noqa: E731
            fn = lambda: out.update(generate.generate(eng, b, stop_at_eos=True, **smp, **kw))          # noqa: E731
            timed(plain, reps=1)
            timed(fn, reps=1)
            same = bool(torch.equal(out["ids"], base["ids"]))
            width = out["rows_per_pass"].tolist() if "rows_per_pass" in out else []
            for k in range(a.pairs or 3):
                t_p, t_l = timed(plain, warm=0), timed(fn, warm=0)
                print(f"{tag} round {k}: generate: {t_p * 1e3:7.1f} ms/batch ({base['steps']} steps) | {name}: {t_l * 1e3:7.1f} "
                      f"ms/batch ({out['steps']} steps, committed per step, row 0: {out['n_committed'][0].tolist()}"
                      + (f", rows per pass {width}" if width else "") + f"), {t_p / t_l:5.2f}x; ids "
                      f"{'equal' if same else 'DIFFER from'} the plain call's", flush=True)


def stream_lines(a, eng, cfg, timed):
    import dataclasses
    from fvqa import stream
    slots, N = a.stream, a.requests
    tag = f"{a.model} L={eng.L} S=128 greedy, {N} requests, budgets 3/6/12/24"
    budgets = [(3, 6, 12, 24)[r % 4] for r in range(N)]
    batches = []
    for k in range(0, N, slots):
        n = min(slots, N - k)
        d = synth.make_batch(dataclasses.replace(cfg, batch_size=n), seed=5 + k)
        d["prefix_index"] = {"vqa": [60 + (k + i) % 32 for i in range(n)]}
        batches.append(d)
    ref, out = [], {}

    def plain():
        ref.clear()
        for k, d in enumerate(batches):
            ref.append(generate.generate(eng, d, stop_at_eos=False, max_new_tokens=max(budgets[k * slots:(k + 1) * slots])))

    timed(plain, reps=1)
    tok_plain = [row[:budgets[r]] for r, row in enumerate(sum((o["tokens"].tolist() for o in ref), []))]
    steps_plain = sum(o["steps"] for o in ref)
    for M in a.admit or [max(1, slots // 2)]:
        fn = lambda: out.update(stream.generate_stream(eng, batches, slots=slots, admit=M, max_new_tokens=budgets,   # noqa: E731
                                                       stop_at_eos=False))
        timed(fn, reps=1)
        same = [row[:budgets[r]] for r, row in enumerate(out["tokens"].tolist())] == tok_plain
        sim = stream.simulate(budgets, slots, M)
        for k in range(a.pairs or 3):
            t_p, t_s = timed(plain, warm=0), timed(fn, warm=0)
            print(f"{tag} round {k}: generate in batches of {slots}: {t_p / N * 1e3:7.2f} ms/request, {steps_plain} token steps, "
                  f"{len(batches)} prefills of {slots}, occupancy {sum(budgets) / (slots * steps_plain):.3f} | stream slots={slots} "
                  f"admit={M}: {t_s / N * 1e3:7.2f} ms/request, {out['steps']} token steps, {out['n_prefills']} prefills of {M}, "
                  f"occupancy {out['occupancy']:.3f} (simulate: {sim[0]} steps, {sim[1]} prefills), {t_p / t_s:5.2f}x; tokens "
                  f"{'equal' if same else 'DIFFER from'} the plain call's", flush=True)


def jump_lines(a, eng, b, timed):
    import numpy as np
    from fvqa.constrain import TokenTrie
    B = a.batch_size
    tag = f"{a.model} L={eng.L} B={B} S=128 greedy"
    eos = eng.model.tokenizer.eos_id
    rng = np.random.default_rng(0)
    tok = lambda n: [int(t) for t in rng.choice(np.arange(3, eng.V), size=n, replace=False)]   # noqa: E731
    options = []
    for _ in range(B):                                      # five options: 0 / 1 share two tokens, 2 / 3 one, 4 stands alone
        t = [tok(int(rng.integers(8, 13))) for _ in range(5)]
        t[1][:2], t[3][:1] = t[0][:2], t[2][:1]
        options.append(t)
    words = [tok(int(rng.integers(1, 3))) for _ in range(60)]                                   # a "word": one or two tokens
    vocab = {tuple(sum((words[int(i)] for i in rng.integers(0, 60, int(rng.integers(1, 4)))), [])) for _ in range(400)}
    tries = (("five options per sample", TokenTrie.from_sequences(options, eos, eng.V)),
             (f"a shared vocabulary of {len(vocab)} answers", TokenTrie.from_sequences([list(v) for v in sorted(vocab)], eos, eng.V)))
    for T in a.jump_forward:
        runs, outs = [], []
        for name, trie in tries:
            base, out = {}, {}
            runs.append((f"generate(constraints: {name})", lambda trie=trie, base=base: base.update(
                generate.generate(eng, b, constraints=trie))))
            runs.append((f"jump_forward={T}, {name}", lambda trie=trie, out=out: out.update(
                generate.generate(eng, b, constraints=trie, jump_forward=T))))
            outs.append((base, out))
        for _, fn in runs:
            timed(fn, reps=1)
        for k in range(a.pairs or 3):
            t = [timed(fn, warm=0) for _, fn in runs]
            parts = []
            for i, (base, out) in enumerate(outs):
                same = bool(torch.equal(out["ids"], base["ids"]) and torch.equal(out["choice"], base["choice"]))
                p_plain = int((base["tokens"] >= 0).any(0).sum())
                p_jump = int((out["n_committed"].sum(0) > 0).sum())
                parts.append(f"{runs[2 * i][0]}: {t[2 * i] * 1e3:7.1f} ms/batch, {p_plain} passes | {runs[2 * i + 1][0]}: "
                             f"{t[2 * i + 1] * 1e3:7.1f} ms/batch, {p_jump} passes ({out['steps']} steps launched), "
                             f"{t[2 * i] / t[2 * i + 1]:5.2f}x; ids and choice {'equal' if same else 'DIFFER from'} the plain call's")
            print(f"{tag} round {k}: " + " || ".join(parts), flush=True)


def beam_lines(a, eng, b, cfg, timed):
    import dataclasses
    from fvqa import ops
    B, T, dev = a.batch_size, generate.N_NEW, eng.device
    tag = f"{a.model} L={eng.L} B={B} S=128"
    for K in a.num_beams:
        t_g = timed(lambda: generate.generate(eng, b, stop_at_eos=False))
        t_b = timed(lambda: generate.generate(eng, b, stop_at_eos=False, num_beams=K))
        print(f"{tag} greedy generate: {t_g * 1e3:7.1f} ms/batch, {B * T / t_g:8.1f} tokens/s | num_beams={K}: "
              f"{t_b * 1e3:7.1f} ms/batch, {B * T / t_b:8.1f} answer tokens/s ({B * K * T / t_b:8.1f} slot tokens/s)", flush=True)
        if K == 1:
            continue
        wide = synth.make_batch(dataclasses.replace(cfg, batch_size=B * K), seed=5)
        wide["prefix_index"] = {"vqa": [60 + i % 32 for i in range(B * K)]}
        t_w = timed(lambda: generate.generate(eng, wide, stop_at_eos=False))
        N, S, V, D = B * K, 128, eng.V, eng.D
        i32 = dict(dtype=torch.int32, device=dev)
        lg = 4 * torch.randn(N, V, device=dev)
        ids = [torch.randint(3, V, (N, S), device=dev), torch.zeros(N, S, dtype=torch.int64, device=dev)]
        pos, done, ngen = torch.full((N,), 70, **i32), torch.zeros(N, **i32), torch.zeros(N, **i32)
        score, pos64 = torch.zeros(N, device=dev), torch.zeros(N, dtype=torch.int64, device=dev)
        par, tok, act, cnt = torch.zeros(N, **i32), torch.zeros(N, **i32), torch.zeros(1, **i32), torch.zeros(1, **i32)
        x = torch.empty(N, D, dtype=eng.dtype, device=dev)

        def step():
            pos.fill_(70)
            ops.beam_step(lg, eng.pack.emb, ids[0], ids[1], pos, score, done, ngen, pos64, par, tok, x, act, cnt, num_beams=K,
                          stop_at_eos=False)

        fill = device_us(lambda: pos.fill_(70))
        c = eng._beam_kv
        W = c["key"][2]
        rot = ((torch.arange(N, device=dev) + 1) % K).to(torch.int32)             # every slot takes its neighbour's rows
        lo, hi = torch.full((N,), 60, **i32), torch.full((N,), 75, **i32)
        us_step = device_us(step) - fill
        us_move = device_us(lambda: ops.kv_beam_move(c["qkv"], c["qkv"], rot, lo, hi, S=S, A=eng.A, scratch=c["scratch"],
                                                     window_rows=W, group=K))
        print(f"{tag} num_beams={K}: per token {t_b / T * 1e3:6.3f} ms against {t_w / T * 1e3:6.3f} ms of a greedy batch of "
              f"{N} rows ({t_b / t_w:5.3f}x); fvqa_beam_step {us_step:7.1f} us, fvqa_kv_beam_move (every slot, 15 rows, "
              f"{eng.L} layers, two launches) {us_move:7.1f} us", flush=True)


if __name__ == "__main__":
    main()
