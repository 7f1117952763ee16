#!/usr/bin/env python3
"""TEST INFRASTRUCTURE — generates the fixtures of the generation API (tests/test_generate_*.py) by running the REFERENCE in the
build container, the way oracle/gen_golden_eval.py and tools/gen_golden_score.py make theirs. Never imported by the product.

gen_eos_<preset>_peakedperm.npz — the reference's own `Transformer.inference` (llama/model.py:367-546) on the validation batch of
    oracle/gen_golden_eval.py with the `peakedperm` weights (LM head tied to the permutation pi = synth.vocab_permutation: token
    t is followed by pi(t)), after the prompt's token at prefix_b - 1 was replaced, in every option row of sample b, by
    pi^{-k_b}(2), k = (1, 3, 6, 12): the k_b-th generated token of sample b is then EOS (id 2). pi is affine mod V and inverts
    in closed form. The premise is ASSERTED on the reference's output (`ids_after`): the first EOS of sample b is its k_b-th
    generated token. Stored: what eval_*.npz stores, plus `eos_k`.

sampler_support.npz — rows of V = 512 logits: 24 tokens at scattered indices carry geometric probabilities r^j, the rest 1e-9
    each; logits = T log q so that softmax(logits / T) = q. Per row (r, T, top_p) and the SUPPORT observed over 50 000 draws of
    the reference's own sample_top_p(softmax(logits / T), top_p) (llama/generation.py:60-68). Asserted: every kept-set boundary
    is at least 5e-3 of mass away from top_p, the smallest kept probability is >= 1e-2 (so 50 000 draws see every kept token).

usage: gen_golden_generate.py [eos <preset> | sampler]      (no arguments: all three files)
"""
import os
import sys
import tempfile
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "flipped-vqa_amd"))
from fvqa import synth  # noqa: E402
import oracle.gen_golden as G  # noqa: E402
import oracle.gen_golden_loader as GL  # noqa: E402
from oracle.fake_sp import FakeSentencePiece  # noqa: E402

EOS = 2
EOS_K = (1, 3, 6, 12)
SAMPLER_ROWS = [(0.7, 1.0, 0.90), (0.5, 0.8, 0.95), (0.8, 1.5, 0.60), (0.6, 0.3, 0.96)]      # (r, T, top_p)
_STATE = {}


def setup():
    """Shims + the validation batch of the reference's reader in generation mode (once per process)."""
    if _STATE:
        return _STATE
    M = G.install_shims()                       # Tensor.cuda / half shims + stub tokenizer; the reference first on sys.path
    sys.modules.setdefault("pysrt", types.ModuleType("pysrt"))
    real_load = torch.load
    torch.load = lambda p, *a, **k: real_load(p, *a, **{**k, "weights_only": False}) if os.path.exists(p) else {}
    import dataloader as D
    import llama.tokenizer as T
    import pandas as pd

    g = torch.Generator().manual_seed(11)
    feats = {k: torch.randn(n, 768, generator=g) for k, n in GL.FRAMES.items()}
    tmp = tempfile.mkdtemp()
    os.makedirs(os.path.join(tmp, "data", "nextqa", "video_features"))
    rows = [r for r in GL.ROWS if len(r[1]) < 80]            # as oracle/gen_golden_eval.py: the long question runs past S
    cols = {"video": [r[0] for r in rows], "question": [r[1] for r in rows], "answer": [r[2] for r in rows],
            "type": [r[3] for r in rows]}
    for i in range(5):
        cols[f"a{i}"] = [r[4][i] for r in rows]
    pd.DataFrame(cols).to_csv(os.path.join(tmp, "data", "nextqa", "val.csv"), index=False)
    torch.save(feats, os.path.join(tmp, "data", "nextqa", "video_features", "clipvitl14.pth"))
    os.chdir(tmp)
    largs = types.SimpleNamespace(max_feats=10, max_seq_len=128, dataset="nextqa", audio=False, audio_only=False,
                                  audio_merge="none", debug=False, is_generation_task=True)
    tok = object.__new__(T.Tokenizer)
    tok.args, tok.sp_model = largs, FakeSentencePiece()
    tok.n_words, tok.bos_id, tok.eos_id, tok.pad_id = 32000, 1, 2, -1
    tok.v_token_id, tok.q_token_id, tok.a_token_id, tok.nl_id = 15167, 16492, 22550, 13
    ds = D.NextQA(args=largs, tokenizer=tok, split="val")
    _STATE.update(M=M, D=D, ds=ds)
    return _STATE


def inverse_permutation_power(V: int, t: int, k: int) -> int:
    """pi^{-k}(t) for pi(t) = (a t + c) mod V (synth.vocab_permutation), in closed form; checked against the table."""
    pi = synth.vocab_permutation(V)
    a = int((pi[1] - pi[0]) % V)
    c = int(pi[0])
    a_inv = pow(a, -1, V)
    x = t
    for _ in range(k):
        x = ((x - c) * a_inv) % V
    y = x
    for _ in range(k):
        y = int(pi[y])
    assert y == t
    return x


def run_eos(pname: str):
    st = setup()
    M, D, ds = st["M"], st["D"], st["ds"]
    V = 32000
    batch = D.batch_collate([ds[i] for i in range(4)])
    prefix = [int(p) for p in batch["prefix_index"]["vqa"]]
    for b, k in enumerate(EOS_K):
        chain = [inverse_permutation_power(V, EOS, j) for j in range(1, 36)]
        assert not set(chain) & {0, 1, 2}                     # no predecessor of EOS is pad / bos / eos
        t = inverse_permutation_power(V, EOS, k)
        batch["text_id"]["vqa"][b, :, prefix[b] - 1] = t
    cfg = synth.preset(pname, vaq=False, qav=False, vocab_size=V, max_seq_len=128, batch_size=4, peaked_perm=True)
    model, margs = G.build_reference(M, cfg)
    margs.is_generation_task = True
    model.eval()
    model.tokenizer.decode = lambda t: ""
    model.answer_token_id = getattr(model, "answer_token_id", 22550)
    sims_seen, ids_seen, margins = [], [], []
    orig = model.find_most_similar

    def spy(o, c):
        idx, sims = orig(o, c)
        sims_seen.append(sims.detach().float())
        return idx, sims

    model.find_most_similar = spy
    orig_filter = model.filter_and_process_output_tokens

    def spy_filter(vqa_ids, mask):
        ids_seen.append(vqa_ids.detach().clone())
        return orig_filter(vqa_ids, mask)

    model.filter_and_process_output_tokens = spy_filter
    orig_output = model.output.forward

    def spy_output(x):
        y = orig_output(x)
        z = y.detach().float()
        if z.dim() == 3:
            z = z.reshape(-1, z.shape[-1])
        top2 = z.topk(2, dim=-1).values
        margins.append(((top2[:, 0] - top2[:, 1]) / (z.max(dim=-1).values - z.min(dim=-1).values).clamp_min(1e-30)).min().item())
        return y

    model.output.forward = spy_output
    original = {"text_id_vqa": batch["text_id"]["vqa"].clone(), "label_vqa": batch["label"]["vqa"].clone()}
    with torch.no_grad():
        best, _ = model(batch, inference=True)
    ids_after = ids_seen[0].numpy()
    for b, k in enumerate(EOS_K):                             # the premise, on the reference's own output
        gen = ids_after[b, prefix[b]:prefix[b] + 31]
        first = int(np.flatnonzero(gen == EOS)[0]) + 1
        assert first == k, (b, k, first, gen[:14])
    out = {"best": best.numpy().astype(np.int64), "sims": sims_seen[0].numpy(), "ids_after": ids_after,
           "text_id_vqa": original["text_id_vqa"].numpy(), "label_vqa": original["label_vqa"].numpy(),
           "prefix_vqa": np.array(prefix, dtype=np.int64),
           "vstart_vqa": np.array(batch["video_start"]["vqa"], dtype=np.int64),
           "answer": batch["answer"].numpy(), "video": batch["video"].numpy(), "qtype": batch["qtype"].numpy(),
           "min_margin_per_call": np.array(margins, dtype=np.float32), "eos_k": np.array(EOS_K, dtype=np.int64)}
    path = os.path.join(ROOT, "tests", "golden", f"gen_eos_{pname}_peakedperm.npz")
    np.savez_compressed(path, **out)
    print(f"[gen_eos_{pname}_peakedperm] best {out['best']} answers {out['answer']} min margin {float(np.min(margins)):.3f} "
          f"first EOS at {EOS_K} -> {path} {os.path.getsize(path) // 1024} KiB", flush=True)
    del model


def kept_rule(q: np.ndarray, top_p: float) -> np.ndarray:
    """The kept set in fp64: order by q descending (ties: index ascending); kept iff the mass in front is <= top_p."""
    order = np.lexsort((np.arange(q.size), -q))
    front = np.cumsum(q[order]) - q[order]
    return np.sort(order[front <= top_p])


def run_sampler():
    st = setup()                                              # the reference first on sys.path
    del st
    from llama.generation import sample_top_p
    V, NP, DRAWS = 512, 24, 50000
    rng = np.random.default_rng(3)
    logits, params, supports = [], [], []
    for row, (r, T, top_p) in enumerate(SAMPLER_ROWS):
        where = np.sort(rng.choice(V, NP, replace=False))
        rng.shuffle(where)                                    # rank j sits at a scattered index
        q = np.full(V, 1e-9)
        q[where] = r ** np.arange(NP)
        q /= q.sum()
        lg = (T * np.log(q)).astype(np.float32)
        p = torch.softmax(torch.from_numpy(lg) / T, dim=-1)
        front = np.cumsum(np.sort(q)[::-1]) - np.sort(q)[::-1]
        margin = float(np.min(np.abs(front - top_p)))
        kept = kept_rule(q, top_p)
        assert margin >= 5e-3, (row, margin)
        assert q[kept].min() >= 1e-2, (row, q[kept].min())
        torch.manual_seed(100 + row)
        seen = set()
        for _ in range(DRAWS // 1000):
            seen.update(sample_top_p(p.repeat(1000, 1), top_p).flatten().tolist())
        sup = np.array(sorted(seen), dtype=np.int64)
        print(f"[sampler row {row}] (r, T, top_p) = {(r, T, top_p)}: support {sup.size} tokens, boundary margin {margin:.2e}, "
              f"smallest kept p {q[kept].min():.3f}, rule == observed: {np.array_equal(sup, kept)}", flush=True)
        pad = np.full(NP, -1, dtype=np.int64)
        pad[:sup.size] = sup
        logits.append(lg)
        params.append((r, T, top_p))
        supports.append(pad)
    path = os.path.join(ROOT, "tests", "golden", "sampler_support.npz")
    np.savez_compressed(path, logits=np.stack(logits), params=np.array(params, dtype=np.float64), support=np.stack(supports),
                        draws=np.int64(DRAWS))
    print("->", path, os.path.getsize(path) // 1024, "KiB")


def main():
    a = sys.argv[1:]
    if not a or a[0] == "sampler":
        run_sampler()
    if not a:
        for p in ("tiny", "7b_l2"):
            run_eos(p)
    elif a[0] == "eos":
        run_eos(a[1])


if __name__ == "__main__":
    main()
