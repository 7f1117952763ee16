#!/usr/bin/env python3
"""TEST INFRASTRUCTURE — generates tests/golden/vocab_tiny.npz and vocab_7b_l2_peakedperm.npz: the log-probability of every member
of an answer vocabulary behind a prompt, as the REFERENCE computes it, the way tools/gen_golden_flipped.py makes the flipped
fixtures. Needs the reference checkout. Never imported by the product.

The prompts are the first three samples of gen_eos_<preset>_peakedperm.npz (tools/gen_golden_generate.py: the reader's validation
batch in generation mode, the token at prefix_b - 1 replaced so that the chain of the `peakedperm` weights — token t is followed
by pi(t) — reaches the EOS at the k_b-th generated token, k = 1, 3, 6), cut at their prefix index as generate.prompt_batch cuts
them. Both fixtures use the peakedperm weights (LM head tied to the permutation): with the plain synthetic weights every member's
mean is log V up to noise and no prediction is decided.

The member sets, one per sample (`members` below): the chain of the sample up to its EOS — the member the model prefers: the
EMPTY member for k = 1 —, proper prefixes of it and members that leave it (shared prefixes, a member that is a proper prefix of
another), one-token members, the empty member, a duplicate; vocab_tiny also one member of 31 tokens, so that the trie has more
than 40 internal nodes and a sample spans two tiles of the tree attention.

The oracle: the fp32-shim reference model, its TRAINING forward (llama/model.py:250-365) called on one (sample, member) row at a
time — the prompt, the member's tokens, the EOS; labels on the member's tokens and the EOS — with the VQA criterion's reduction
switched to 'none', so that the forward returns the per-token losses it averages.

Stored: the prompt batch (text_id_vqa (B, 1, S), prefix_vqa, vstart_vqa, video), members (B, M, 31) int64 padded with -1 and
member_len (B, M) (tokens without the EOS), token_logprob (B, M, 32) fp32 (the member's tokens, then its EOS; 0 behind),
logprob_sum, count, mean (B, M), prediction (B,) = the argmax of the mean (lowest index on ties) and gap (B,) = (best mean -
second-best mean) / |second-best mean| over the DISTINCT members (the larger of the two magnitudes: at 7B width the chain's own
member is predicted with certainty, its mean is exactly 0): how decided the reference's own choice is.

usage: gen_golden_vocab.py [tiny | 7b_l2]       (no arguments: both fixtures, gaps printed)
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "flipped-vqa_amd"))
from fvqa import synth  # noqa: E402
import oracle.gen_golden as G  # noqa: E402

EOS, V, S, B = 2, 32000, 128, 3
NAMES = {"tiny": "vocab_tiny", "7b_l2": "vocab_7b_l2_peakedperm"}
_STATE = {}


def members(pname: str, b: int, last: int):
    """Sample b's list. `last`: the prompt's last token; chain[i] = pi^(i+1)(last)."""
    pi = synth.vocab_permutation(V)
    chain, t = [], last
    for _ in range(40):
        t = int(pi[t])
        chain.append(t)
    k = chain.index(EOS)                                     # the sample's k - 1: the chain's tokens in front of its EOS
    best = chain[:k]
    rng = np.random.default_rng(100 + b)
    free = lambda n: [int(x) for x in rng.integers(3, V, n)]           # noqa: E731
    # past the EOS the chain goes on: a member may not hold the EOS, so a member that follows the chain further is cut there
    out = [free(2), best, [], free(1), best + free(1), best[:max(k - 1, 0)] + free(2), free(1)]
    if k >= 2:
        out += [best[:1], best[:k - 1], best[:1] + free(3)]
    a = free(3)
    out += [a, a[:2], a[:2] + free(2), a[:1] + free(1)]               # a family with shared prefixes away from the chain
    if pname == "tiny":
        out.append(free(31))
        out += [free(int(n)) for n in rng.integers(1, 6, 6)]
    out.append(list(best))                                            # the duplicate (of the preferred member)
    assert all(EOS not in m and 0 not in m for m in out)
    return out


def run(pname: str):
    if "M" not in _STATE:
        _STATE["M"] = G.install_shims()
    M = _STATE["M"]
    src = dict(np.load(os.path.join(ROOT, "tests", "golden", f"gen_eos_{pname}_peakedperm.npz")))
    prefix = [int(p) for p in src["prefix_vqa"][:B]]
    vstart = [int(v) for v in src["vstart_vqa"][:B]]
    ids = torch.zeros(B, 1, S, dtype=torch.int64)
    for b in range(B):
        ids[b, 0, :prefix[b]] = torch.from_numpy(src["text_id_vqa"][b, 0, :prefix[b]])
    video = torch.from_numpy(src["video"][:B])
    sets = [members(pname, b, int(ids[b, 0, prefix[b] - 1])) for b in range(B)]
    Mx = max(len(s) for s in sets)
    cfg = synth.preset(pname, vaq=False, qav=False, vocab_size=V, max_seq_len=S, batch_size=1, peaked_perm=True)
    model, _ = G.build_reference(M, cfg)
    model.eval()
    model.vqa_criterion = torch.nn.CrossEntropyLoss(ignore_index=0, reduction="none")
    mem = np.full((B, Mx, 31), -1, dtype=np.int64)
    mlen = np.zeros((B, Mx), dtype=np.int64)
    tok_lp = np.zeros((B, Mx, 32), dtype=np.float32)
    lp_sum = np.full((B, Mx), -np.inf, dtype=np.float32)
    count = np.zeros((B, Mx), dtype=np.int64)
    mean = np.full((B, Mx), -np.inf, dtype=np.float32)
    with torch.no_grad():
        for b in range(B):
            for m, seq in enumerate(sets[b]):
                n = len(seq) + 1
                assert len(seq) <= 31 and prefix[b] + n <= S, (b, m, prefix[b], n)
                row = ids[b:b + 1].clone()
                row[0, 0, prefix[b]:prefix[b] + n] = torch.tensor(seq + [EOS])
                lab = torch.zeros_like(row)
                lab[0, 0, prefix[b]:prefix[b] + n] = row[0, 0, prefix[b]:prefix[b] + n]
                one = {"video": video[b:b + 1], "text_id": {"vqa": row, "vaq": row, "qav": row},
                       "label": {"vqa": lab, "vaq": torch.zeros_like(row), "qav": torch.full_like(row, -1)},
                       "video_start": {"vqa": [vstart[b]], "vaq": [vstart[b]]},
                       "video_index": {"qav": torch.zeros(1, 1, cfg.max_feats, dtype=torch.int64)}}
                loss = model(one)[0].float().reshape(-1)                 # (S - 1,): row t predicts token t + 1
                lp = -loss[prefix[b] - 1:prefix[b] - 1 + n].double()
                rest = loss.clone()
                rest[prefix[b] - 1:prefix[b] - 1 + n] = 0
                assert loss.numel() == S - 1 and not bool(rest.any())    # every other row is ignored
                mem[b, m, :len(seq)], mlen[b, m] = seq, len(seq)
                tok_lp[b, m, :n] = lp.float().numpy()
                lp_sum[b, m], count[b, m], mean[b, m] = float(lp.sum()), n, float(lp.sum() / n)
    pred = np.zeros(B, dtype=np.int64)
    gap = np.zeros(B, dtype=np.float32)
    for b in range(B):
        first = {}
        for m, seq in enumerate(sets[b]):
            first.setdefault(tuple(seq), m)
        cols = sorted(first.values())
        order = sorted(cols, key=lambda m: (-mean[b, m], m))
        pred[b] = order[0]
        gap[b] = (mean[b, order[0]] - mean[b, order[1]]) / abs(mean[b, order[1]])
    name = NAMES[pname]
    path = os.path.join(ROOT, "tests", "golden", name + ".npz")
    np.savez_compressed(path, text_id_vqa=ids.numpy(), prefix_vqa=np.array(prefix, dtype=np.int64),
                        vstart_vqa=np.array(vstart, dtype=np.int64), video=video.numpy(), members=mem, member_len=mlen,
                        n_listed=np.array([len(s) for s in sets], dtype=np.int64), token_logprob=tok_lp, logprob_sum=lp_sum,
                        count=count, mean=mean, prediction=pred, gap=gap, weights=np.array("peakedperm"))
    for b in range(B):
        print(f"[{name}] sample {b}: {len(sets[b])} members, prediction {pred[b]} (mean {mean[b, pred[b]]:.5f}, "
              f"{count[b, pred[b]]} tokens), gap to the second best {gap[b]:.4f}", flush=True)
    print(f"[{name}] mean range [{float(mean[np.isfinite(mean)].min()):.4f}, {float(mean.max()):.4f}] -> {path} "
          f"{os.path.getsize(path) // 1024} KiB", flush=True)
    del model


def main():
    for p in (sys.argv[1:] or ["tiny", "7b_l2"]):
        run(p)


if __name__ == "__main__":
    main()
