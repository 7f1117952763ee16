"""Constrained decoding on the GPU: the two kernels alone (fvqa_decode_next_trie, fvqa_beam_step_trie) — bit for bit against
the entries they extend when every node is -1, against the fp64 restatements of tests/test_constrained_cpu.py under a trie, on
the edges where an unallowed token could slip in — and `generate(constraints=...)` end to end on the tiny fixture of
tests/test_beam_gpu.py: against teacher-forced dense forwards of what it returns and against `score_options` on the
multiple-choice twin of the batch."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from fvqa import generate, ops, score
from fvqa.constrain import TokenTrie, options_of
from tests.test_beam_gpu import GAP, D_STEP, S_STEP, dense_logits, eos_batch, step_case, tiny  # noqa: F401  (tiny: the fixture)
from tests.test_constrained_cpu import allowed_of, beam_step_trie_ref, walk
from tests.test_generate_gpu import DEV, DTYPES, EPS, model_of, spread_u
from tests.test_sampling_cpu import penalised
from tests.test_sampling_gpu import assert_same_bits, make_emb, step_ex

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VOCABS = (509, 32000, 40003)         # ragged strided tails | the row in LDS | 4 * V > 144 KiB: recomputed
EOS = 2
NEG = float("-inf")
U_TOP = np.float32(1 - 2.0 ** -24)   # the largest float below 1


# ------------------------------------------------------------------------------------------------ the token step alone
def step_trie(logits, node, trie, *, emb=None, u=None, ids=None, pos=None, done=None, gen_start=None, S=16, D=128,
              dtype=torch.float32, counter=None, **kw):
    """tests/test_sampling_gpu.py::step_ex through the trie entry: one launch on host arrays -> dict of host arrays."""
    lg_host = np.asarray(logits, dtype=np.float32)
    lg = torch.as_tensor(lg_host, device=DEV).clone()
    B, V = lg.shape
    if emb is None:
        emb = make_emb(V, D, dtype)
    t = lambda a, dt: torch.as_tensor(np.asarray(a), dtype=dt, device=DEV).contiguous()   # noqa: E731
    ids = t(np.zeros((B, S)) if ids is None else ids, torch.int64)
    pos = t(np.full(B, 3) if pos is None else pos, torch.int32)
    done = t(np.zeros(B) if done is None else done, torch.int32)
    gs = t(np.zeros(B) if gen_start is None else gen_start, torch.int32)
    nd = t(node, torch.int32)
    x = torch.full((B, emb.shape[1]), float("nan"), dtype=emb.dtype, device=DEV)
    i32 = lambda n: torch.full((n,), -7, dtype=torch.int32, device=DEV)                  # noqa: E731
    tok, kept, act = i32(B), i32(B), i32(1)
    lp = torch.full((B,), float("nan"), dtype=torch.float32, device=DEV)
    pos64 = torch.full((B,), -7, dtype=torch.int64, device=DEV)
    if counter is None:
        counter = torch.zeros(1, dtype=torch.int32, device=DEV)
    ops.decode_next_trie(lg, emb, ids, pos, done, gs, x, tok, kept, lp, act, counter, nd, trie.to(DEV),
                         u=None if u is None else t(u, torch.float32), pos64=pos64, **kw)
    torch.cuda.synchronize()
    return {"token": tok.cpu().numpy(), "n_kept": kept.cpu().numpy(), "n_active": int(act), "ids": ids.cpu().numpy(),
            "pos": pos.cpu().numpy(), "done": done.cpu().numpy(), "x": x.cpu(), "emb": emb.cpu(), "pos64": pos64.cpu().numpy(),
            "logprob": lp.cpu().numpy(), "counter": int(counter), "logits_after": lg.cpu().numpy(), "logits": lg_host,
            "node": nd.cpu().numpy()}


def fan_trie(V, counts, seed, vocab=None):
    """One root per entry of `counts` with that many children (single-token answers, so every child is followed by the EOS
    alone). -> (trie, roots)."""
    rng = np.random.default_rng(seed)
    sets = [[[int(t)] for t in rng.choice(np.arange(3, V), size=n, replace=False)] for n in counts]
    trie = TokenTrie.from_sequences(sets, EOS, V if vocab is None else vocab)
    return trie, trie.root.tolist()


# ---- 1
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("V", VOCABS)
def test_every_node_minus_one_is_decode_next_ex_bit_for_bit(V, dtype):
    rng = np.random.default_rng(V)
    lg = (6.0 * rng.standard_normal((16, V))).astype(np.float32)
    u = rng.random(16).astype(np.float32)
    ids = rng.integers(0, V, (16, 16))
    ids[:, 1:4] = np.argsort(-lg, axis=1)[:, :3]                  # the span of the penalty holds each row's three best
    trie, _ = fan_trie(V, (1, 2, 7), 1)
    emb = make_emb(V, 36, dtype)
    for kw in (dict(temperature=0.0), dict(temperature=0.7, top_k=40, top_p=0.9, repetition_penalty=1.3)):
        kw = dict(emb=emb, ids=ids, u=u if kw["temperature"] > 0 else None, gen_start=np.full(16, 1), eos_id=EOS, **kw)
        old = step_ex(lg, **kw)
        new = step_trie(lg, np.full(16, -1), trie, **kw)
        assert_same_bits(old, new)                                # token, n_kept, ids, pos, pos64, done, logprob, x_next, n_active
        assert new["counter"] == 0 and (new["node"] == -1).all() and new["x"].dtype == dtype
        assert np.array_equal(new["logits_after"].view(np.uint32), lg.view(np.uint32))


def run_beam(c, K, dtype, emb, node=None, trie=None, count_any_live=False):
    """tests/test_beam_gpu.py::run_step, through fvqa_beam_step_trie when a trie is given."""
    N, V = c["logits"].shape
    S = c["ids"].shape[1]
    d = lambda t: t.to(DEV).contiguous()                                       # noqa: E731
    st = {k: d(c[k]) for k in ("score", "done", "pos", "ngen")}
    ids_out = torch.full((N, S), -9, dtype=torch.int64, device=DEV)
    x = torch.full((N, emb.shape[1]), float("nan"), dtype=dtype, device=DEV)
    i32 = lambda n: torch.full((n,), -7, dtype=torch.int32, device=DEV)         # noqa: E731
    parent, token, act = i32(N), i32(N), i32(1)
    pos64 = torch.full((N,), -7, dtype=torch.int64, device=DEV)
    counter = torch.zeros(1, dtype=torch.int32, device=DEV)
    kw = dict(num_beams=K, eos_id=EOS, stop_at_eos=True, count_any_live=count_any_live)
    out = {}
    if trie is None:
        ops.beam_step(d(c["logits"]), emb, d(c["ids"]), ids_out, st["pos"], st["score"], st["done"], st["ngen"], pos64, parent,
                      token, x, act, counter, **kw)
    else:
        nd = torch.as_tensor(np.asarray(node), dtype=torch.int32, device=DEV)
        ops.beam_step_trie(d(c["logits"]), emb, d(c["ids"]), ids_out, st["pos"], st["score"], st["done"], st["ngen"], pos64,
                           parent, token, x, act, counter, nd, trie.to(DEV), **kw)
        out["node"] = nd
    torch.cuda.synchronize()
    out.update({"parent": parent, "token": token, "ids": ids_out, "pos": st["pos"], "score": st["score"], "done": st["done"],
                "ngen": st["ngen"], "pos64": pos64, "x": x, "n_active": act, "counter": counter})
    return {k: v.cpu() for k, v in out.items()}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,K,V,seed", [(2, 1, 512, 4), (3, 3, 512, 5), (2, 8, 32000, 4)])
def test_every_node_minus_one_is_beam_step_bit_for_bit(B, K, V, seed, dtype):
    c, _ = step_case(B, K, V, seed)
    emb = torch.randn(V, D_STEP, generator=torch.Generator().manual_seed(1)).to(dtype).to(DEV)
    trie, _ = fan_trie(V, (1, 2, 7), 1)
    for any_live in (False, True):
        old = run_beam(c, K, dtype, emb, count_any_live=any_live)
        new = run_beam(c, K, dtype, emb, node=np.full(B * K, -1), trie=trie, count_any_live=any_live)
        for k in old:
            assert torch.equal(old[k].view(torch.uint8) if old[k].is_floating_point() else old[k],
                               new[k].view(torch.uint8) if new[k].is_floating_point() else new[k]), k
        assert int(new["counter"]) == 0 and bool((new["node"] == -1).all())


# ---- 2
def check_trie_rows(r, lg, u, T, top_k, top_p, trie, nodes, spans=None, rep=1.0):
    """Every row against the rule in fp64 (tests/test_constrained_cpu.py::kept_set_trie, spelled out so that the bounds can
    move): the token is allowed, n_kept and the token are the rule's with the nucleus bound and the walk moved by EPS of the
    row's ALLOWED mass, node out is the child of the edge taken. Asserts the premise first: the gap of l1 / T at rank k exceeds
    GAP (else fp32 could not tell which token has rank k)."""
    B, V = lg.shape
    for b in range(B):
        al, kids = allowed_of(trie, int(nodes[b]), V)
        R = [] if spans is None else spans[b]
        tok, n = int(r["token"][b]), int(r["n_kept"][b])
        assert tok in al.tolist(), (b, tok)                          # allowed, first of all
        j = int(np.searchsorted(al, tok))
        assert int(r["node"][b]) == int(kids[j]), (b, tok)
        sub = penalised(lg[b], R, rep)[al]
        if T == 0:
            assert n == 1 and j == int(np.argmax(sub)), (b, tok)
            continue
        x = sub / T
        p = np.exp(x - x.max())
        p /= p.sum()
        nA = al.size
        order = np.lexsort((np.arange(nA), -p))
        front = np.cumsum(p[order]) - p[order]
        k = top_k if 1 <= top_k < nA else nA
        if k < nA:
            xs = np.sort(x)[::-1]
            assert xs[k - 1] - xs[k] > GAP, (b, k, xs[k - 1] - xs[k])
        z_k = float(p[order[:k]].sum())
        in_k = np.arange(nA) < k
        n_lo = int((in_k & (front <= (top_p - EPS) * z_k)).sum())
        n_hi = int((in_k & (front <= (top_p + EPS) * z_k)).sum())
        exact = int((in_k & (front <= top_p * z_k)).sum())
        print(f"V={V} T={T} top_p={top_p} k={top_k} row {b} ({nA} allowed): n_kept {n} in [{n_lo}, {n_hi}] (fp64 {exact})")
        assert n_lo <= exact <= n_hi and n_lo <= n <= n_hi and n <= nA, (b, n, n_lo, n_hi)
        if top_p == 1.0:
            assert n == k, (b, n, k)
        kept = np.sort(order[:n])                                   # the n_kept highest allowed tokens, walked in token order
        assert j in kept.tolist(), (b, tok)
        cdf = np.cumsum(p[kept])
        M = cdf[-1]
        i = int(np.searchsorted(kept, j))
        lo, hi = (cdf[i - 1] if i else 0.0) - EPS * M, cdf[i] + EPS * M
        assert lo <= float(u[b]) * M <= hi, (b, tok, lo, float(u[b]) * M, hi)


def logprob_bound(lg):
    """tests/test_sampling_gpu.py::test_logprob_is_log_softmax_of_the_raw_logits: 4 x what torch's own fp32 log_softmax
    deviates from fp64 on these logits, floor 1e-6. -> (fp64 log_softmax, bound)."""
    lg32 = torch.from_numpy(lg)
    ref = torch.log_softmax(lg32.double(), -1)
    return ref.numpy(), max(4.0 * float((torch.log_softmax(lg32, -1).double() - ref).abs().max()), 1e-6)


MODES = [(0.0, 1.0, 0), (0.7, 1.0, 0), (1.0, 0.9, 0), (0.7, 0.9, 5), (1.0, 1.0, 400)]


@pytest.mark.parametrize("T,top_p,top_k", MODES)
@pytest.mark.parametrize("V", VOCABS)
def test_the_rule_in_fp64_under_a_trie(V, T, top_p, top_k):
    """16 rows at nodes with 1, 2, 7 and 300 children (300: more than one element per thread), four rows each."""
    trie, roots = fan_trie(V, (1, 2, 7, 300), 11)
    rng = np.random.default_rng(V + top_k)
    lg = (3.0 * rng.standard_normal((16, V))).astype(np.float32)
    nodes = np.array([roots[b % 4] for b in range(16)])
    u = spread_u(16)
    r = step_trie(lg, nodes, trie, u=u if T > 0 else None, temperature=T, top_p=top_p, top_k=top_k, eos_id=EOS)
    check_trie_rows(r, lg, u, T, top_k, top_p, trie, nodes)
    ref, bound = logprob_bound(lg)                               # the RAW, WHOLE row's log-probability
    err = np.abs(r["logprob"] - ref[np.arange(16), r["token"]]).max()
    print(f"V={V}: largest log-probability error {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    assert r["done"].tolist() == [0] * 16 and r["n_active"] == 16 and r["counter"] == 0
    assert np.array_equal(r["ids"][:, 4], r["token"]) and r["pos"].tolist() == [4] * 16
    assert torch.equal(r["x"].view(torch.uint8), r["emb"][torch.from_numpy(r["token"]).long()].view(torch.uint8))


# ---- 3
@pytest.mark.parametrize("V", VOCABS)
def test_the_maximum_is_taken_over_the_allowed_set(V):
    """The allowed logits all lie 100 below the row's maximum at T = 0.5: with the row's maximum every e would underflow
    ((l - m) / T <= -200) and every u would return one token."""
    trie, roots = fan_trie(V, (7,), 3)
    al, _ = allowed_of(trie, roots[0], V)
    rng = np.random.default_rng(V + 1)
    row = rng.standard_normal(V).astype(np.float32)
    row[al] = (rng.standard_normal(al.size) - 100.0).astype(np.float32)
    lg = np.tile(row, (64, 1))
    u = spread_u(64)
    nodes = np.full(64, roots[0])
    r = step_trie(lg, nodes, trie, u=u, temperature=0.5, top_p=1.0)
    check_trie_rows(r, lg, u, 0.5, 0, 1.0, trie, nodes)
    assert (r["n_kept"] == 7).all() and len(set(r["token"].tolist())) >= 3


@pytest.mark.parametrize("V", VOCABS)
def test_top_k_beyond_the_children_with_u_at_the_top(V):
    trie, roots = fan_trie(V, (2, 7), 5)
    rng = np.random.default_rng(V + 2)
    lg = (3.0 * rng.standard_normal((8, V))).astype(np.float32)
    nodes = np.array([roots[b % 2] for b in range(8)])
    u = np.full(8, U_TOP)
    for top_k in (8, 50, V, 2 ** 31 - 1):
        r = step_trie(lg, nodes, trie, u=u, temperature=1.0, top_p=1.0, top_k=top_k)
        check_trie_rows(r, lg, u, 1.0, top_k, 1.0, trie, nodes)            # (asserts: allowed; n_kept = the number allowed)
        assert r["n_kept"].tolist() == [2, 7] * 4


@pytest.mark.parametrize("V", VOCABS)
def test_an_underflowed_allowed_token_beside_tokens_that_are_not(V):
    """Allowed: a (logit 0), b < c (logits -200, -300: e underflows to 0 in fp32) and an edge whose token lies past the
    vocabulary (the trie was built for a larger one: skipped). The best logits of the row are not allowed. No unallowed token is
    ever returned or counted, over 64 values of u."""
    a, b, c = 40, 77, V - 2
    trie = TokenTrie.from_sequences([[a], [b], [c], [V + 7]], EOS, V + 50)
    root = int(trie.root[0])
    assert trie.children(root)[0].tolist() == [a, b, c, V + 7]
    row = np.full(V, 5.0, dtype=np.float32)                      # every unallowed token is more likely than any allowed one
    row[a], row[b], row[c] = 0.0, -200.0, -300.0
    lg = np.tile(row, (64, 1))
    u = spread_u(64)
    nodes = np.full(64, root)
    for top_k, want_kept in ((0, 3), (50, 3), (2, 2), (1, 1)):
        r = step_trie(lg, nodes, trie, u=u, temperature=1.0, top_p=1.0, top_k=top_k)
        assert set(r["token"].tolist()) <= {a, b, c}, (top_k, set(r["token"].tolist()))
        assert r["token"].tolist() == [a] * 64                  # (all the mass: a's running mass exceeds u * M for every u < 1)
        assert r["n_kept"].tolist() == [want_kept] * 64, (top_k, r["n_kept"])
        assert (r["node"] == walk(trie, root, [a])).all()
    g = step_trie(lg, nodes, trie, temperature=0.0)
    assert g["token"].tolist() == [a] * 64
    # only underflowed tokens left (a is not allowed here): the maximum is b's, nothing underflows
    trie2 = TokenTrie.from_sequences([[b], [c], [V + 7]], EOS, V + 50)
    nodes2 = np.full(64, int(trie2.root[0]))
    r = step_trie(lg, nodes2, trie2, u=u, temperature=1.0, top_p=1.0)
    assert r["token"].tolist() == [b] * 64 and r["n_kept"].tolist() == [2] * 64


def test_a_penalised_allowed_token_flips_the_greedy_pick():
    V, S = 509, 16
    trie, roots = fan_trie(V, (2,), 9)
    al, kids = allowed_of(trie, roots[0], V)
    a, b = int(al[0]), int(al[1])
    lg = np.full((2, V), -5.0, dtype=np.float32)
    lg[:, 300] = 9.0                                             # (not allowed; in the span as well)
    lg[0, a], lg[0, b] = 4.0, 2.5                                # 4 / 1.5 = 2.67 > 2.5 > 4 / 1.7 = 2.35
    lg[1, a], lg[1, b] = -1.4, -1.0                              # -1 * 1.3 = -1.3 > -1.4 > -1 * 1.5: b is in the span here
    ids = np.full((2, S), 300)
    ids[0, 5], ids[1, 5] = a, b
    kw = dict(ids=ids, pos=np.full(2, 8), gen_start=np.full(2, 4), S=S, temperature=0.0)
    nodes = np.full(2, roots[0])
    lo = step_trie(lg, nodes, trie, repetition_penalty=1.3, **kw)
    mid = step_trie(lg, nodes, trie, repetition_penalty=1.5, **kw)
    hi = step_trie(lg, nodes, trie, repetition_penalty=1.7, **kw)
    assert lo["token"].tolist() == [a, b] and mid["token"].tolist() == [a, a] and hi["token"].tolist() == [b, a]
    ref, bound = logprob_bound(lg)
    for r in (lo, mid, hi):
        assert np.abs(r["logprob"] - ref[np.arange(2), r["token"]]).max() <= bound            # the raw row's, whatever the penalty did
        assert np.array_equal(r["logits_after"].view(np.uint32), lg.view(np.uint32))
        assert r["node"].tolist() == [int(kids[al.tolist().index(t)]) for t in r["token"].tolist()]


@pytest.mark.parametrize("T", [0.0, 0.8])
def test_a_mixed_batch(T):
    """Row 0 at a node with two children, row 1 unconstrained, row 2 done, row 3 without room, row 4 at a leaf, row 5 at a node
    past the trie."""
    V, S = 509, 16
    trie = TokenTrie.from_sequences([[40, 41], [60]], EOS, V)
    root = int(trie.root[0])
    leaf = walk(trie, root, [60, EOS])
    past = trie.n_nodes + 5
    lg = np.full((6, V), -30.0, dtype=np.float32)
    lg[1] = 0.0
    lg[:, 77] = 9.0                                              # the favourite of every row, allowed in none
    lg[0, 40], lg[0, 60] = 1.0, 8.0                              # (u = 0.5 walks past 40, whose share is 1.6e-4)
    ids0 = np.arange(6 * S).reshape(6, S) % 400 + 3
    pos0 = [3, 4, 5, S - 1, 6, 7]
    nodes = [root, -1, root, root, leaf, past]
    r = step_trie(lg, nodes, trie, ids=ids0, pos=pos0, done=[0, 0, 1, 0, 0, 0], S=S, eos_id=EOS, temperature=T,
                  u=np.full(6, 0.5) if T > 0 else None)
    want = ids0.copy()
    want[0, 4], want[1, 5] = 60, 77
    assert np.array_equal(r["ids"], want)                        # rows 2 .. 5 untouched
    assert r["token"].tolist() == [60, 77, -1, -1, -1, -1] and r["n_kept"][2:].tolist() == [0, 0, 0, 0]
    assert r["done"].tolist() == [0, 0, 1, 1, 1, 1] and r["n_active"] == 2 and r["counter"] == 0
    assert r["pos"].tolist() == [4, 5, 5, S - 1, 6, 7] == r["pos64"].tolist()
    assert r["node"].tolist() == [walk(trie, root, [60]), -1, root, root, leaf, past]
    assert r["logprob"][2:].tolist() == [0.0] * 4 and (r["logprob"][:2] < 0).all()
    emb = r["emb"]
    assert torch.equal(r["x"][0], emb[60]) and torch.equal(r["x"][1], emb[77])
    for b in (2, 3, 4, 5):                                       # the embedding of the row's current token
        assert torch.equal(r["x"][b], emb[int(ids0[b, pos0[b]])]), b
    # the next step of row 0: its only child is the EOS
    r2 = step_trie(lg[:1], [walk(trie, root, [60])], trie, ids=r["ids"][:1], pos=r["pos"][:1], S=S, eos_id=EOS, temperature=T,
                   u=np.full(1, 0.5) if T > 0 else None)
    assert r2["token"].tolist() == [EOS] and r2["done"].tolist() == [1] and r2["node"].tolist() == [leaf] and r2["n_active"] == 0


@pytest.mark.parametrize("B", [5, 20])
def test_two_launches_give_the_same_bits(B):
    V, S = 32000, 16
    trie, roots = fan_trie(V, (2, 7, 300), 13)
    rng = np.random.default_rng(B)
    lg = (4.0 * rng.standard_normal((B, V))).astype(np.float32)
    lg[:, EOS] = -50.0                                           # (no unconstrained row ends here)
    u = rng.random(B).astype(np.float32)
    ids = rng.integers(3, V, (B, S))
    nodes = np.array([(roots + [-1])[b % 4] for b in range(B)])
    for b in range(B):                                           # the span of the penalty holds allowed tokens
        if nodes[b] >= 0:
            ids[b, 3:5] = allowed_of(trie, int(nodes[b]), V)[0][:2]
    pos, done = np.full(B, 6), np.zeros(B)
    pos[2], done[3] = S - 1, 1
    kw = dict(u=u, ids=ids, pos=pos, done=done, gen_start=np.full(B, 2), S=S, temperature=0.9, top_p=0.9, top_k=40,
              repetition_penalty=1.2, eos_id=EOS)
    counter = torch.zeros(1, dtype=torch.int32, device=DEV)
    a = step_trie(lg, nodes, trie, counter=counter, **kw)
    b2 = step_trie(lg, nodes, trie, counter=counter, **kw)       # back to back on the same word
    assert a["n_active"] == B - 2 == int((a["done"] == 0).sum()) and a["counter"] == 0 and b2["counter"] == 0
    assert_same_bits(a, b2)
    assert np.array_equal(a["node"], b2["node"])


# ---- 4
def beam_trie_case(K, seed):
    """B = 3 samples on one trie of answers that share prefixes. Sample 0: slot 0 at a node with two children, the other slots
    empty at the root (fewer finite candidates than K). Sample 1: slots at different nodes, a finished slot carried with its
    node, and slot 1 far in front of slot 0 with one child planted 30 above its row, so that the parents swap and the nodes
    follow. Sample 2: an
    unconstrained slot, a live slot at a leaf and one at a node past the trie (both finished first), the rest at the root."""
    V, S = 512, S_STEP
    members = [[5, 6], [5, 7, 8], [5, 7, 9], [30], [31, 32], [31, 33], [400, 401, 402]]
    trie = TokenTrie.from_sequences(members, EOS, V)
    root = int(trie.root[0])
    at = lambda *p: walk(trie, root, list(p))                                       # noqa: E731
    g = torch.Generator().manual_seed(seed)
    N = 3 * K
    c = {"logits": (4.0 * torch.randn(N, V, generator=g)).float(),
         "score": -(0.25 + 3.0 * torch.rand(N, generator=g)).float(),
         "done": torch.zeros(N, dtype=torch.int32), "pos": torch.randint(3, 9, (N,), generator=g).to(torch.int32),
         "ids": torch.randint(3, V, (N, S), generator=g)}
    c["ngen"] = (c["pos"] - 2).clone()
    node = [root] * N
    c["score"][0], c["score"][1:K] = 0.0, NEG                                        # sample 0
    node[0] = at(5)
    s1 = K                                                                          # sample 1
    node[s1], node[s1 + 1], node[s1 + 2] = at(5), at(31), at(5, 7, 8, EOS)
    c["score"][s1], c["score"][s1 + 1] = -9.0, -0.1
    c["logits"][s1 + 1, 32] = 30.0
    c["done"][s1 + 2], c["score"][s1 + 2] = 1, -4.0
    for i in range(3, K):
        node[s1 + i] = (at(5, 7), at(400), at(400, 401), at(31), at(5))[i - 3]
    s2 = 2 * K                                                                      # sample 2
    node[s2], node[s2 + 1], node[s2 + 2] = -1, at(30, EOS), trie.n_nodes + 5
    c["score"][s2 + 1], c["score"][s2 + 2] = -0.2, -6.0
    if K == 8:
        c["pos"][s2 + 5], c["score"][s2 + 5] = S - 1, -0.4                          # out of room: carried
    return c, node, trie


@pytest.mark.parametrize("K,seed", [(3, 1), (8, 2)])
def test_beam_step_under_a_trie_follows_the_rule_in_fp64(K, seed):
    c, node, trie = beam_trie_case(K, seed)
    V = c["logits"].shape[1]
    emb = torch.randn(V, D_STEP, generator=torch.Generator().manual_seed(1)).to(DEV)
    r = run_beam(c, K, torch.float32, emb, node=node, trie=trie)
    lg64 = c["logits"].double()
    dev32 = float((torch.log_softmax(c["logits"], -1).double() - torch.log_softmax(lg64, -1)).abs().max())
    bound = max(4.0 * dev32, 1e-6)
    n_run = 0
    swapped = False
    for b in range(3):
        sl = slice(b * K, (b + 1) * K)
        want = beam_step_trie_ref(lg64[sl], c["score"][sl].double(), c["done"][sl].tolist(), c["pos"][sl].tolist(), c["ids"][sl],
                                  c["ngen"][sl].tolist(), node[sl], trie, eos_id=EOS)
        for (v0, _, _), (v1, _, _) in zip(want["ranked"][:-1], want["ranked"][1:]):   # near ties would make the order undecidable
            assert v1 == NEG or v0 - v1 > GAP, (b, want["ranked"])
        assert r["parent"][sl].tolist() == want["parent"] and r["token"][sl].tolist() == want["token"], b
        assert r["node"][sl].tolist() == want["node"], b
        assert torch.equal(r["ids"][sl], want["ids"])
        assert r["pos"][sl].tolist() == want["pos"] == r["pos64"][sl].tolist()
        assert r["done"][sl].tolist() == want["done"] and r["ngen"][sl].tolist() == want["n_generated"]
        for i in range(K):
            got, ref, tok = float(r["score"][b * K + i]), want["score"][i], want["token"][i]
            if tok < 0 or ref == NEG:
                assert got == ref
            else:
                assert abs(got - ref) <= bound, (b, i, got, ref, bound)
            j = b * K + want["parent"][i]
            src = tok if tok >= 0 else int(c["ids"][j, int(c["pos"][j])])
            assert torch.equal(r["x"][b * K + i].view(torch.uint8), emb[src].cpu().view(torch.uint8)), (b, i)
        n_run += want["done"][0] == 0
        swapped |= b == 1 and want["parent"][0] == 1
        if b == 0:                                                                  # two finite candidates, the rest at -inf
            assert [s != NEG for s in want["score"]] == [True, True] + [False] * (K - 2) and want["parent"][:3] == [0, 0, 1]
            assert want["token"][:2] == [6, 7] or want["token"][:2] == [7, 6]
        if b == 1:
            carried = [i for i in range(K) if want["parent"][i] == 2]
            assert len(carried) == 1 and want["token"][carried[0]] == -1 and want["node"][carried[0]] == node[K + 2]
        if b == 2:                                                                  # the leaf and the node past the trie: carried
            for j in (1, 2):
                i = want["parent"].index(j) if j in want["parent"] else None
                assert i is None or want["token"][i] == -1
    assert swapped                                                                  # slot 1's child leads sample 1, with slot 1's node
    assert int(r["n_active"]) == n_run and int(r["counter"]) == 0
    again = run_beam(c, K, torch.float32, emb, node=node, trie=trie)
    for k in r:
        assert torch.equal(r[k].view(torch.uint8) if r[k].is_floating_point() else r[k],
                           again[k].view(torch.uint8) if again[k].is_floating_point() else again[k]), k


# ------------------------------------------------------------------------------------------------ end to end
def members_for(tiny, seed=0, n=5):  # noqa: F811
    """Five random members per sample, lengths 1-4, tokens in [3, V), distinct by construction: two with first tokens of their
    own and a random length, three that share their first token and have the lengths 2, 3 and 4 (so no two are equal, and the
    trie branches at depth 0 and at depth 1)."""
    rng = np.random.default_rng(seed)
    V = tiny.eng.V
    out = []
    for _ in tiny.prefix:
        first = rng.choice(np.arange(3, V), size=3, replace=False)
        sets = []
        for i in range(n):
            length = int(rng.integers(1, 5)) if i < 2 else i
            tail = rng.choice(np.arange(3, V), size=length - 1, replace=False).tolist()
            sets.append([int(first[min(i, 2)])] + [int(t) for t in tail])
        assert len({tuple(s) for s in sets}) == n
        out.append(sets)
    return out


def dense_lp(tiny, ids):  # noqa: F811
    return dense_logits(tiny.eng, tiny.batch, ids).double().log_softmax(-1)


def test_greedy_under_five_members_per_sample(tiny):  # noqa: F811
    sets = members_for(tiny)
    trie = TokenTrie.from_sequences(sets, EOS, tiny.eng.V)
    out = generate.generate(tiny.eng, tiny.batch, temperature=0.0, constraints=sets, return_logprobs=True)
    assert tuple(out["choice"].shape) == (len(tiny.prefix),) and out["choice"].dtype == torch.int64
    lp = dense_lp(tiny, out["ids"])                                                 # one teacher-forced pass of the finished rows
    for b, p in enumerate(tiny.prefix):
        n = int(out["n_generated"][b])
        row = out["ids"][b, p:p + n].tolist()
        c = int(out["choice"][b])
        assert row[-1] == EOS and row[:-1] in sets[b] and sets[b].index(row[:-1]) == c          # a member, and choice names it
        assert out["tokens"][b, :n].tolist() == row and bool((out["tokens"][b, n:] == -1).all())
        node = int(trie.root[b])
        for t, tok in enumerate(row):                            # every step: the most likely ALLOWED token of the dense forward
            al, kids = allowed_of(trie, node, tiny.eng.V)
            at = lp[b, p - 1 + t]
            best = float(at[torch.from_numpy(al).to(at.device)].max())
            assert float(at[tok]) >= best - 2 * tiny.tol, (b, t, tok, float(at[tok]), best)
            assert abs(float(out["logprobs"][b, t]) - float(at[tok])) <= tiny.tol, (b, t)
            node = int(kids[al.tolist().index(tok)])
        assert node in trie.leaf_choice
    same = generate.generate(tiny.eng, tiny.batch, temperature=0.0, constraints=trie)            # a compiled trie is taken as it is
    assert torch.equal(same["ids"], out["ids"]) and torch.equal(same["choice"], out["choice"]) and "logprobs" not in same
    shared = generate.generate(tiny.eng, tiny.batch, temperature=0.0, constraints=sets[0])        # one set for the batch
    for b, p in enumerate(tiny.prefix):
        row = shared["ids"][b, p:p + int(shared["n_generated"][b])].tolist()
        assert row[-1] == EOS and sets[0].index(row[:-1]) == int(shared["choice"][b])


def test_sampling_under_members(tiny):  # noqa: F811
    sets = members_for(tiny, seed=1)
    n = 3
    out = generate.generate(tiny.eng, tiny.batch, temperature=1.0, num_return_sequences=n, constraints=sets, seed=7,
                            return_logprobs=True)
    B = len(tiny.prefix)
    assert tuple(out["choice"].shape) == (B, n) and tuple(out["ids"].shape) == (B, n, 128)
    for k in range(n):
        lp = dense_lp(tiny, out["ids"][:, k])
        for b, p in enumerate(tiny.prefix):
            m = int(out["n_generated"][b, k])
            row = out["ids"][b, k, p:p + m].tolist()
            assert row[-1] == EOS and sets[b].index(row[:-1]) == int(out["choice"][b, k]), (b, k, row)      # a member of ITS sample
            want = sum(float(lp[b, p - 1 + t, row[t]]) for t in range(m))
            got = float(out["sum_logprob"][b, k])
            print(f"sample {b} draw {k}: member {int(out['choice'][b, k])}, sum_logprob {got:.6f}, dense {want:.6f}")
            assert abs(got - want) <= m * tiny.tol, (b, k, got, want)
    again = generate.generate(tiny.eng, tiny.batch, temperature=1.0, num_return_sequences=n, constraints=sets, seed=7)
    assert torch.equal(again["ids"], out["ids"]) and torch.equal(again["choice"], out["choice"])


def mc_twin(tiny, sets):  # noqa: F811
    """The multiple-choice twin of the batch: text_id (B, 5, S) = prompt + member + EOS, labels on those positions."""
    ids0 = tiny.batch["text_id"]["vqa"]
    B, _, S = ids0.shape
    text = torch.zeros(B, 5, S, dtype=torch.int64)
    label = torch.zeros(B, 5, S, dtype=torch.int64)
    for b, p in enumerate(tiny.prefix):
        for c, m in enumerate(sets[b]):
            text[b, c, :p] = ids0[b, 0, :p]
            text[b, c, p:p + len(m) + 1] = torch.tensor(m + [EOS])
            label[b, c, p:p + len(m) + 1] = text[b, c, p:p + len(m) + 1]
    twin = dict(tiny.batch)
    twin.update({"text_id": {"vqa": text}, "label": {"vqa": label}})
    return twin


@pytest.mark.parametrize("a", [0.0, 1.0])
def test_beam_search_ranks_the_whole_set(tiny, a):  # noqa: F811
    sets = members_for(tiny, seed=2)
    K = 5
    out = generate.generate(tiny.eng, tiny.batch, num_beams=K, length_penalty=a, constraints=sets)
    bm = out["beams"]
    B = len(tiny.prefix)
    assert tuple(bm["choice"].shape) == (B, K) and tuple(out["choice"].shape) == (B,)
    mean_lp = torch.zeros(B, K, dtype=torch.float64)
    for k in range(K):
        lp = dense_lp(tiny, bm["ids"][:, k])
        for b, p in enumerate(tiny.prefix):
            assert float(bm["score"][b, k]) != NEG                                  # five members, five slots: every slot is finite
            m = int(bm["n_generated"][b, k])
            row = bm["ids"][b, k, p:p + m].tolist()
            c = int(bm["choice"][b, k])
            assert row[-1] == EOS and sets[b].index(row[:-1]) == c and int(bm["done"][b, k]) == 1
            want = sum(float(lp[b, p - 1 + t, row[t]]) for t in range(m))
            got = float(bm["score"][b, k])
            print(f"a={a} sample {b} slot {k}: member {c}, {m} tokens, score {got:.6f}, dense {want:.6f}")
            assert abs(got - want) <= m * tiny.tol, (b, k, got, want)
            mean_lp[b, c] = got / m
    for b in range(B):
        assert sorted(bm["choice"][b].tolist()) == list(range(K))                   # exactly the five members, each once
        rank = (bm["score"][b].double().cpu() / bm["n_generated"][b].double().cpu() ** a).tolist()
        best = rank.index(max(rank))
        assert int(out["choice"][b]) == int(bm["choice"][b, best]) and torch.equal(out["ids"][b], bm["ids"][b, best])
        assert float(out["score"][b]) == float(bm["score"][b, best])
    if a == 1.0:                                                                    # the multiple-choice criterion
        sc = score.score_options(tiny.eng, mc_twin(tiny, sets))
        mc = -sc["mean"].double().cpu()                                             # mean log-probability per option, EOS counted
        for b in range(B):
            assert sc["count"][b].tolist() == [len(m) + 1 for m in sets[b]]
            pick = int(out["choice"][b])
            print(f"sample {b}: beam search picks option {pick}; score_options means {mc[b].tolist()}")
            assert float(mc[b, pick]) >= float(mc[b].max()) - 2 * tiny.tol
            assert float((mc[b] - mean_lp[b]).abs().max()) <= tiny.tol, (b, mc[b], mean_lp[b])


# ---- 8
def test_the_public_surface():
    m = model_of("tiny_peakedperm", torch.float32)
    batch = eos_batch("tiny_peakedperm")
    opts = options_of(batch, m.tokenizer)
    for beams in (1, 3):
        m.args.gen_constrain, m.args.num_beams = "options", beams
        try:
            best, extracted = m(batch, inference=True)
        finally:
            del m.args.gen_constrain, m.args.num_beams
        g = m.last_generation
        assert torch.equal(best.cpu(), g["choice"].cpu()) and bool((g["choice"] >= 0).all()) and len(extracted) == 4
        for b, p in enumerate(batch["prefix_index"]["vqa"]):
            want = opts[b][int(best[b])]
            row = g["ids"][b, p:p + len(want) + 1].tolist()
            assert row == want + [EOS], (beams, b)                 # the ids behind the prompt are the chosen option's tokens
    ans = m.generate(batch, constraints=opts)                       # the keyword goes through; "choice" is left behind
    assert "choice" in m.last_generation and len(ans) == 4
    for b in range(4):
        assert ans[b] == opts[b][int(m.last_generation["choice"][b])]
    m.generate(batch)
    assert "choice" not in m.last_generation


def test_answer_cli_constrained():
    r = subprocess.run([sys.executable, "answer.py", "--random_init", "--synthetic", "--question", "what is the man doing",
                        "--options", "a", "b", "c", "--constrain"], cwd=os.path.join(ROOT, "flipped-vqa_amd"),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    hit = re.search(r"^choice (\d): (\w)$", r.stdout, re.M)
    assert hit and (int(hit.group(1)), hit.group(2)) in [(0, "a"), (1, "b"), (2, "c")], r.stdout[-500:]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_sixteen_bit_builds_return_members(dtype):
    m = model_of("tiny_peakedperm", dtype)
    batch = eos_batch("tiny_peakedperm")
    opts = options_of(batch, m.tokenizer)
    for kw in (dict(temperature=0.0), dict(temperature=0.9, top_k=3, seed=1), dict(num_beams=5, length_penalty=1.0)):
        out = generate.generate(m.ensure_engine(), batch, constraints=opts, **kw)
        for b, p in enumerate(batch["prefix_index"]["vqa"]):
            c = int(out["choice"][b])
            assert c >= 0 and out["ids"][b, p:p + int(out["n_generated"][b])].tolist() == opts[b][c] + [EOS], (kw, b)
