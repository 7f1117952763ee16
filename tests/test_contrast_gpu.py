"""Contrastive decoding against a twin prompt on the GPU: the token-step kernel alone (fvqa_decode_next_pair, csrc/sample.hip)
against fvqa_decode_next_ex bit for bit at neutral parameters and on identical twins, against the fp64 restatement of
tests/test_contrast_cpu.py everywhere else; then `generate(contrast=...)` end to end on the tiny fixture of tests/test_beam_gpu.py
— against plain greedy decoding, against teacher-forced dense forwards with the clip and with zeros, against the scoring path."""
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from fvqa import generate, ops, score
from tests.test_beam_gpu import GAP, dense_logits, tiny  # noqa: F401  (tiny: the fixture and its tolerance)
from tests.test_constrained_cpu import allowed_of, kept_set_trie
from tests.test_constrained_gpu import mc_twin, members_for
from tests.test_contrast_cpu import contrast_parts, contrast_pick
from tests.test_generate_gpu import DEV, DTYPES, EPS, model_of, spread_u
from tests.test_sampling_gpu import BOOK, VOCABS, assert_same_bits, book_case, check_rows, make_emb, step_ex
from fvqa.constrain import TokenTrie

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EOS = 2
NP = 16                                               # pairs per launch


# ------------------------------------------------------------------------------------------------ the kernel alone
@functools.lru_cache(maxsize=None)
def rows_of(V, scale):
    """The 16 positive and 16 negative rows of the checks below (read only: shared by every test of a vocabulary)."""
    rng = np.random.default_rng(V)
    lp = (scale * rng.standard_normal((NP, V))).astype(np.float32)
    ln = (0.8 * lp + 0.6 * scale * rng.standard_normal((NP, V))).astype(np.float32)
    return lp, ln


def step_pair(lpos, lneg, *, alpha, beta, emb=None, u=None, ids=None, ids_neg=None, pos=None, pos_neg=None, done=None,
              done_neg=None, gen_start=None, node=None, trie=None, S=16, D=128, dtype=torch.float32, counter=None, **kw):
    """tests/test_sampling_gpu.py::step_ex through the pair entry: one launch on host arrays -> dict of host arrays. The keys of
    step_ex hold the POSITIVE half (so that assert_same_bits compares it with step_ex's result), "neg" the same keys of the
    negative half."""
    both = np.concatenate([np.asarray(lpos, dtype=np.float32), np.asarray(lneg, dtype=np.float32)], 0)
    lg = torch.as_tensor(both, device=DEV).clone()
    B = both.shape[0] // 2
    V = both.shape[1]
    if emb is None:
        emb = make_emb(V, D, dtype)
    t = lambda a, dt: torch.as_tensor(np.asarray(a), dtype=dt, device=DEV).contiguous()   # noqa: E731

    def two(a, b, fill):                              # the positive half, then the negative one (a copy of it by default)
        a = fill if a is None else np.asarray(a)
        return np.concatenate([a, a if b is None else np.asarray(b)], 0)
    ids = t(two(ids, ids_neg, np.zeros((B, S))), torch.int64)
    pos = t(two(pos, pos_neg, np.full(B, 3)), torch.int32)
    done = t(two(done, done_neg, np.zeros(B)), torch.int32)
    gs = t(np.zeros(B) if gen_start is None else gen_start, torch.int32)
    x = torch.full((2 * B, emb.shape[1]), float("nan"), dtype=emb.dtype, device=DEV)
    i32 = lambda n: torch.full((n,), -7, dtype=torch.int32, device=DEV)                  # noqa: E731
    tok, kept, npl, act = i32(B), i32(B), i32(B), i32(1)
    lp = torch.full((B,), float("nan"), dtype=torch.float32, device=DEV)
    pos64 = torch.full((2 * B,), -7, dtype=torch.int64, device=DEV)
    if counter is None:
        counter = torch.zeros(1, dtype=torch.int32, device=DEV)
    nd = None if node is None else t(node, torch.int32)
    ops.decode_next_pair(lg, emb, ids, pos, done, gs, x, tok, kept, npl, lp, act, counter, alpha=alpha, beta=beta, node=nd,
                         trie=None if trie is None else trie.to(DEV), u=None if u is None else t(u, torch.float32), pos64=pos64,
                         **kw)
    torch.cuda.synchronize()
    h = lambda a: a.cpu().numpy()                                                        # noqa: E731
    out = {"token": h(tok), "n_kept": h(kept), "n_plausible": h(npl), "n_active": int(act), "ids": h(ids[:B]), "pos": h(pos[:B]),
           "done": h(done[:B]), "x": x[:B].cpu(), "emb": emb.cpu(), "pos64": h(pos64[:B]), "logprob": h(lp),
           "counter": int(counter), "logits_after": h(lg), "logits": both,
           "neg": {"ids": h(ids[B:]), "pos": h(pos[B:]), "done": h(done[B:]), "x": x[B:].cpu(), "pos64": h(pos64[B:])}}
    if nd is not None:
        out["node"] = h(nd)
    return out


def assert_twin_follows(r, ids_neg_before=None):
    """The negative half after the step: the same token at the same position of its id row (nothing else of the row changed),
    the same embedding row, the positive row's pos, pos64 and done."""
    n = r["neg"]
    assert np.array_equal(n["pos"], r["pos"]) and np.array_equal(n["pos64"], r["pos64"]) and np.array_equal(n["done"], r["done"])
    assert torch.equal(n["x"].view(torch.uint8), r["x"].view(torch.uint8))
    for b, tok in enumerate(r["token"]):
        if tok >= 0:
            assert n["ids"][b, r["pos"][b]] == tok == r["ids"][b, r["pos"][b]], b
    if ids_neg_before is not None:
        want = np.asarray(ids_neg_before).copy()
        for b, tok in enumerate(r["token"]):
            if tok >= 0:
                want[b, r["pos"][b]] = tok
        assert np.array_equal(n["ids"], want)


NEUTRAL = ((0.0, 1.0), (0.8, 0.95), (1.0, 0.5), (0.3, 0.9), (1.5, 0.99))     # greedy + the settings of the existing neutral test


# ---- 1
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("V,scale", VOCABS)
def test_neutral_parameters_are_decode_next_ex_bit_for_bit(V, scale, dtype):
    lp, ln = rows_of(V, scale)
    rng = np.random.default_rng(V + 1)
    u = rng.random(NP).astype(np.float32)
    ids = rng.integers(0, V, (NP, 16))
    ids_neg = rng.integers(0, V, (NP, 16))                               # (the twin's own row: only position pos + 1 may change)
    both = np.concatenate([lp, ln], 0)
    for D in (128, 36):                               # (36 elements: 16-bit rows that are no multiple of 16 bytes)
        emb = make_emb(V, D, dtype)
        for T, top_p in NEUTRAL:
            kw = dict(emb=emb, ids=ids, u=u if T > 0 else None, temperature=T, top_p=top_p, eos_id=EOS, gen_start=np.full(NP, 1))
            old = step_ex(lp, **kw)
            new = step_pair(lp, ln, alpha=0.0, beta=0.0, ids_neg=ids_neg, **kw)
            assert_same_bits(old, new)                # token, n_kept, ids, pos, pos64, done, logprob, x, n_active
            assert_twin_follows(new, ids_neg)
            assert new["counter"] == 0 and new["x"].dtype == dtype
            assert np.array_equal(new["logits_after"].view(np.uint32), both.view(np.uint32))
            assert np.array_equal(new["n_plausible"], np.full(NP, V))


# ---- 2
@pytest.mark.parametrize("alpha", [0.5, 2.0])
@pytest.mark.parametrize("V,scale", VOCABS)
def test_identical_twins_are_the_plain_rule_at_any_alpha(V, scale, alpha):
    """l- = l+: the two lse have the same bits and c = l+ + alpha * 0. A twin read from row b + 1 in place of b + n_seq would
    see another row (the 16 rows are distinct) and fail here."""
    lp, _ = rows_of(V, scale)
    assert len({row.tobytes() for row in lp}) == NP
    u = np.random.default_rng(V + 1).random(NP).astype(np.float32)
    ids = np.random.default_rng(V + 2).integers(0, V, (NP, 16))
    emb = make_emb(V, 128, torch.float32)
    for T, top_p in NEUTRAL:
        kw = dict(emb=emb, ids=ids, u=u if T > 0 else None, temperature=T, top_p=top_p, eos_id=EOS, gen_start=np.full(NP, 1))
        old = step_ex(lp, **kw)
        new = step_pair(lp, lp, alpha=alpha, beta=0.0, **kw)
        assert_same_bits(old, new)
        assert_twin_follows(new, ids)
        assert np.array_equal(new["n_plausible"], np.full(NP, V)) and new["counter"] == 0


# ---- 3
@pytest.mark.parametrize("beta", [0.0, 0.1, 0.5])
@pytest.mark.parametrize("alpha", [0.5, 1.0, 2.0])
@pytest.mark.parametrize("V,scale", VOCABS)
def test_greedy_follows_the_rule_in_fp64(V, scale, alpha, beta):
    """Every row, none skipped. The premise is asserted first: in fp64 the two best c inside P are more than GAP apart and no
    token lies within GAP of the plausibility bound (for this generator and these seeds the smallest top-2 gaps over the nine
    settings are 3.0e-3 / 3.1e-2 / 3.7e-2 at V = 509 / 32000 / 40003, the smallest distances to the bound 4.6e-3 / 7.7e-3 /
    2.4e-2; the contrast changes the pick in 53 / 78 / 57 of the 144 row-settings, so a kernel that ignores l- fails)."""
    lp, ln = rows_of(V, scale)
    r = step_pair(lp, ln, alpha=alpha, beta=beta, temperature=0.0)
    changed = 0
    for b in range(NP):
        c, P, dist = contrast_parts(lp[b], ln[b], None, alpha, beta)
        best = np.sort(c[P])[::-1]
        gap = best[0] - best[1] if best.size > 1 else np.inf
        assert gap > GAP and dist > GAP, (b, gap, dist)
        tok, kept, n_pl = contrast_pick(lp[b], ln[b], None, [], 1.0, 0.0, 0, 1.0, alpha, beta, 0.0)
        changed += tok != int(lp[b].argmax())
        print(f"V={V} alpha={alpha} beta={beta} row {b}: token {r['token'][b]} (fp64 {tok}), |P| {r['n_plausible'][b]} "
              f"(fp64 {n_pl}), top-2 gap {gap:.3e}, distance to the bound {dist:.3e}")
        assert int(r["token"][b]) == tok and int(r["n_plausible"][b]) == n_pl and int(r["n_kept"][b]) == 1, b
    print(f"the contrast changes the pick of {changed} of {NP} rows")
    assert_twin_follows(r)
    assert np.array_equal(r["logits_after"].view(np.uint32), r["logits"].view(np.uint32)) and r["n_active"] == NP


# ---- 4
@pytest.mark.parametrize("T,top_k,top_p,rep", [(0.8, 0, 0.9, 1.0), (1.0, 40, 1.0, 1.0), (0.7, 5, 0.8, 1.3)])
@pytest.mark.parametrize("V,scale", VOCABS)
def test_sampling_follows_the_rule_in_fp64(V, scale, T, top_k, top_p, rep):
    """alpha = 1, beta = 0.1. Per row the row that the rule samples from — c over P, in fp64 — goes through
    tests/test_sampling_gpu.py::check_rows as a vocabulary of |P| tokens: n_kept inside its [n_lo, n_hi] bracket (EPS of the
    mass of the k, unchanged) and the token where u * M falls. Where u * M is further than EPS * M from every boundary of the
    walk, the token is the restatement's own."""
    alpha, beta, S = 1.0, 0.1, 16
    lp, ln = rows_of(V, scale)
    u = spread_u(NP)
    rng = np.random.default_rng(9000 + V)
    ids = rng.integers(0, V, (NP, S))
    ids[:, 5:10] = np.argsort(-lp, axis=1)[:, :5]                         # the span holds each row's five most likely tokens,
    ids[:, 10] = ids[:, 5]                                                # one of them twice, an id past the vocabulary
    ids[:, 11], ids[:, 12] = V + 3, -1                                    # and a negative one
    gs, pos = np.full(NP, 5), np.full(NP, 13)
    r = step_pair(lp, ln, alpha=alpha, beta=beta, u=u, ids=ids, pos=pos, gen_start=gs, S=S, temperature=T, top_k=top_k,
                  top_p=top_p, repetition_penalty=rep)
    exact = 0
    for b in range(NP):
        c, P, dist = contrast_parts(lp[b], ln[b], None, alpha, beta)
        assert dist > GAP, (b, dist)
        assert int(r["n_plausible"][b]) == P.size and 1 <= int(r["n_kept"][b]) <= P.size, b
        tok = int(r["token"][b])
        assert tok in P, (b, tok)
        R = ids[b, 5:14].tolist()
        in_P = {int(t): j for j, t in enumerate(P)}
        sub_R = [in_P[t] for t in R if t in in_P]                         # the penalised tokens of P, as indices into c[P]
        one = {"n_kept": r["n_kept"][b:b + 1], "token": np.array([in_P[tok]])}
        check_rows(one, c[P][None, :], u[b:b + 1], T, top_k, top_p, spans=[sub_R], rep=rep)
        want, kept, _ = contrast_pick(lp[b], ln[b], None, R, rep, T, top_k, top_p, alpha, beta, float(u[b]))
        if kept == int(r["n_kept"][b]):
            ks, p = kept_set_trie(c, P, R, rep, T, top_k, top_p)
            cdf = np.cumsum(p[np.searchsorted(P, ks)])
            if np.abs(cdf - float(u[b]) * cdf[-1]).min() > EPS * cdf[-1]:
                assert tok == want, (b, tok, want)
                exact += 1
    print(f"V={V} T={T} top_k={top_k} top_p={top_p} r={rep}: {exact} of {NP} tokens compared with the restatement's one to one")
    assert exact >= NP // 2
    assert_twin_follows(r, ids)
    assert np.array_equal(r["logits_after"].view(np.uint32), r["logits"].view(np.uint32))


# ---- 5
def test_pair_bookkeeping():
    """The BOOK case of tests/test_sampling_gpu.py as five pairs — pair 2 is full, pair 3 is done, pair 4 starts at -1 —, the
    negative rows with pos and done of their own that must be overwritten by the positive rows'."""
    lg, ids0 = book_case()
    S, V = BOOK["S"], BOOK["V"]
    ids_neg = ids0 + 1
    kw = dict(ids=ids0, ids_neg=ids_neg, pos=BOOK["pos"], pos_neg=[9, 9, 2, 2, 7], done=BOOK["done"], done_neg=[1, 0, 0, 0, 1],
              S=S, eos_id=EOS, gen_start=[2, 2, 2, 2, 0], alpha=1.0, beta=0.1)
    for stop, done_want, act_want in ((True, [0, 1, 1, 1, 1], 1), (False, [0, 0, 1, 1, 0], 3)):
        r = step_pair(lg, lg, stop_at_eos=stop, **kw)
        want = ids0.copy()
        want[0, 4], want[1, 5], want[4, 0] = 40, EOS, EOS
        assert np.array_equal(r["ids"], want)                                   # pairs 2 (full) and 3 (done) untouched
        want_neg = ids_neg.copy()
        want_neg[0, 4], want_neg[1, 5], want_neg[4, 0] = 40, EOS, EOS
        assert np.array_equal(r["neg"]["ids"], want_neg)                        # ... in both rows
        assert r["pos"].tolist() == [4, 5, S - 1, 6, 0] == r["pos64"].tolist() == r["neg"]["pos"].tolist()
        assert r["neg"]["pos64"].tolist() == [4, 5, S - 1, 6, 0]
        assert r["done"].tolist() == done_want == r["neg"]["done"].tolist()     # the positive row's, whatever the twin's were
        assert r["n_active"] == act_want and r["counter"] == 0                  # PAIRS still running
        assert r["token"].tolist() == [40, EOS, -1, -1, EOS] and r["n_kept"].tolist() == [1, 1, 0, 0, 1]
        assert r["n_plausible"].tolist() == [1, 1, 0, 0, 1]                     # (the one token 4.0 above the rest; 0: no pick)
        assert r["logprob"][2] == 0.0 and r["logprob"][3] == 0.0 and (r["logprob"][[0, 1, 4]] < 0).all()
        emb = r["emb"]
        for x in (r["x"], r["neg"]["x"]):
            assert torch.equal(x[0], emb[40]) and torch.equal(x[1], emb[EOS])
            assert torch.equal(x[2], emb[int(ids0[2, S - 1])]) and torch.equal(x[3], emb[int(ids0[3, 6])])   # the POSITIVE row's token
        assert_same_bits(step_ex(lg, ids=ids0, pos=BOOK["pos"], done=BOOK["done"], S=S, eos_id=EOS, gen_start=[2, 2, 2, 2, 0],
                                 stop_at_eos=stop), r)
    assert V == lg.shape[1]


# ---- 6
@pytest.mark.parametrize("V,scale", VOCABS)
def test_under_a_trie(V, scale):
    lp, ln = rows_of(V, scale)
    u = spread_u(NP)
    ids = np.random.default_rng(V + 3).integers(0, V, (NP, 16))
    emb = make_emb(V, 128, torch.float32)
    a, b_tok = int(np.argsort(-lp[0])[1]) % (V - 8) + 3, V - 2
    trie = TokenTrie.from_sequences([[a], [b_tok], [V + 5]], EOS, V + 10)        # three edges at the root, one outside [0, V)
    root = int(trie.root[0])
    al, kids = allowed_of(trie, root, V)
    assert al.tolist() == [a, b_tok] and trie.children(root)[0].tolist() == [a, b_tok, V + 5]
    # every node -1: the pairs pick from the vocabulary, bit for bit what the entry without a trie gives (and so decode_next_ex)
    for T, top_p in NEUTRAL[:3]:
        kw = dict(emb=emb, ids=ids, u=u if T > 0 else None, temperature=T, top_p=top_p, eos_id=EOS, gen_start=np.full(NP, 1))
        free = step_pair(lp, ln, alpha=0.0, beta=0.0, node=np.full(NP, -1), trie=trie, **kw)
        assert_same_bits(step_ex(lp, **kw), free)
        assert (free["node"] == -1).all() and np.array_equal(free["n_plausible"], np.full(NP, V))
        bare = step_pair(lp, ln, alpha=1.0, beta=0.1, **kw)
        with_trie = step_pair(lp, ln, alpha=1.0, beta=0.1, node=np.full(NP, -1), trie=trie, **kw)
        assert_same_bits(bare, with_trie)
        assert np.array_equal(bare["n_plausible"], with_trie["n_plausible"])
    # every pair at the root: P and the pick inside the two usable edges
    for T in (0.0, 0.9):
        for alpha, beta in ((1.0, 0.1), (2.0, 0.0), (0.5, 1.0)):
            r = step_pair(lp, ln, alpha=alpha, beta=beta, node=np.full(NP, root), trie=trie, emb=emb, ids=ids,
                          u=u if T > 0 else None, temperature=T, eos_id=EOS)
            for b in range(NP):
                c, P, dist = contrast_parts(lp[b], ln[b], al, alpha, beta)
                assert dist > GAP or beta == 1.0, (b, dist)
                tok = int(r["token"][b])
                assert tok in P.tolist() and int(r["n_plausible"][b]) == P.size <= 2 and int(r["n_kept"][b]) <= P.size, b
                if T == 0.0 and (P.size == 1 or abs(c[P[0]] - c[P[1]]) > GAP):
                    assert tok == contrast_pick(lp[b], ln[b], al, [], 1.0, 0.0, 0, 1.0, alpha, beta, 0.0)[0], b
                assert int(r["node"][b]) == int(kids[al.tolist().index(tok)]), b          # the child of the edge taken
            assert_twin_follows(r, ids)
            assert r["n_active"] == NP and r["counter"] == 0


# ---- 7
def test_operand_checks():
    V, S, D = 64, 8, 16
    dev = dict(device=DEV)
    i32 = lambda n: torch.zeros(n, dtype=torch.int32, **dev)                    # noqa: E731

    def call(B, alpha=1.0, beta=0.1, **over):
        a = dict(logits=torch.zeros(2 * B, V, **dev), emb=torch.zeros(V, D, **dev), ids=torch.zeros(2 * B, S, dtype=torch.int64, **dev),
                 pos=i32(2 * B), done=i32(2 * B), gen_start=i32(B), x_next=torch.zeros(2 * B, D, **dev), token=i32(B), n_kept=i32(B),
                 n_plausible=i32(B), logprob=torch.zeros(B, **dev), n_active=i32(1), counter=i32(1))
        a.update(over)
        return ops.decode_next_pair(*a.values(), alpha=alpha, beta=beta)

    call(2)                                                                     # (the operands as such are fine)
    torch.cuda.synchronize()
    for kw in (dict(alpha=-0.1), dict(alpha=float("nan")), dict(beta=-0.1), dict(beta=1.01), dict(beta=float("nan")),
               dict(n_plausible=i32(3)), dict(token=i32(4)), dict(logits=torch.zeros(3, V, **dev)),
               dict(n_plausible=torch.zeros(2, **dev))):
        with pytest.raises(ValueError):
            call(2, **kw)
    with pytest.raises(ValueError, match="come together"):
        ops.decode_next_pair(torch.zeros(4, V, **dev), torch.zeros(V, D, **dev), torch.zeros(4, S, dtype=torch.int64, **dev), i32(4),
                             i32(4), i32(2), torch.zeros(4, D, **dev), i32(2), i32(2), i32(2), torch.zeros(2, **dev), i32(1), i32(1),
                             alpha=1.0, beta=0.1, node=i32(2))
    with pytest.raises(RuntimeError, match="fvqa_decode_next_pair"):            # FVQA_ESHAPE: 2 * n_seq > 65535, refused by the library
        call(32768)


# ------------------------------------------------------------------------------------------------ end to end
def test_a_twin_equal_to_the_batch_decodes_the_plain_greedy_ids(tiny):  # noqa: F811
    eng, batch = tiny.eng, tiny.batch
    ref = generate.generate(eng, batch, temperature=0.0, stop_at_eos=True)
    out = generate.generate(eng, batch, temperature=0.0, stop_at_eos=True, contrast={"video": batch["video"]}, contrast_alpha=2.0)
    assert set(out) == set(ref) | {"n_plausible"} and out["steps"] == ref["steps"]
    for k in ("ids", "n_generated", "tokens"):
        assert out[k].shape == ref[k].shape and torch.equal(out[k], ref[k]), k
    assert tuple(out["n_plausible"].shape) == tuple(out["tokens"].shape) and out["n_plausible"].dtype == torch.int32
    assert bool((out["n_plausible"][out["tokens"] >= 0] >= 1).all()) and bool((out["n_plausible"][out["tokens"] < 0] == 0).all())


def test_blind_contrast_follows_the_rule_on_dense_forwards(tiny):  # noqa: F811
    """alpha = 1, beta = 0.1 (the issue's first setting; it leaves few positions undecided on this fixture, see the printed
    count): the returned rows are teacher-forced through the EXISTING forward twice, with the clip and with zeros, and at
    every generated position the token must be the restatement's pick from those two rows of logits — wherever the fp64 gap
    between the two best c exceeds 2 * (1 + 2 * alpha) * tol (a token's c moves by at most (1 + 2 * alpha) times the per-token
    tolerance) and no token lies within 2 * tol of the plausibility bound."""
    eng, batch = tiny.eng, tiny.batch
    alpha, beta, T = 1.0, 0.1, 12
    out = generate.generate(eng, batch, temperature=0.0, max_new_tokens=T, stop_at_eos=False, contrast="blind",
                            contrast_alpha=alpha, contrast_beta=beta)
    assert out["steps"] == T and tuple(out["tokens"].shape) == (len(tiny.prefix), T)
    blind = dict(batch)
    blind["video"] = torch.zeros_like(batch["video"])
    lpos = dense_logits(eng, batch, out["ids"]).double().cpu().numpy()
    lneg = dense_logits(eng, blind, out["ids"]).double().cpu().numpy()
    undecided = total = moved = 0
    for b, p in enumerate(tiny.prefix):
        for t in range(T):
            tok = int(out["tokens"][b, t])
            assert tok == int(out["ids"][b, p + t])
            c, P, dist = contrast_parts(lpos[b, p - 1 + t], lneg[b, p - 1 + t], None, alpha, beta)
            best = np.sort(c[P])[::-1]
            gap = best[0] - best[1] if best.size > 1 else np.inf
            total += 1
            if gap > 2 * (1 + 2 * alpha) * tiny.tol and dist > 2 * tiny.tol:
                want, _, n_pl = contrast_pick(lpos[b, p - 1 + t], lneg[b, p - 1 + t], None, [], 1.0, 0.0, 0, 1.0, alpha, beta, 0.0)
                assert tok == want and int(out["n_plausible"][b, t]) == n_pl, (b, t, tok, want)
                moved += want != int(lpos[b, p - 1 + t].argmax())
            else:
                undecided += 1
    print(f"{total} generated positions, {undecided} undecided (gap <= {2 * (1 + 2 * alpha) * tiny.tol:.1e} or a token within "
          f"{2 * tiny.tol:.1e} of the bound); the contrast moves the pick at {moved} positions")
    assert 8 * undecided <= total


def test_three_contrastive_samples_per_prompt_share_one_prefill(tiny, monkeypatch):  # noqa: F811
    eng, batch = tiny.eng, tiny.batch
    B, n, S = len(tiny.prefix), 3, 128
    calls = []
    real = eng.forward
    monkeypatch.setattr(eng, "forward", lambda data: (calls.append(int(data["text_id"]["vqa"].shape[0])), real(data))[1])
    kw = dict(temperature=0.8, seed=5, num_return_sequences=n, return_logprobs=True, max_new_tokens=12, contrast="blind")
    out = generate.generate(eng, batch, **kw)
    assert calls == [2 * B]                                                     # ONE prefill, of the batch and its twin
    monkeypatch.undo()
    steps = out["steps"]
    assert tuple(out["ids"].shape) == (B, n, S) and tuple(out["n_generated"].shape) == (B, n)
    assert tuple(out["tokens"].shape) == (B, n, steps) == tuple(out["logprobs"].shape) == tuple(out["n_plausible"].shape)
    assert tuple(out["sum_logprob"].shape) == (B, n)
    again = generate.generate(eng, batch, **kw)
    for k in ("ids", "tokens", "logprobs", "n_plausible"):
        assert torch.equal(out[k], again[k]), k
    worst = 0.0
    for k in range(n):
        lp = dense_logits(eng, batch, out["ids"][:, k]).double().log_softmax(-1)
        for b, p in enumerate(tiny.prefix):
            assert torch.equal(out["ids"][b, k, :p].cpu(), batch["text_id"]["vqa"][b, 0, :p])       # the prompt of ITS sample
            m = int(out["n_generated"][b, k])
            assert 1 <= m <= 12
            for t in range(m):
                tok = int(out["ids"][b, k, p + t])
                assert tok == int(out["tokens"][b, k, t]) and int(out["n_plausible"][b, k, t]) >= 1
                d = abs(float(lp[b, p - 1 + t, tok]) - float(out["logprobs"][b, k, t]))           # lp+: the model WITH the clip
                worst = max(worst, d)
                assert d <= tiny.tol, (b, k, t, d, tiny.tol)
            assert bool((out["tokens"][b, k, m:] == -1).all()) and bool((out["n_plausible"][b, k, m:] == 0).all())
    print(f"largest difference of a log-probability to the dense forward with the clip {worst:.3e}, tolerance {tiny.tol:.3e}")


def test_contrast_under_constraints(tiny):  # noqa: F811
    sets = [s[:2] for s in members_for(tiny, seed=3)]                          # two members per sample, distinct first tokens
    assert all(s[0][0] != s[1][0] for s in sets)
    out = generate.generate(tiny.eng, tiny.batch, temperature=0.0, constraints=sets, contrast="blind", contrast_alpha=1.0,
                            contrast_beta=0.1)
    assert tuple(out["choice"].shape) == (len(tiny.prefix),)
    for b, p in enumerate(tiny.prefix):
        c = int(out["choice"][b])
        assert c in (0, 1) and out["ids"][b, p:p + int(out["n_generated"][b])].tolist() == sets[b][c] + [EOS]
        assert 1 <= int(out["n_plausible"][b, 0]) <= 2                          # the root has two edges
        assert bool((out["n_plausible"][b, :int(out["n_generated"][b])] >= 1).all())


def test_contrastive_scoring(tiny):  # noqa: F811
    eng = tiny.eng
    data = mc_twin(tiny, members_for(tiny, seed=2))
    alpha = 1.0
    plain = score.score_options(eng, data)
    zeroed = dict(data)
    zeroed["video"] = torch.zeros_like(data["video"])
    by_hand = score.score_options(eng, zeroed)
    r = score.score_options(eng, data, contrast="blind", contrast_alpha=alpha)
    assert torch.equal(r["prediction_plain"], plain["prediction"]) and torch.equal(r["mean"], plain["mean"])
    assert torch.equal(r["individual_losses"], plain["individual_losses"])
    assert torch.equal(r["mean_blind"], by_hand["mean"]) and torch.equal(r["prediction_blind"], by_hand["prediction"])
    mp, mn = plain["mean"].double().cpu().numpy(), by_hand["mean"].double().cpu().numpy()
    s = plain["mean"].cpu().numpy() + np.float32(alpha) * (plain["mean"].cpu().numpy() - by_hand["mean"].cpu().numpy())
    assert bool((plain["count"] > 0).all())
    assert r["prediction"].cpu().tolist() == np.argmin(s, 1).tolist()           # (numpy's argmin: the first of equal minima)
    print("means with the clip", mp.tolist(), "blind", mn.tolist(), "prediction", r["prediction"].tolist())
    m = model_of("tiny_peakedperm", torch.float32)
    m.score_options(data, contrast="blind", contrast_alpha=alpha)
    assert {"mean_blind", "prediction_blind", "prediction_plain"} <= set(m.last_scoring)
    assert torch.equal(m.last_scoring["prediction"], r["prediction"])
    m.score_options(data)
    assert "mean_blind" not in m.last_scoring


def test_answer_cli_with_contrast():
    r = subprocess.run([sys.executable, "answer.py", "--random_init", "--synthetic", "--question", "what is the man doing",
                        "--contrast", "blind", "--contrast_alpha", "1.0", "--contrast_beta", "0.1"],
                       cwd=os.path.join(ROOT, "flipped-vqa_amd"), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert re.search(r"^\[\d+ tokens, \d+ steps, plausible tokens per step [\d.]+\]$", r.stdout, re.M), r.stdout[-500:]
    assert re.search(r"^\d+( \d+)*$", r.stdout, re.M), r.stdout[-500:]          # the answer, as token ids
