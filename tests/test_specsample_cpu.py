"""Draft-and-verify under sampling, without a GPU: the rule of include/fvqa.h (fvqa_spec_step_sample, fvqa_tree_spec_step_sample)
restated in numpy fp64 — `pick_ref` (rules 1 to 5 of fvqa_decode_next_ex with one draw), `spec_sample_ref` and `tree_sample_ref`, the
yardsticks of tests/test_specsample_gpu.py — and checked against a naive form that draws token by token with the plain rule and
counts the agreeing drafts; the two C entries exported by both builds and refusing bad operands before any launch; what `generate`
still refuses, with no engine present, and what it now lets through."""
import ctypes as C
import os
import sys
import types

import numpy as np
import pytest
import torch

from fvqa import _lib, generate, ops
from tests.test_lookahead_cpu import given_draft, lookup_draft, spec_step_ref
from tests.test_sampling_cpu import kept_set_ex, penalised, ranked
from tests.test_treedraft_cpu import DREL, TILE, WALK, plan_of, sample_plan, tree_step_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A = C.c_void_p(256)
BUILDS = [("bf16", _lib.BF16), ("f16", _lib.F16)]
EOS = 2


# ------------------------------------------------------------------------------------------------ the rule
def pick_ref(row, R, rep, T, top_k, top_p, u):
    """Rules 1 to 5 of fvqa_decode_next_ex on one raw row in fp64, with the draw u. -> dict(token, n_kept, logprob, and how well
    the pick is conditioned, all relative: margin — the distance of u * M to the two running-mass boundaries of the token (a
    boundary nothing lies behind does not count: 0 below the first kept token, M above the last) —, cut — the distance of
    top_p * Z_k to the mass in front of the last kept and of the first unkept rank —, gap_k — the gap of l1 / T at rank k, with
    p_k the share of the token at rank k in Z_k: what a swap at rank k can move any boundary by —;
    bounds — every such distance d with the cumulative share c of the mass its boundary sits at: logits that move by at most
    delta move a boundary by at most (2 * delta / T) * c * (1 - c), see `slack`).
    A row of NaNs (the header asks for finite logits; the kernel's comparisons then all fail the same way): the last token,
    n_kept = k, logprob NaN."""
    lg = np.asarray(row, dtype=np.float64)
    V = lg.size
    k = top_k if 1 <= top_k < V else V
    if np.isnan(lg).all():
        return dict(token=V - 1, n_kept=k, logprob=float("nan"), margin=1.0, cut=1.0, gap_k=np.inf, p_k=0.0, bounds=[])
    x = penalised(lg, R, rep) / T                                  # tests/test_sampling_cpu.py kept_set_ex, with one sort
    p = np.exp(x - x.max())
    p /= p.sum()
    order = np.argsort(-p, kind="stable")                          # p descending, index ascending
    front = np.cumsum(p[order]) - p[order]
    z_k = 1.0 if k == V else float(p[order[:k]].sum())
    kept = np.sort(order[(np.arange(V) < k) & (front <= top_p * z_k)])
    n = kept.size
    cut, bounds = 1.0, []                                          # (top_p == 1 cuts nothing: every rank < k has at most Z_k in front)
    if top_p < 1:
        cut = (top_p * z_k - front[n - 1]) / z_k
        bounds = [(cut, front[n - 1] / z_k)]
        if n < k:
            bounds.append(((front[n] - top_p * z_k) / z_k, front[n] / z_k))
            cut = min(cut, bounds[-1][0])
    gap_k, p_k = np.inf, 0.0
    if k < V:
        gap_k, p_k = float(x[order[k - 1]] - np.delete(x, order[:k]).max()), float(p[order[k - 1]]) / z_k
    cdf = np.cumsum(p[kept])
    M = cdf[-1]
    target = float(u) * M
    over = np.nonzero(cdf > target)[0]
    j = int(over[0]) if over.size else n - 1
    margin = np.inf
    if j > 0:
        margin = min(margin, (target - cdf[j - 1]) / M)
        bounds.append((margin, cdf[j - 1] / M))
    if j < n - 1:
        bounds.append(((cdf[j] - target) / M, cdf[j] / M))
        margin = min(margin, bounds[-1][0])
    mx = lg.max()
    tok = int(kept[j])
    return dict(token=tok, n_kept=int(n), logprob=float(lg[tok] - (mx + np.log(np.exp(lg - mx).sum()))), margin=float(margin),
                cut=float(cut), gap_k=gap_k, p_k=p_k, bounds=[(float(d), float(c)) for d, c in bounds])


def slack(pk, delta, T):
    """How far a pick (pick_ref's dict) is from changing when every logit may move by delta: the derivative of a cumulative share
    c of a softmax(l / T) with respect to logit shifts of size 1 is at most 2 * c * (1 - c) / T, so a boundary at share c moves
    by at most eps * c * (1 - c), eps = 2 * delta / T; the rank-k gap of l / T closes by at most eps, and once it can close the
    token at rank k may be swapped for its neighbour, which moves every boundary by at most p_k. < 0: the pick may flip."""
    eps = 2.0 * delta / T
    swap = pk["p_k"] if pk["gap_k"] <= eps else 0.0
    return min([d - eps * c * (1.0 - c) - swap for d, c in pk["bounds"]] + [1.0])


def _span(ids, g0, pos):
    """R: the ids at positions max(g0, 0) .. pos."""
    return [int(t) for t in ids[max(int(g0), 0):pos + 1]]


def spec_sample_ref(logits, w, m, ids, pos, done, n_generated, u, gen_start, *, T, temperature, top_p=1.0, top_k=0,
                    repetition_penalty=1.0, eos_id=EOS, stop_at_eos=True, max_new_tokens, drafts=None, G=2, pick=None):
    """One row of fvqa_spec_step_sample in fp64: tests/test_lookahead_cpu.py spec_step_ref with the pick of row i made by
    `pick_ref` with the draw u[min(n_generated + i, max_new_tokens - 1)] (u: the row's column of the draws, (max_new_tokens,)) on
    R = ids[gen_start .. pos], which holds what the rows before committed. -> spec_step_ref's dict plus n_kept and `picks`
    (pick_ref's dicts). pick (None: the sampler): pick(row, R, token index) -> a pick_ref dict."""
    lg = np.asarray(logits, dtype=np.float64)
    V, S = lg.shape[1], len(ids)
    ids = np.array(ids, dtype=np.int64)
    m = min(max(int(m), 1), T)
    if pick is None:
        pick = lambda row, R, t: pick_ref(row, R, repetition_penalty, temperature, top_k, top_p,       # noqa: E731
                                          u[min(max(t, 0), max_new_tokens - 1)])
    live = done == 0 and pos >= -1 and pos + 1 < S and n_generated < max_new_tokens
    toks, lps, picks = [], [], []
    if not live:
        at = min(max(pos, 0), S - 1)
        return dict(ids=ids, pos=pos, done=1, n_generated=n_generated, tokens=toks, logprobs=lps, n_committed=0, n_drafted=0,
                    w_next=[], w0=int(min(max(ids[at], 0), V - 1)), start=at, live=False, n_kept=[], picks=picks)
    for i in range(m):
        pk = pick(lg[i], _span(ids, gen_start, pos), n_generated)
        g = pk["token"]
        picks.append(pk)
        toks.append(g)
        lps.append(pk["logprob"])
        pos += 1
        n_generated += 1
        ids[pos] = g
        if stop_at_eos and g == eos_id:
            done = 1
            break
        if n_generated == max_new_tokens:
            done = 1
            break
        if pos + 1 >= S or i + 1 >= m or int(w[i + 1]) != g:
            break
    room = 0 if done else min(T, max_new_tokens - n_generated, S - 1 - pos)
    if room < 1:
        w_next = []
    elif drafts is not None:
        w_next = [toks[-1]] + given_draft(drafts, n_generated, room - 1, V)
    else:
        w_next = [toks[-1]] + lookup_draft(ids, pos, G, room - 1, V)
    return dict(ids=ids, pos=pos, done=done, n_generated=n_generated, tokens=toks, logprobs=lps, n_committed=len(toks),
                n_drafted=m - 1, w_next=w_next, w0=toks[-1], start=pos, live=True, n_kept=[q["n_kept"] for q in picks], picks=picks)


def tree_sample_ref(logits, plan1, ids, pos, done, n_generated, node, m, u, gen_start, *, R_in, R_out, temperature, top_p=1.0,
                    top_k=0, repetition_penalty=1.0, eos_id=EOS, stop_at_eos=True, max_new_tokens, pick=None):
    """One row of fvqa_tree_spec_step_sample in fp64: tests/test_treedraft_cpu.py tree_step_ref with the i-th commit of the step
    picked as in `spec_sample_ref` on the row the walk stands at. -> tree_step_ref's dict plus n_kept and `picks`."""
    lg = np.asarray(logits, dtype=np.float64)
    V, S = lg.shape[1], len(ids)
    ids = np.array(ids, dtype=np.int64)
    NP, ptok, pdep, pend, ppar = plan1
    NP = min(max(int(NP), 0), len(ptok))
    clampv = lambda t: int(min(max(int(t), 0), V - 1))                           # noqa: E731
    if pick is None:
        pick = lambda row, R, t: pick_ref(row, R, repetition_penalty, temperature, top_k, top_p,       # noqa: E731
                                          u[min(max(t, 0), max_new_tokens - 1)])
    a = int(node)
    if a < 0 or a >= NP:
        a = -1
    m = min(max(int(m), 1), R_in)
    m = 1 if a < 0 else min(m, NP - a)
    live = done == 0 and pos >= -1 and pos + 1 < S and n_generated < max_new_tokens
    tiles = (R_out + TILE - 1) // TILE
    pad = dict(depth=[0] * R_out, end=[j + 1 for j in range(R_out)], tile_anc=[[-1] * TILE for _ in range(tiles)])
    p0 = pos
    if not live:
        at = min(max(pos, 0), S - 1)
        return dict(ids=ids, pos=pos, done=1, n_generated=n_generated, node=int(node), tokens=[], logprobs=[], path=[],
                    n_committed=0, n_drafted=0, len=0, start=at, start_old=at, x_tokens=[clampv(ids[at])], running=False,
                    on_trie=False, live=False, n_kept=[], picks=[], **pad)
    toks, lps, path, picks, nd, j = [], [], [], [], a, 0
    while True:
        pk = pick(lg[j], _span(ids, gen_start, pos), n_generated)
        g = pk["token"]
        picks.append(pk)
        toks.append(g)
        lps.append(pk["logprob"])
        path.append(j)
        pos += 1
        n_generated += 1
        ids[pos] = g
        if (stop_at_eos and g == eos_id) or n_generated >= max_new_tokens:
            done, nd = 1, -1
            break
        if pos + 1 >= S:
            nd = -1
            break
        if nd < 0:
            break
        G = a + j
        e = min(int(pend[G]), NP)
        kids = [r for r in range(G + 1, e) if int(ppar[r]) == G and int(ptok[r]) == g]
        if not kids:
            nd = -1
            break
        nd = kids[0]
        if nd - a >= m or len(toks) >= WALK:
            break
        j = nd - a
    m2 = 0
    if not done:
        dmax = min(DREL, max_new_tokens - n_generated - 1, S - 2 - pos)
        if dmax >= 0 and nd < 0:
            m2 = 1
        if dmax >= 0 and nd >= 0:
            e = max(min(int(pend[nd]), nd + R_out, NP), nd + 1)
            cut = [r for r in range(nd + 1, e) if int(pdep[r]) - int(pdep[nd]) > dmax]
            m2 = min([e] + cut[:1]) - nd
    depth, end, x_tokens = list(pad["depth"]), list(pad["end"]), [toks[-1]]
    anc = [[-1] * TILE for _ in range(tiles)]
    if nd >= 0:
        for jj in range(m2):
            r = nd + jj
            depth[jj] = min(max(int(pdep[r]) - int(pdep[nd]), 0), DREL)
            end[jj] = min(max(int(pend[r]) - nd, jj + 1), m2)
            if jj >= 1:
                x_tokens.append(clampv(ptok[r]))
        for t in range(1, tiles):
            q = t * TILE
            if q < m2:
                k, r = depth[q], nd + q
                while k > 0:
                    pr = int(ppar[r])
                    if pr < nd or pr >= r:
                        break
                    k -= 1
                    anc[t][k] = pr - nd
                    r = pr
    return dict(ids=ids, pos=pos, done=done, n_generated=n_generated, node=nd, tokens=toks, logprobs=lps, path=path,
                n_committed=len(toks), n_drafted=m - 1, len=m2, start=pos, start_old=min(max(p0, 0), S - 1), x_tokens=x_tokens,
                running=not done, on_trie=(not done) and nd >= 0, live=True, depth=depth, end=end, tile_anc=anc,
                n_kept=[q["n_kept"] for q in picks], picks=picks)


def _argmax_pick(row, R, t):
    lg = np.asarray(row, dtype=np.float64)
    g, mx = int(np.argmax(lg)), lg.max()
    return dict(token=g, n_kept=1, logprob=float(lg[g] - (mx + np.log(np.exp(lg - mx).sum()))), margin=1.0, cut=1.0, gap_k=np.inf,
                p_k=0.0, bounds=[])


SAME_KEYS = ("pos", "done", "n_generated", "tokens", "logprobs", "n_committed", "n_drafted", "w_next", "w0", "start", "live")


def test_with_the_arg_max_as_the_pick_the_restatements_are_the_greedy_ones():
    """spec_sample_ref and tree_sample_ref are the greedy restatements with another pick: handed the arg-max they return what
    spec_step_ref and tree_step_ref return."""
    rng = np.random.default_rng(3)
    plan1 = sample_plan(plan_of([[5, 6, 7], [5, 8, 9], [5, 9], [11]], V=40), 0)
    for _ in range(200):
        T, V, S = int(rng.integers(1, 6)), 40, 12
        lg = rng.standard_normal((T, V)).astype(np.float32)
        for i in range(T):
            lg[i, rng.choice([5, 6, 7, 8, 9, 11, EOS, 20])] += 4
        w = np.concatenate([[-1], lg.argmax(1)[:-1]]).astype(np.int32)
        if T > 1 and rng.random() < 0.5:
            w[int(rng.integers(1, T))] = 30
        ids = rng.integers(3, 9, S)
        pos, done, ngen, m = int(rng.integers(-1, S)), int(rng.random() < 0.1), int(rng.integers(0, 9)), int(rng.integers(0, T + 2))
        drafts = rng.integers(-1, V + 1, 8) if rng.random() < 0.5 else None
        kw = dict(T=T, max_new_tokens=8, drafts=drafts, G=2)
        a = spec_sample_ref(lg, w, m, ids, pos, done, ngen, None, 0, temperature=1.0, pick=_argmax_pick, **kw)
        b = spec_step_ref(lg, w, m, ids, pos, done, ngen, **kw)
        assert all(a[k] == b[k] for k in SAME_KEYS) and np.array_equal(a["ids"], b["ids"])
        node = int(rng.integers(-1, 8))
        kw = dict(R_in=T, R_out=int(rng.integers(1, 9)), max_new_tokens=8)
        a = tree_sample_ref(lg, plan1, ids, pos, done, ngen, node, m, None, 0, temperature=1.0, pick=_argmax_pick, **kw)
        b = tree_step_ref(lg, plan1, ids, pos, done, ngen, node, m, **kw)
        assert all(np.array_equal(a[k], b[k]) for k in b), [k for k in b if not np.array_equal(a[k], b[k])]


def naive_step(lg, w, m, ids, pos, ngen, u, g0, *, T, max_new, prm, stop=True):
    """The naive form of one live row's step: draw a token on EVERY row of the pass with the plain rule — row i with the draw of
    token index n_generated + i and the penalty set the plain loop would hold there, the prompt span plus the tokens drawn so
    far —, count the drafts that agree from the front, commit that many plus one, and cut at the EOS, the budget and the end
    of the sequence. -> the committed tokens."""
    S = len(ids)
    row_ids = [int(t) for t in ids]
    drawn = []
    for i in range(m):
        R = row_ids[max(g0, 0):pos + 1] + drawn
        drawn.append(pick_ref(lg[i], R, prm["repetition_penalty"], prm["temperature"], prm["top_k"], prm["top_p"],
                              u[min(ngen + i, max_new - 1)])["token"])
    agree = 0
    while agree + 1 < m and int(w[agree + 1]) == drawn[agree]:
        agree += 1
    out = []
    for g in drawn[:agree + 1]:
        if pos + 1 + len(out) >= S:
            break
        out.append(g)
        if (stop and g == EOS) or ngen + len(out) == max_new:
            break
    return out


def test_the_step_rule_is_the_plain_rule_token_by_token():
    """A few hundred random small live rows: the restatement of the step against the naive form. (Row i + 1's penalty set must
    hold what row i committed, and its draw must be the next TOKEN's: a restatement that took either per step would differ.)"""
    rng = np.random.default_rng(17)
    n_multi = n_pen = 0
    for case in range(400):
        T, V, S, max_new = int(rng.integers(1, 7)), 12, 14, 9
        prm = dict(temperature=float(rng.choice([0.7, 1.3])), top_p=float(rng.choice([1.0, 0.9, 0.6])),
                   top_k=int(rng.choice([0, 1, 3, 5])), repetition_penalty=float(rng.choice([1.0, 1.7, 3.0])))
        lg = (2.0 * rng.standard_normal((T, V))).astype(np.float32)
        u = rng.random(max_new)
        ids = rng.integers(0, V, S)
        pos, ngen, g0 = int(rng.integers(-1, S - 1)), int(rng.integers(0, max_new)), int(rng.integers(-2, 6))
        m = int(rng.integers(1, T + 1))
        w = np.full(T, -1)
        # drafts that agree with what will be drawn for a random number of rows, found by running the restatement on them
        want_agree = int(rng.integers(0, m))
        for _ in range(m):
            r = spec_sample_ref(lg, w, m, ids, pos, 0, ngen, u, g0, T=T, max_new_tokens=max_new, drafts=rng.integers(0, V, max_new),
                                **prm)
            nc = r["n_committed"]
            if nc - 1 >= want_agree or nc >= m or r["done"] or r["w_next"] == []:
                break
            w[nc] = r["tokens"][nc - 1]
        got = spec_sample_ref(lg, w, m, ids, pos, 0, ngen, u, g0, T=T, max_new_tokens=max_new, drafts=rng.integers(0, V, max_new),
                              **prm)
        want = naive_step(lg, w, m, ids, pos, ngen, u, g0, T=T, max_new=max_new, prm=prm)
        assert got["tokens"] == want, (case, got["tokens"], want)
        assert got["n_committed"] == len(want) and got["ids"][pos + 1:pos + 1 + len(want)].tolist() == want
        assert got["n_kept"] == [q["n_kept"] for q in got["picks"]] and len(got["n_kept"]) == len(want)
        n_multi += len(want) > 1
        n_pen += prm["repetition_penalty"] > 1 and len(want) > 1
    assert n_multi >= 100 and n_pen >= 50, (n_multi, n_pen)      # the cases do commit several tokens, under a penalty too


def test_the_pick_keeps_what_the_sampling_tests_restatement_keeps():
    rng = np.random.default_rng(23)
    for V, scale in ((64, 2.0), (509, 3.0), (4000, 6.0)):
        for T, top_p, top_k, rep in ((0.8, 0.95, 0, 1.0), (1.0, 0.5, 7, 1.3), (0.3, 1.0, 3, 2.0), (1.5, 0.99, V + 1, 1.0)):
            lg = (scale * rng.standard_normal(V)).astype(np.float32)
            lg[5] = lg[9] = lg[11]                                 # ties are ordered by index in both
            R = rng.integers(-2, V + 2, 6).tolist()
            kept, p = kept_set_ex(lg, R, rep, T, top_k, top_p)
            _, order, _ = ranked(lg, R, rep, T)
            for u in (0.0, 0.37, 0.999999):
                pk = pick_ref(lg, R, rep, T, top_k, top_p, u)
                cdf = np.cumsum(p[kept])
                over = np.nonzero(cdf > u * cdf[-1])[0]
                assert pk["n_kept"] == kept.size and pk["token"] == int(kept[over[0] if over.size else -1]), (V, T, u)
            if 1 <= top_k < V:
                xs = np.sort(penalised(lg, R, rep) / T)[::-1]
                assert abs(pk["gap_k"] - (xs[top_k - 1] - xs[top_k])) < 1e-12


def test_the_pick_by_hand():
    lg = [2.0, 1.0, 0.0, -1.0]                                     # p = 0.644, 0.237, 0.087, 0.032
    assert [pick_ref(lg, [], 1.0, 1.0, 0, 1.0, u)["token"] for u in (0.0, 0.5, 0.7, 0.9, 0.99)] == [0, 0, 1, 2, 3]
    assert [pick_ref(lg, [], 1.0, 1.0, 2, 1.0, u)["token"] for u in (0.0, 0.7, 0.74, 0.99)] == [0, 0, 1, 1]    # M = 0.881
    assert pick_ref(lg, [], 1.0, 1.0, 2, 1.0, 0.5)["n_kept"] == 2 and pick_ref(lg, [], 1.0, 1.0, 0, 0.7, 0.5)["n_kept"] == 2
    assert pick_ref(lg, [0], 4.0, 1.0, 1, 1.0, 0.5)["token"] == 1  # 2 / 4 < 1: the penalty moves the head
    pk = pick_ref(lg, [], 1.0, 1.0, 0, 1.0, 0.65)                  # 0.65 lies 0.006 past the boundary at 0.644
    assert pk["token"] == 1 and 0.005 < pk["margin"] < 0.007
    assert abs(pk["logprob"] - np.log(0.2369)) < 1e-3
    assert slack(pk, 0.0, 1.0) == pk["margin"] and slack(pk, 0.05, 1.0) < 0 < slack(pk, 0.005, 1.0)
    nan = pick_ref([np.nan] * 4, [], 1.0, 1.0, 2, 1.0, 0.5)
    assert nan["token"] == 3 and nan["n_kept"] == 2 and np.isnan(nan["logprob"])


# ------------------------------------------------------------------------------------------------ the C entries
def _chain_args(dt, n_seq=3, T=4, u=A, temperature=0.8, top_p=0.9, top_k=0, rep=1.0, gen_start=A, n_kept=A, V=509):
    #       logits u emb drafts G temperature top_p top_k rep eos stop max_new
    return [A, u, A, A, 2, temperature, top_p, top_k, rep, 2, 1, 8,
            # ids pos done ngen gen_start w len start x token n_kept logprob nc nd act cnt pos64
            A, A, A, A, gen_start, A, A, A, A, A, n_kept, A, A, A, A, A, A,
            n_seq, T, V, 128, 16, dt, None]                          # B T V D S dtype stream


def _tree_args(dt, n_seq=3, R_in=4, R_out=4, u=A, temperature=0.8, top_p=0.9, top_k=0, rep=1.0, gen_start=A, n_kept=A, V=509):
    #       logits u emb plan_n token depth end parent P stride temperature top_p top_k rep eos stop max_new
    return [A, u, A, A, A, A, A, A, 9, 0, temperature, top_p, top_k, rep, 2, 1, 8,
            # ids pos done ngen gen_start node len start x depth end anc path n_path start_old token n_kept logprob nc nd act trie cnt pos64
            A, A, A, A, gen_start, A, A, A, A, A, A, A, A, A, A, A, n_kept, A, A, A, A, A, A, A,
            n_seq, R_in, R_out, V, 128, 16, dt, None]


@pytest.mark.parametrize("which,h16", BUILDS)
def test_the_entries_are_exported_and_refuse_bad_operands_before_any_launch(which, h16):
    """Every call here must be refused: one that passed validation would launch a kernel on fake addresses."""
    lib = _lib.load(which)
    assert lib.fvqa_version() == _lib.ABI_VERSION == 18          # added entries change no signature
    assert callable(ops.spec_step_sample) and callable(ops.tree_spec_step_sample)
    for fn, args, rows_kw, limit in ((lib.fvqa_spec_step_sample, _chain_args, "T", 16),
                                     (lib.fvqa_tree_spec_step_sample, _tree_args, "R_in", 64)):
        name = "fvqa_spec_step_sample" if args is _chain_args else "fvqa_tree_spec_step_sample"
        assert len(args(h16)) == len(_lib.SIGNATURES[name][1])
        for dt in (h16, _lib.F32):
            for kw in (dict(u=None), dict(gen_start=None), dict(n_kept=None)):
                assert fn(*args(dt, **kw)) == -1, (name, kw)
            for t in (0.0, -0.5, float("nan")):
                assert fn(*args(dt, temperature=t)) == -1, (name, t)
            for p in (0.0, -0.1, 1.5, float("nan")):
                assert fn(*args(dt, top_p=p)) == -1, (name, p)
            assert fn(*args(dt, top_k=-1)) == -1
            for r in (0.5, 0.999, float("nan")):
                assert fn(*args(dt, rep=r)) == -1, (name, r)
            assert fn(*args(dt, **{rows_kw: limit + 1})) == -2 and fn(*args(dt, **{rows_kw: 0})) == -2
            assert fn(*args(dt, n_seq=65536, **{rows_kw: 1})) == -2
            # the bitmap of the penalty lives in LDS: fvqa_decode_next_ex's vocabulary limit, only under a penalty
            assert fn(*args(dt, V=1216513, rep=1.3)) == -2
            for kw in (dict(u=C.c_void_p(258)), dict(gen_start=C.c_void_p(258)), dict(n_kept=C.c_void_p(258))):
                assert fn(*args(dt, **kw)) == -3, (name, kw)
            a = args(dt)
            a[0] = None                                              # a pointer of the extended entry: its own refusal
            assert fn(*a) == -1
    if which == "bf16":
        assert lib.fvqa_tree_spec_step_sample(*_tree_args(h16, R_in=4, R_out=65)) == -2


def test_the_ops_wrappers_refuse_host_tensors_and_greedy_parameters():
    z = torch.zeros(2, dtype=torch.int32)
    with pytest.raises(ValueError):
        ops.spec_step_sample(torch.zeros(2, 9), torch.zeros(9, 4), torch.zeros(2, 8, dtype=torch.int64), *([z] * 15),
                             u=torch.zeros(4, 2), max_new_tokens=4, temperature=0.7)
    with pytest.raises(ValueError):
        ops.tree_spec_step_sample(torch.zeros(2, 9), torch.zeros(9, 4), {"n_plan": z}, *([z] * 23), u=torch.zeros(4, 2),
                                  max_new_tokens=4, temperature=0.7)


# ------------------------------------------------------------------------------------------------ the keywords
class NoEngine:
    """Any touch of the engine fails the test: the refusals come before it."""

    def __getattr__(self, name):
        raise AssertionError(f"the engine was touched ({name}) before the call was refused")


def _batch(B=2, S=16):
    return {"text_id": {"vqa": torch.ones(B, 1, S, dtype=torch.int64)}, "prefix_index": {"vqa": [4] * B}}


C_ = [[5, 6], [7]]
SAMPLED = dict(temperature=0.8, top_p=0.9, top_k=20, repetition_penalty=1.3, seed=5)
FORMS = [dict(lookahead=4), dict(lookahead=16, draft_tokens=torch.zeros(2, 31, dtype=torch.int32)),
         dict(lookahead=16, draft_answers=C_)]
REFUSED = [dict(num_return_sequences=2), dict(num_beams=2), dict(num_beams=2, temperature=0.0), dict(constraints=C_),
           dict(contrast="blind"), dict(jump_forward=4, constraints=C_), dict(frame_attention=True),
           dict(top_p=0.0), dict(top_p=1.5), dict(top_k=-1), dict(top_k=2.5), dict(repetition_penalty=0.5),
           dict(temperature=0.0), dict(temperature=0.0, top_k=0), dict(temperature=0.0, repetition_penalty=1.0, top_k=5),
           dict(seed=None)]                                       # (no seed: no plain call to be equal to)


@pytest.mark.parametrize("form", FORMS, ids=lambda f: " ".join(sorted(f)))
@pytest.mark.parametrize("kw", REFUSED, ids=lambda kw: " ".join(f"{k}={v}" for k, v in kw.items() if k != "constraints") or "c")
def test_what_a_sampled_draft_call_still_refuses_is_refused_before_the_engine(form, kw):
    """(temperature=0.0 with the sampled call's top_k or repetition_penalty left on: greedy drafts verify against the plain
    greedy choice, which knows neither.)"""
    with pytest.raises(ValueError):
        generate.generate(NoEngine(), _batch(), **{**SAMPLED, **form, **kw})


@pytest.mark.parametrize("form", FORMS, ids=lambda f: " ".join(sorted(f)))
def test_a_sampled_draft_call_passes_the_checks_and_goes_on_to_the_engine(form):
    for kw in (SAMPLED, dict(temperature=0.7, seed=0), dict(temperature=1.3, top_p=1.0, seed=11, return_logprobs=True)):
        with pytest.raises(AssertionError, match="the engine was touched"):
            generate.generate(NoEngine(), _batch(), **{**kw, **form})


def test_the_stream_still_refuses_drafts():
    import llama
    m = types.SimpleNamespace(ensure_engine=lambda: pytest.fail("refused before the engine is built"))
    for kw in (dict(lookahead=4, temperature=0.8), dict(lookahead=16, draft_answers=C_, temperature=0.8)):
        with pytest.raises(ValueError):
            llama.Transformer.generate_stream(m, [_batch()], slots=2, **kw)


def test_at_temperature_zero_the_greedy_loops_are_called_as_before(monkeypatch):
    seen = {}
    monkeypatch.setattr(generate, "_generate_lookahead", lambda eng, data, **k: seen.update(chain=k))
    monkeypatch.setattr(generate, "_generate_tree_draft", lambda eng, data, **k: seen.update(tree=k))
    generate.generate(NoEngine(), _batch(), lookahead=4, seed=3, top_p=0.5)
    generate.generate(NoEngine(), _batch(), lookahead=4, draft_answers=C_)
    assert seen["chain"]["sampling"] is None and seen["tree"]["sampling"] is None
    generate.generate(NoEngine(), _batch(), lookahead=4, **SAMPLED)
    generate.generate(NoEngine(), _batch(), lookahead=4, draft_answers=C_, **SAMPLED)
    want = dict(temperature=0.8, top_p=0.9, top_k=20, repetition_penalty=1.3)
    assert seen["chain"]["sampling"] == want == seen["tree"]["sampling"] and seen["chain"]["seed"] == seen["tree"]["seed"] == 5


def test_the_model_passes_the_sampling_keywords_through(monkeypatch):
    from llama.model import Transformer
    seen = {}
    ids = torch.tensor([[7, 8, 9, EOS, 0, 0]])

    def fake(eng, data, **kw):
        seen.update(kw)
        return {"ids": ids, "n_generated": torch.tensor([3]), "steps": 2, "tokens": ids[:, 1:4].int(),
                "n_committed": torch.tensor([[1, 2]]), "n_drafted": torch.tensor([[0, 3]])}
    monkeypatch.setattr(generate, "generate", fake)
    me = types.SimpleNamespace(ensure_engine=lambda: None, tokenizer=types.SimpleNamespace(eos_id=EOS, sp_model=None))
    assert Transformer.generate.__wrapped__(me, {"prefix_index": {"vqa": [1]}}, max_new_tokens=3, lookahead=4, **SAMPLED) == [[8, 9]]
    assert seen == dict(max_new_tokens=3, lookahead=4, **SAMPLED)


def test_answer_cli_takes_drafts_together_with_the_sampling_flags():
    sys.path.insert(0, os.path.join(ROOT, "flipped-vqa_amd"))
    import answer
    q = ["--question", "what ?"]
    smp = ["--temperature", "0.8", "--top_p", "0.9", "--top_k", "20", "--repetition_penalty", "1.3", "--seed", "3"]
    a = answer.get_args_parser().parse_args(q + ["--lookahead", "8"] + smp)
    assert a.lookahead == 8 and a.temperature == 0.8 and a.top_k == 20 and a.repetition_penalty == 1.3
    a = answer.get_args_parser().parse_args(q + ["--options", "a", "b", "--draft", "options", "--lookahead", "33"] + smp)
    assert a.draft == "options" and a.temperature == 0.8
    for bad in (q + ["--lookahead", "8", "--temperature", "0.8", "--num_samples", "2"],
                q + ["--lookahead", "8", "--temperature", "0.8", "--num_beams", "2"],
                q + ["--lookahead", "8", "--top_k", "5"],                          # top_k without a temperature: greedy drafts
                q + ["--lookahead", "8", "--temperature", "0.8"],                  # no --seed
                q + ["--options", "a", "b", "--draft", "options", "--lookahead", "8", "--temperature", "0.8"],
                q + ["--options", "a", "b", "--draft", "options", "--lookahead", "8", "--temperature", "0.8", "--num_samples", "2"],
                q + ["--options", "a", "b", "--draft", "options", "--lookahead", "8", "--temperature", "0.8", "--constrain"]):
        with pytest.raises(SystemExit):
            answer.get_args_parser().parse_args(bad)
