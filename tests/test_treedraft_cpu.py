"""Tree-shaped draft verification, without a GPU: the rule of include/fvqa.h (fvqa_tree_spec_step) restated in numpy —
`tree_step_ref`, the yardstick of tests/test_treedraft_gpu.py — and checked on hand-made tries; the draft plan against a brute-force
walk of the trie; `predict_passes`, the host model of commits per step; the two C entries exported by both builds at ABI 18 and
refusing bad operands before any launch; `generate`'s keyword, what it refuses before an engine exists, and the flags."""
import ctypes as C
import inspect
import os
import sys
import types

import numpy as np
import pytest
import torch

from fvqa import _lib, constrain, generate, ops, stream, vocab

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A = C.c_void_p(256)
BUILDS = [("bf16", _lib.BF16), ("f16", _lib.F16)]
EOS = 2
WALK, TILE, DREL = 32, 32, 31


def plan_of(answers, B=1, V=32000, eos=EOS):
    """answers: one list of token sequences, or one list per sample -> the host plan (fvqa.vocab.plan_draft)."""
    return vocab.plan_draft(constrain.compile_constraints(answers, eos, V), B)


def sample_plan(plan, b):
    """One sample's (n_plan, token, depth, end, parent) of a shared or per-sample plan."""
    if plan["shared"]:
        return int(plan["n_plan"][0]), plan["token"], plan["depth"], plan["end"], plan["parent"]
    return int(plan["n_plan"][b]), plan["token"][b], plan["depth"][b], plan["end"][b], plan["parent"][b]


# ------------------------------------------------------------------------------------------------ the rule
def tree_step_ref(logits, plan1, ids, pos, done, n_generated, node, m, *, R_in, R_out, eos_id=EOS, stop_at_eos=True,
                  max_new_tokens):
    """One row of fvqa_tree_spec_step in fp64. logits (R_in, V); plan1 = (n_plan, token, depth, end, parent) of the row's sample;
    ids (S,), copied. -> dict of the row's state after the step and every output of the entry for this row (lists / ints;
    x_tokens: the tokens whose embeddings are the next pass's rows, zeros behind)."""
    lg = np.asarray(logits, dtype=np.float64)
    V, S = lg.shape[1], len(ids)
    ids = np.array(ids, dtype=np.int64)
    NP, ptok, pdep, pend, ppar = plan1
    NP = min(max(int(NP), 0), len(ptok))
    clampv = lambda t: int(min(max(int(t), 0), V - 1))                           # noqa: E731
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
                    on_trie=False, live=False, **pad)
    toks, lps, path, nd, j = [], [], [], a, 0
    while True:
        g = int(np.argmax(lg[j]))
        mx = lg[j].max()
        toks.append(g)
        lps.append(float(lg[j, g] - (mx + np.log(np.exp(lg[j] - mx).sum()))))
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
                running=not done, on_trie=(not done) and nd >= 0, live=True, depth=depth, end=end, tile_anc=anc)


def predict_passes(true_tokens, plan1, p, *, R, max_new, S, stop=True, eos=EOS, narrow_from=None, trace=None):
    """What each token step commits for one row, by the restatement: behind a correct prefix the model's pick is the plain greedy
    run's next token, so only the plan decides how far a pass gets. narrow_from: the step from which the loop asks for one-row
    passes (None: never — a row off its trie feeds one row at either width). trace: a list that receives, per step, whether the
    row is still running on its trie after it. -> the list of n_committed up to the step that ends the row."""
    NP, ptok, pdep, pend, ppar = plan1
    pos, ngen, done, node, m, out, t = p - 1, 0, False, 0, 1, [], 0
    while not done and pos + 1 < S and ngen < max_new:
        a, j, nc = node, 0, 0
        while True:
            g = int(true_tokens[ngen])
            pos, ngen, nc = pos + 1, ngen + 1, nc + 1
            if (stop and g == eos) or ngen >= max_new:
                done, node = True, -1
                break
            if pos + 1 >= S:
                node = -1
                break
            if node < 0:
                break
            G = a + j
            kids = [r for r in range(G + 1, min(int(pend[G]), NP)) if int(ppar[r]) == G and int(ptok[r]) == g]
            if not kids:
                node = -1
                break
            node = kids[0]
            if node - a >= m or nc >= WALK:
                break
            j = node - a
        out.append(nc)
        if trace is not None:
            trace.append(not done and node >= 0)
        r_out = 1 if narrow_from is not None and t >= narrow_from else R
        dmax = min(DREL, max_new - ngen - 1, S - 2 - pos)
        if done or dmax < 0:
            m = 0
        elif node < 0:
            m = 1
        else:
            e = max(min(int(pend[node]), node + r_out, NP), node + 1)
            cut = [r for r in range(node + 1, e) if int(pdep[r]) - int(pdep[node]) > dmax]
            m = min([e] + cut[:1]) - node
        t += 1
    return out


# ------------------------------------------------------------------------------------------------ the plan
def brute(answers, eos=EOS):
    """The trie as nested dicts, walked in pre-order with children in ascending token order -> rows [(path tuple)] of the
    internal nodes (every proper prefix of member + [eos], the empty one included)."""
    root = {}
    for a in answers:
        at = root
        for t in list(a) + [eos]:
            at = at.setdefault(int(t), {})
    rows = []

    def walk(at, path):
        if not at:
            return                                                   # a leaf (behind an EOS): no row
        rows.append(path)
        for t in sorted(at):
            walk(at[t], path + (t,))
    walk(root, ())
    return rows


SETS = {
    "three siblings": [[5, 6, 7], [5, 8, 9], [5, 9], [11]],
    "a prefix member": [[5, 6], [5, 6, 7, 8], [5]],
    "duplicates": [[4, 4, 4], [4, 4, 4], [4]],
    "deep": [list(range(10, 60))],                                   # 50 tokens: deeper than plan_vocab's 32
    "wide": [[100 + i, 7] for i in range(70)],
}


@pytest.mark.parametrize("name", sorted(SETS))
def test_the_plan_is_the_pre_order_walk(name):
    answers = SETS[name]
    NP, tok, dep, end, par = sample_plan(plan_of(answers), 0)
    rows = brute(answers)
    assert NP == len(rows)
    for g, path in enumerate(rows):
        assert int(dep[g]) == len(path) and (g == 0 or int(tok[g]) == path[-1])
        sub = [r for r, q in enumerate(rows) if q[:len(path)] == path]
        assert sub == list(range(g, int(end[g]))), (g, "the subtree is the contiguous range [g, end[g])")
        assert int(par[g]) == (-1 if g == 0 else rows.index(path[:-1]))
        kids, c = [], g + 1                                          # the children by the end chain: G + 1, end[G + 1], ...
        while c < int(end[g]):
            kids.append(c)
            c = int(end[c])
        assert kids == [r for r in range(NP) if int(par[r]) == g]
        assert [int(tok[k]) for k in kids] == sorted(int(tok[k]) for k in kids)
        for e in range(g, int(end[g]) + 1):                          # any prefix of the subtree is closed under ancestors
            assert all(int(par[r]) >= g for r in range(g + 1, e))
    deepest = max(len(a) for a in answers)
    assert int(dep[:NP].max()) == deepest                            # (no 32-token member limit: "deep" has depth 50)


def test_shared_and_per_sample_plans():
    sh = plan_of(SETS["three siblings"], B=3)
    assert sh["shared"] and sh["n_plan"].shape == (1,) and sh["token"].ndim == 1
    per = plan_of([SETS["three siblings"], SETS["deep"], [[9]]], B=3)
    assert not per["shared"] and per["n_plan"].tolist() == [8, 51, 2] and per["token"].shape == (3, 51)
    assert per["end"][2].tolist() == [2, 2] + list(range(3, 52)) and per["parent"][2, 2:].tolist() == [-1] * 49   # padding rows
    for k in ("token", "depth", "end", "parent"):
        assert np.array_equal(per[k][0, :8], sh[k])
    with pytest.raises(ValueError):
        plan_of([SETS["deep"], [[9]]], B=3)                          # a per-sample set built for another batch size


# ------------------------------------------------------------------------------------------------ the rule by hand
def peaked(tokens, V=40, R=None):
    lg = np.full((R or len(tokens), V), -1.0)
    for i, t in enumerate(tokens):
        if t is not None:
            lg[i, t] = 2.0
    return lg


def test_a_row_of_the_rule_by_hand():
    #  plan rows: 0 root | 1 "5" | 2 "5 6" | 3 "5 6 7" | 4 "5 8" | 5 "5 8 9" | 6 "5 9" | 7 "11"
    plan1 = sample_plan(plan_of(SETS["three siblings"]), 0)
    assert plan1[0] == 8 and plan1[1][1:8].tolist() == [5, 6, 7, 8, 9, 9, 11] and plan1[3][:8].tolist() == [8, 7, 4, 4, 6, 6, 7, 8]
    ids = [3, 4, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]
    base = dict(R_in=8, R_out=8, max_new_tokens=20)
    # the first step: the prefill's row alone says 5; the next pass is the whole subtree under "5" (6 rows)
    r = tree_step_ref(peaked([5], R=8), plan1, ids, 1, 0, 0, 0, 1, **base)
    assert r["tokens"] == [5] and r["node"] == 1 and r["len"] == 6 and r["path"] == [0] and r["n_drafted"] == 0
    assert r["x_tokens"] == [5, 6, 7, 8, 9, 9] and r["depth"][:6] == [0, 1, 2, 1, 2, 1] and r["end"][:6] == [6, 3, 3, 5, 5, 6]
    assert r["depth"][6:] == [0, 0] and r["end"][6:] == [7, 8] and r["start"] == 2 and r["start_old"] == 1
    # that pass: local rows 0 "5", 1 "5 6", 2 "5 6 7", 3 "5 8", 4 "5 8 9", 5 "5 9". The model says 8, 9, EOS: the MIDDLE sibling
    lg = peaked([8, None, None, 9, EOS, None], R=8)
    s = tree_step_ref(lg, plan1, r["ids"], r["pos"], 0, 1, 1, 6, **base)
    assert s["tokens"] == [8, 9, EOS] and s["path"] == [0, 3, 4] and s["done"] == 1 and s["node"] == -1 and s["len"] == 0
    assert s["ids"].tolist()[:6] == [3, 4, 5, 8, 9, EOS] and s["n_drafted"] == 5 and s["start_old"] == 2
    # the EOS with stop_at_eos off: the EOS edge leads to a leaf, no row has it — the row leaves the trie and goes on
    s = tree_step_ref(lg, plan1, r["ids"], r["pos"], 0, 1, 1, 6, stop_at_eos=False, **base)
    assert s["tokens"] == [8, 9, EOS] and s["done"] == 0 and s["node"] == -1 and s["len"] == 1 and s["x_tokens"] == [EOS]
    # leaving at depth 1: 5 then 30, which no child of "5" holds
    s = tree_step_ref(peaked([30], R=8), plan1, r["ids"], r["pos"], 0, 1, 1, 6, **base)
    assert s["tokens"] == [30] and s["node"] == -1 and s["len"] == 1 and s["on_trie"] is False and s["running"]
    # leaving at the root
    s = tree_step_ref(peaked([30], R=8), plan1, ids, 1, 0, 0, 0, 1, **base)
    assert s["tokens"] == [30] and s["node"] == -1
    # a child beyond the pass: R = 2 fed rows "5", "5 6" only; the model says 8 -> row 4 was cut, it becomes the next root
    s = tree_step_ref(peaked([8], R=2), plan1, r["ids"], r["pos"], 0, 1, 1, 2, R_in=2, R_out=2, max_new_tokens=20)
    assert s["tokens"] == [8] and s["node"] == 4 and s["len"] == 2 and s["x_tokens"] == [8, 9] and s["end"] == [2, 2]
    # node = -1: one token, one row
    s = tree_step_ref(peaked([7, 8], R=8), plan1, r["ids"], r["pos"], 0, 1, -1, 6, **base)
    assert s["tokens"] == [7] and s["n_drafted"] == 0 and s["len"] == 1
    # exact ties go to the lower index, on the trie or off it
    tie = peaked([8, None, None, 9], R=8)
    tie[0, 6] = 2.0
    assert tree_step_ref(tie, plan1, r["ids"], r["pos"], 0, 1, 1, 6, **base)["tokens"][0] == 6     # 6 ties with 8: the lower index
    # the budget: two tokens left -> the next pass may only hold relative depth 0; one left -> done after it
    s = tree_step_ref(peaked([5], R=8), plan1, ids, 1, 0, 0, 0, 1, R_in=8, R_out=8, max_new_tokens=2)
    assert s["len"] == 1 and s["done"] == 0
    s = tree_step_ref(peaked([5], R=8), plan1, ids, 1, 0, 0, 0, 1, R_in=8, R_out=8, max_new_tokens=1)
    assert s["done"] == 1 and s["len"] == 0
    # the end of the sequence: S = 4 -> after the commit at position 2 only relative depth 0 fits (its token lands at S - 1)
    s = tree_step_ref(peaked([5], R=8), plan1, ids[:4], 1, 0, 0, 0, 1, **base)
    assert s["pos"] == 2 and s["len"] == 1 and s["done"] == 0
    s = tree_step_ref(peaked([5], R=8), plan1, ids[:3], 1, 0, 0, 0, 1, **base)          # the row fills: done at its NEXT step
    assert s["pos"] == 2 and s["len"] == 0 and s["done"] == 0 and s["node"] == -1
    s = tree_step_ref(peaked([5], R=8), plan1, s["ids"], s["pos"], 0, 1, s["node"], 0, **base)
    assert not s["live"] and s["done"] == 1 and s["x_tokens"] == [5] and s["start"] == 2 and s["n_committed"] == 0


def test_the_budget_cut_keeps_a_prefix():
    plan1 = sample_plan(plan_of(SETS["three siblings"]), 0)
    ids = [3, 4] + [0] * 10
    # after the commit n_generated = 1; max_new = 3 -> Dmax = 1: rows "5", "5 6" fit, "5 6 7" (depth 2) cuts the pass in front of it
    s = tree_step_ref(peaked([5], R=8), plan1, ids, 1, 0, 0, 0, 1, R_in=8, R_out=8, max_new_tokens=3)
    assert s["len"] == 2 and s["x_tokens"] == [5, 6] and s["end"][:2] == [2, 2]


def test_the_tile_edge_chain():
    # a chain of 40 tokens: row 32 of the pass has relative depth 32 > 31 -> cut at 32 rows; with a fan in front of it, depth 1
    chain = plan_of([list(range(100, 140))])
    p1 = sample_plan(chain, 0)
    r = tree_step_ref(peaked([100], V=200, R=1), p1, [3] + [0] * 60, 0, 0, 0, 0, 1, R_in=1, R_out=64, max_new_tokens=60)
    assert r["len"] == 32 and r["depth"][:32] == list(range(32))                    # the relative depth cut at 31
    fan = plan_of([[50, 60 + i] for i in range(31)] + [[50, 95, 96]])                # root, "50", 31 leaves' parents ...
    p1 = sample_plan(fan, 0)
    r = tree_step_ref(peaked([7], V=200, R=1), p1, [3] + [0] * 60, 0, 0, 0, -1, 1, R_in=1, R_out=64, max_new_tokens=60)
    assert r["len"] == 1
    r = tree_step_ref(np.full((1, 200), -1.0), p1, [3] + [0] * 60, 0, 0, 0, 0, 1, R_in=1, R_out=64, max_new_tokens=60)
    assert r["node"] == -1                                                           # (argmax 0 is no child of the root)
    # rooted at the root itself: rows 0 root, 1 "50", 2 .. 32 "50 6x", 33 "50 95", 34 "50 95 96": row 32 has the chain [0, 1]
    lg = np.full((1, 200), -1.0)
    r = tree_step_ref(lg, p1, [3] + [0] * 60, -1, 0, 0, 0, 1, R_in=1, R_out=64, max_new_tokens=60)
    assert r["tokens"] == [0]


# ------------------------------------------------------------------------------------------------ the host model
def test_predict_passes_by_hand():
    plan1 = sample_plan(plan_of(SETS["three siblings"]), 0)
    kw = dict(max_new=31, S=128)
    assert predict_passes([5, 8, 9, EOS], plan1, 10, R=8, **kw) == [1, 3]            # the whole member in the second pass
    assert predict_passes([5, 8, 9, EOS], plan1, 10, R=2, **kw) == [1, 1, 2]         # "5 8" lies beyond two rows: the next root
    assert predict_passes([5, 8, 9, EOS], plan1, 10, R=4, **kw) == [1, 2, 1]         # "5 8 9" lies beyond four rows
    assert predict_passes([30, 31, 32, EOS], plan1, 10, R=8, **kw) == [1, 1, 1, 1]   # never on the trie
    assert predict_passes([5, 6, 30, EOS], plan1, 10, R=8, **kw) == [1, 2, 1]        # leaves at depth 2
    assert predict_passes([5, 6, 7, 9, EOS], plan1, 10, R=8, **kw) == [1, 3, 1]      # the member is a proper prefix of the answer
    assert sum(predict_passes([5, 8, 9, 4, 4, 4], plan1, 10, R=8, stop=False, max_new=6, S=128)) == 6
    trace = []
    assert predict_passes([5, 6, 30, EOS], plan1, 10, R=8, trace=trace, **kw) == [1, 2, 1] and trace == [True, False, False]


# ------------------------------------------------------------------------------------------------ the C entries
def _step_args(dt, n_seq=3, R_in=4, R_out=4, P=9, stride=0, max_new=8):
    #       logits emb n tok dep end par  P  stride eos stop max_new | 22 pointers, pos64 last | B Rin Rout V D S dtype stream
    return [A, A, A, A, A, A, A, P, stride, 2, 1, max_new] + [A] * 22 + [n_seq, R_in, R_out, 509, 128, 16, dt, None]


def _commit_args(dt, rows=4, Dh=128, rot=1):
    #       cache rows(B) path n_path start_old cos sin  n_seq rows S  H  Dh  A   L  rot dtype stream
    return [A, C.c_void_p(512), A, A, A, A, A, 3, rows, 32, 2, Dh, 10, 2, rot, dt, None]


@pytest.mark.parametrize("which,h16", BUILDS)
def test_the_entries_are_exported_and_check_their_operands_on_the_host(which, h16):
    """Every call here must be refused: one that passed validation would launch a kernel on fake addresses."""
    lib = _lib.load(which)
    assert lib.fvqa_version() == _lib.ABI_VERSION == 18              # added entries change no signature
    fn, cm = lib.fvqa_tree_spec_step, lib.fvqa_kv_tree_commit
    assert len(_step_args(h16)) == len(_lib.SIGNATURES["fvqa_tree_spec_step"][1])
    assert len(_commit_args(h16)) == len(_lib.SIGNATURES["fvqa_kv_tree_commit"][1])
    assert callable(ops.tree_spec_step) and callable(ops.kv_tree_commit)
    for dt in (h16, _lib.F32):
        base = _step_args(dt)
        for at in list(range(0, 7)) + list(range(12, 33)):           # every required pointer (pos64, the last one, may be NULL)
            a = list(base)
            a[at] = None
            assert fn(*a) == -1, at
        for kw in (dict(n_seq=0), dict(R_in=0), dict(R_out=0), dict(R_in=65), dict(R_out=65), dict(n_seq=65536, R_in=1, R_out=1),
                   dict(n_seq=1024, R_in=64, R_out=1), dict(n_seq=1024, R_in=1, R_out=64), dict(P=0), dict(stride=5),
                   dict(max_new=0)):
            assert fn(*_step_args(dt, **kw)) == -2, kw
        for at in (37, 38, 39):                                      # V, D, S <= 0
            a = list(base)
            a[at] = 0
            assert fn(*a) == -2, at
        for at in (0, 2, 6, 13, 20, 27, 32):                         # logits, plan_n, parent, pos, depth, logprob, counter off 4
            a = list(base)
            a[at] = C.c_void_p(258)
            assert fn(*a) == -3, at
        a = list(base)
        a[12] = C.c_void_p(260)                                      # ids off 8
        assert fn(*a) == -3
        cb = _commit_args(dt)
        for at in (0, 1, 2, 3, 4, 5, 6):
            a = list(cb)
            a[at] = None
            assert cm(*a) == -1, at
        a = list(cb)
        a[1] = A                                                     # the rows ARE the cache
        assert cm(*a) == -1
        a = list(_commit_args(dt, rot=0))
        a[5] = a[6] = None                                           # no tables needed for a raw cache — refused further on:
        a[0] = C.c_void_p(264)                                       # ... the cache off its 16-byte boundary
        assert cm(*a) == -3
        for kw in (dict(rows=0), dict(rows=65), dict(Dh=64)):
            assert cm(*_commit_args(dt, **kw)) == -2, kw
        a = list(cb)
        a[2] = C.c_void_p(258)
        assert cm(*a) == -3
    other = _lib.F16 if h16 == _lib.BF16 else _lib.BF16
    assert fn(*_step_args(other)) == -1 and cm(*_commit_args(other)) == -1     # the other build's 16-bit code


# ------------------------------------------------------------------------------------------------ the keyword
def _batch(B=2, S=16):
    return {"text_id": {"vqa": torch.ones(B, 1, S, dtype=torch.int64)}, "prefix_index": {"vqa": [4] * B}}


class NoEngine:
    """Any touch of the engine fails the test: the refusals come before it."""

    def __getattr__(self, name):
        raise AssertionError(f"the engine was touched ({name}) before the call was refused")


C_ = [[5, 6], [7]]
REFUSED = [
    dict(draft_answers=C_),                                                        # no lookahead
    dict(draft_answers=C_, lookahead=1),
    dict(draft_answers=C_, lookahead=65),
    dict(draft_answers=C_, lookahead=2.5),
    dict(draft_answers=C_, lookahead=4, draft_tokens=torch.zeros(2, 31, dtype=torch.int32)),
    dict(draft_answers=C_, lookahead=4, temperature=0.7),
    dict(draft_answers=C_, lookahead=4, top_k=5),
    dict(draft_answers=C_, lookahead=4, repetition_penalty=1.2),
    dict(draft_answers=C_, lookahead=4, num_return_sequences=2),
    dict(draft_answers=C_, lookahead=4, num_beams=2),
    dict(draft_answers=C_, lookahead=4, constraints=C_),
    dict(draft_answers=C_, lookahead=4, contrast="blind"),
    dict(draft_answers=C_, lookahead=4, jump_forward=4),
    dict(draft_answers=C_, lookahead=4, jump_forward=4, constraints=C_),
    dict(draft_answers=C_, lookahead=4, frame_attention=True),
]


@pytest.mark.parametrize("kw", REFUSED, ids=lambda kw: " ".join(sorted(set(kw) - {"draft_answers"})) or "alone")
def test_the_keyword_refuses_before_the_engine_is_touched(kw):
    with pytest.raises(ValueError):
        generate.generate(NoEngine(), _batch(), **kw)


def test_the_rows_of_a_pass_are_bounded_and_the_stream_refuses_the_keyword():
    big = {"text_id": {"vqa": torch.ones(1100, 1, 16, dtype=torch.int64)}, "prefix_index": {"vqa": [4] * 1100}}
    with pytest.raises(ValueError, match="65535"):
        generate.generate(NoEngine(), big, lookahead=64, draft_answers=C_)         # B * R = 70400
    import llama
    m = types.SimpleNamespace(ensure_engine=lambda: pytest.fail("refused before the engine is built"))
    with pytest.raises(ValueError, match="draft_answers"):                         # the stream has no such keyword: refused where
        llama.Transformer.generate_stream(m, [_batch()], slots=2, draft_answers=C_)    # its other absent keywords are
    assert "draft_answers" not in inspect.signature(stream.generate_stream).parameters
    with pytest.raises(ValueError):                                                # lookahead alone keeps its limit of 16
        generate.generate(NoEngine(), _batch(), lookahead=17)


def test_the_ops_wrappers_refuse_host_tensors():
    z = torch.zeros(2, dtype=torch.int32)
    with pytest.raises(ValueError):
        ops.kv_tree_commit(torch.zeros(1, 2 * 8 + 1, 768), torch.zeros(1, 4, 768), torch.zeros(2, 32, dtype=torch.int32), z, z, None,
                           n_seq=2, S=8, H=2, Dh=128, A=1, cache_rotated=False)
    with pytest.raises(ValueError):
        ops.tree_spec_step(torch.zeros(2, 9), torch.zeros(9, 4), {"n_plan": z}, *([z] * 21), max_new_tokens=4)


# ------------------------------------------------------------------------------------------------ the flags
def _parse(module, argv):
    sys.path.insert(0, os.path.join(ROOT, "flipped-vqa_amd"))
    import importlib
    m = importlib.import_module(module)
    return m.get_args_parser().parse_args(argv)


def test_train_flags(tmp_path):
    f = tmp_path / "vocab.txt"
    f.write_text("yes\nno\n")
    base = ["--is_generation_task", "--lookahead", "8"]
    a = _parse("train", base + ["--gen_draft", "options"])
    assert a.gen_draft == "options" and a.lookahead == 8
    a = _parse("train", ["--is_generation_task", "--lookahead", "64", "--gen_draft", "vocab", "--answer_vocab", str(f)])
    assert a.gen_draft == "vocab" and a.lookahead == 64
    assert _parse("train", ["--lookahead", "16"]).gen_draft is None
    for bad in (["--gen_draft", "options"],                                         # no --lookahead, no generation task
                ["--is_generation_task", "--gen_draft", "options"],
                ["--lookahead", "8", "--gen_draft", "options"],
                ["--is_generation_task", "--lookahead", "1", "--gen_draft", "options"],
                ["--is_generation_task", "--lookahead", "65", "--gen_draft", "options"],
                ["--lookahead", "17"],                                              # 16 stays the limit without the flag
                base + ["--gen_draft", "vocab"],                                    # no --answer_vocab
                base + ["--gen_draft", "both"],
                base + ["--gen_draft", "options", "--num_beams", "2"],
                base + ["--gen_draft", "options", "--gen_constrain", "options"],
                base + ["--gen_draft", "options", "--contrast", "blind"],
                base + ["--gen_draft", "options", "--gen_stream", "4"],
                base + ["--gen_draft", "options", "--gen_stop_eos", "--gen_frame_attention"],
                base + ["--gen_draft", "vocab", "--answer_vocab", str(f), "--val_vocab"],
                base + ["--gen_draft", "options", "--gen_constrain", "options", "--gen_jump_forward", "4"]):
        with pytest.raises(SystemExit):
            _parse("train", bad)


def test_answer_flags(tmp_path):
    f = tmp_path / "vocab.txt"
    f.write_text("yes\nno\n")
    q = ["--question", "what ?"]
    a = _parse("answer", q + ["--options", "a", "b", "--draft", "options", "--lookahead", "33"])
    assert a.draft == "options" and a.lookahead == 33
    a = _parse("answer", q + ["--answer_vocab", str(f), "--draft", "vocab", "--lookahead", "64"])
    assert a.draft == "vocab"
    for bad in (q + ["--options", "a", "b", "--draft", "options"],                  # no --lookahead
                q + ["--draft", "options", "--lookahead", "8"],                     # no --options
                q + ["--draft", "vocab", "--lookahead", "8"],                       # no --answer_vocab
                q + ["--lookahead", "17"],
                q + ["--options", "a", "b", "--draft", "options", "--lookahead", "65"],
                q + ["--options", "a", "b", "--draft", "options", "--lookahead", "8", "--constrain"],
                q + ["--options", "a", "b", "--draft", "options", "--lookahead", "8", "--num_beams", "2"],
                q + ["--options", "a", "b", "--draft", "options", "--lookahead", "8", "--contrast", "blind"],
                q + ["--options", "a", "b", "--draft", "options", "--lookahead", "8", "--frame_attention"],
                q + ["--options", "a", "b", "--draft", "options", "--lookahead", "8", "--temperature", "0.7"],
                q + ["--answer_vocab", str(f), "--draft", "vocab", "--lookahead", "8", "--jump_forward", "4"],
                q + ["--answer_vocab", str(f), "--draft", "vocab", "--lookahead", "8", "--rank", "3"]):
        with pytest.raises(SystemExit):
            _parse("answer", bad)
