"""Jump-forward constrained decoding, without a GPU: the rule of include/fvqa.h (fvqa_trie_jump_step) restated in numpy —
`jump_step_ref`, the yardstick of tests/test_jump_gpu.py — and held to hand-made tries; `predict_steps`, which gives the tokens
each step commits from a row's generated path alone; the C entry exported by both builds at ABI 18 and refusing bad operands before
any launch; `generate`'s keyword, what it refuses, and the flags."""
import ctypes as C
import os
import sys
import types

import numpy as np
import pytest
import torch

from fvqa import _lib, generate, ops
from fvqa.constrain import TokenTrie
from tests.test_constrained_cpu import _data, _eng

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A = C.c_void_p(256)
BUILDS = [("bf16", _lib.BF16), ("f16", _lib.F16)]
EOS = 2


# ------------------------------------------------------------------------------------------------ the rule
def edges_of(trie, node, V):
    """(node_first, edge_token, edge_child) -> the node's clamped edge range as [(token, child)], the child clamped to n_nodes; and
    the indices of the usable ones (token inside [0, V)). None: a node outside the trie."""
    nf, et, ec = (np.asarray(a) for a in trie)
    n_nodes, n_edges = len(nf) - 1, len(et)
    if not 0 <= node < n_nodes:
        return None, []
    e0 = min(max(int(nf[node]), 0), n_edges)
    e1 = min(max(int(nf[node + 1]), e0), n_edges)
    edges = [(int(et[i]), int(ec[i]) if 0 <= int(ec[i]) < n_nodes else n_nodes) for i in range(e0, e1)]
    return edges, [i for i, (t, _) in enumerate(edges) if 0 <= t < V]


def lse64(row):
    mx = row.max()
    return float(mx + np.log(np.exp(row - mx).sum()))


def jump_step_ref(logits, w, m, ids, pos, done, n_generated, node, trie, *, T, eos_id=EOS, max_new_tokens, chain_eos=True,
                  want_logprobs=False):
    """One row of fvqa_trie_jump_step in fp64. logits (T, V); w (T,) the tokens the pass was fed; ids (S,), copied; trie: the
    arrays (node_first, edge_token, edge_child), or None. -> dict(ids, pos, done, n_generated, node, tokens, logprob_pick,
    logprob_fed (T,), n_committed, w (the row's w afterwards), len, start, feed (the token of every x_next row that is not zeros),
    live, why (what ended the step's chain, and what the pick met: the names the tests ask for))."""
    lg = np.asarray(logits, dtype=np.float64)
    V, S = lg.shape[1], len(ids)
    ids = np.array(ids, dtype=np.int64)
    w = [int(t) for t in w]
    m = min(max(int(m), 1), T)
    why = set()
    live0 = done == 0 and pos >= -1 and pos + 1 < S and n_generated < max_new_tokens
    fed = [0.0] * T
    if want_logprobs and live0:
        for j in range(1, m):
            if 0 <= w[j] < V:
                fed[j] = float(lg[j - 1, w[j]]) - lse64(lg[j - 1])
    live = live0
    row = lg[m - 1]
    cand = None
    if not live0:
        why.add("dead")
    elif node == -1:
        why.add("free")
        cand = [(t, -1) for t in range(V)]
    else:
        edges, usable = edges_of(trie, node, V) if trie is not None else (None, [])
        if edges is None:
            why.add("node_outside")
        if not usable:
            live = False
            why.add("no_usable_edge")
        else:
            cand = [edges[i] for i in usable]
            if len(edges) > 256:
                why.add("wide")
    if not live:
        at = min(max(pos, 0), S - 1)
        return dict(ids=ids, pos=pos, done=1, n_generated=n_generated, node=node, tokens=[], logprob_pick=0.0, logprob_fed=fed,
                    n_committed=0, w=[-1] * T if live0 else w, len=0, start=at, feed=[int(min(max(ids[at], 0), V - 1))],
                    live=False, why=why)
    vals = np.array([row[t] for t, _ in cand])
    k = int(np.argmax(vals))                                       # (the first of equal maxima: the lowest token / edge)
    if (vals == vals[k]).sum() > 1:
        why.add("tie")
    tok, child = cand[k]
    toks = [tok]
    lp = float(row[tok]) - lse64(row)
    pos, n_generated = pos + 1, n_generated + 1
    ids[pos] = tok
    if node != -1:
        node = child
    done = 1 if tok == eos_id or n_generated >= max_new_tokens else 0
    if "free" not in why:                                          # (a free row: no chain follows)
        while not done:
            if len(toks) >= T:
                why.add("cut_at_T")
                break
            if pos + 1 >= S:
                why.add("row_end")
                break
            edges, usable = edges_of(trie, node, V)
            if edges is None:
                why.add("child_outside")
                break
            if len(edges) != 1:
                why.add("branch" if len(edges) > 1 else "dead_end")
                break
            if not usable:
                why.add("edge_outside")
                break
            t, child = edges[0]
            if t == eos_id and not chain_eos:
                why.add("before_eos")
                break
            toks.append(t)
            pos, n_generated = pos + 1, n_generated + 1
            ids[pos] = t
            node = child
            if t == eos_id:
                done = 1
                why.add("leaf")
            elif n_generated >= max_new_tokens:
                done = 1
                why.add("budget")
    nc = len(toks)
    if m == T and T > 1:
        why.add("len_T")
    return dict(ids=ids, pos=pos, done=done, n_generated=n_generated, node=node, tokens=toks, logprob_pick=lp, logprob_fed=fed,
                n_committed=nc, w=toks + [-1] * (T - nc), len=0 if done else nc, start=pos if done else pos - nc + 1,
                feed=[toks[-1]] if done else toks, live=True, why=why)


def predict_steps(trie, root, path, T, want_logprobs):
    """The tokens each step commits for one row, from its generated path (the EOS included) alone: a step picks one token, then
    takes what the trie fixes — a node with exactly one child — up to T tokens in all; with want_logprobs the EOS is never
    chained. (The budget and the end of the row play no part: generate refuses a set that does not fit.)"""
    path = [int(t) for t in path]
    at, i, out = int(root), 0, []
    while i < len(path):
        toks, kids = trie.children(at)
        at = int(kids[toks.tolist().index(path[i])])
        i, nc = i + 1, 1
        while path[i - 1] != trie.eos_id and nc < T and i < len(path):
            toks, kids = trie.children(at)
            if len(toks) != 1 or (int(toks[0]) == trie.eos_id and want_logprobs):
                break
            assert int(toks[0]) == path[i], (path, i)
            at, i, nc = int(kids[0]), i + 1, nc + 1
        out.append(nc)
    return out


def arrays(trie):
    return trie.node_first, trie.edge_token, trie.edge_child


V_, S_ = 40, 16
SETS = [[5, 6, 7, 8], [5, 6, 7, 9, 10], [11]]                       # 5 6 7 is a chain, then a branch; 11 EOS is a chain to a leaf
TRIE = TokenTrie.from_sequences(SETS, EOS, V_)


def peaked(T, picks):
    """logits (T, V_): row j prefers picks[j] (None: nothing in particular)."""
    lg = np.full((T, V_), -1.0)
    for j, t in enumerate(picks):
        if t is not None:
            lg[j, t] = 2.0
    return lg


def step(lg, node, *, T, w=None, m=1, pos=3, done=0, ngen=0, trie=TRIE, ids=None, **kw):
    kw.setdefault("max_new_tokens", 20)
    return jump_step_ref(lg, [-1] * T if w is None else w, m, np.arange(S_) + 20 if ids is None else ids, pos, done, ngen, node,
                         None if trie is None else (arrays(trie) if isinstance(trie, TokenTrie) else trie), T=T, **kw)


def test_a_chain_runs_to_its_leaf_or_stops_in_front_of_the_eos():
    root = int(TRIE.root[0])
    r = step(peaked(4, [11]), root, T=4)
    assert r["tokens"] == [11, EOS] and r["done"] == 1 and r["why"] == {"leaf"} and r["node"] in TRIE.leaf_choice
    assert r["len"] == 0 and r["start"] == 5 and r["feed"] == [EOS] and r["w"] == [11, EOS, -1, -1] and r["pos"] == 5
    assert r["ids"][4:6].tolist() == [11, EOS] and r["n_generated"] == 2
    r = step(peaked(4, [11]), root, T=4, chain_eos=False)
    assert r["tokens"] == [11] and r["done"] == 0 and r["why"] == {"before_eos"} and r["len"] == 1 and r["start"] == 4
    again = step(peaked(4, [EOS]), r["node"], T=4, pos=r["pos"], ngen=1, w=r["w"], m=1, chain_eos=False)   # the EOS is PICKED
    assert again["tokens"] == [EOS] and again["done"] == 1 and again["node"] in TRIE.leaf_choice


def test_a_chain_is_cut_at_T_and_stops_at_a_branch():
    root = int(TRIE.root[0])
    r = step(peaked(2, [5]), root, T=2)
    assert r["tokens"] == [5, 6] and r["why"] == {"cut_at_T"} and r["done"] == 0 and r["len"] == 2 and r["start"] == 4
    assert r["feed"] == [5, 6] and r["w"] == [5, 6]
    # the next step picks on its LAST fed row: row 0 prefers a token that is not allowed, row 1 the 7
    r2 = step(peaked(2, [30, 7]), r["node"], T=2, w=r["w"], m=2, pos=r["pos"], ngen=2)
    assert r2["tokens"] == [7] and r2["why"] == {"branch", "len_T"} and r2["len"] == 1 and r2["start"] == 6
    r = step(peaked(16, [5]), root, T=16)
    assert r["tokens"] == [5, 6, 7] and r["why"] == {"branch"} and r["node"] == walk_node([5, 6, 7])
    r3 = step(peaked(16, [None, None, 9]), r["node"], T=16, w=r["w"], m=3, pos=r["pos"], ngen=3)
    assert r3["tokens"] == [9, 10, EOS] and r3["done"] == 1 and r3["why"] == {"leaf"}


def walk_node(prefix, trie=TRIE, root=None):
    at = int(trie.root[0]) if root is None else root
    for t in prefix:
        toks, kids = trie.children(at)
        at = int(kids[toks.tolist().index(t)])
    return at


def test_the_budget_and_the_end_of_the_row_inside_a_chain():
    root = int(TRIE.root[0])
    r = step(peaked(8, [5]), root, T=8, ngen=18)                                     # two tokens are left of 20
    assert r["tokens"] == [5, 6] and r["done"] == 1 and r["why"] == {"budget"} and r["len"] == 0 and r["feed"] == [6]
    r = step(peaked(8, [5]), root, T=8, ngen=19)                                     # the pick spends the budget: no chain
    assert r["tokens"] == [5] and r["done"] == 1 and r["why"] == set()
    r = step(peaked(8, [5]), root, T=8, pos=S_ - 3)                                  # positions S - 2 and S - 1 are left
    assert r["tokens"] == [5, 6] and r["pos"] == S_ - 1 and r["done"] == 0 and r["why"] == {"row_end"}
    assert r["len"] == 2 and r["start"] == S_ - 2                                    # both are fed; the row ends at its next step
    r2 = step(peaked(8, [None, 7]), r["node"], T=8, w=r["w"], m=2, pos=r["pos"], ngen=2, ids=r["ids"])
    assert not r2["live"] and r2["done"] == 1 and r2["tokens"] == [] and r2["start"] == S_ - 1 and r2["feed"] == [6]
    assert r2["w"] == r["w"] and r2["node"] == r["node"] and r2["len"] == 0          # a dead row keeps its state
    for kw in (dict(done=1), dict(ngen=20), dict(pos=S_ - 1), dict(pos=-2)):
        assert step(peaked(8, [5]), root, T=8, **kw)["why"] == {"dead"}
    r = step(peaked(8, [5]), root, T=8, pos=-1)                                      # a row that starts at position 0
    assert r["tokens"] == [5, 6, 7] and r["start"] == 0 and r["ids"][:3].tolist() == [5, 6, 7]


def test_a_free_row_a_tie_and_a_broken_trie():
    lg = peaked(4, [None, 33])
    r = step(lg, -1, T=4, m=2)                                                       # node == -1: the whole vocabulary, no chain
    assert r["tokens"] == [33] and r["node"] == -1 and r["why"] == {"free"} and r["len"] == 1
    lg[1, 17] = 2.0
    assert step(lg, -1, T=4, m=2)["tokens"] == [17] and step(lg, -1, T=4, m=2)["why"] == {"free", "tie"}
    root = int(TRIE.root[0])
    tie = peaked(4, [5])
    tie[0, 11] = 2.0                                                                 # an exact tie among the edges: the lower token
    r = step(tie, root, T=4)
    assert r["tokens"][0] == 5 and "tie" in r["why"]
    lp = step(peaked(4, [5]), root, T=4)["logprob_pick"]
    assert abs(lp - (2.0 - np.log(np.exp(2.0) + (V_ - 1) * np.exp(-1.0)))) < 1e-12   # over the WHOLE raw row, not the edges
    # hand-made arrays. node 0: edges (5 -> 1), (7 -> 9: outside); node 1: one edge whose token is V_ (outside); node 2: none
    broken = (np.array([0, 2, 3, 3]), np.array([5, 7, V_]), np.array([1, 9, 2]))
    r = step(peaked(4, [5]), 0, T=4, trie=broken)
    assert r["tokens"] == [5] and r["node"] == 1 and r["why"] == {"edge_outside"} and r["done"] == 0
    r = step(peaked(4, [5]), 1, T=4, trie=broken)                                    # ... which the next pick cannot use either
    assert not r["live"] and r["why"] == {"no_usable_edge"} and r["done"] == 1 and r["w"] == [-1] * 4 and r["node"] == 1
    r = step(peaked(4, [7]), 0, T=4, trie=broken)                                    # a child outside the trie: n_nodes
    assert r["tokens"] == [7] and r["node"] == 3 and r["why"] == {"child_outside"} and r["done"] == 0
    for node in (3, 99, -2):                                                         # a node outside the trie
        r = step(peaked(4, [7]), node, T=4, trie=broken)
        assert not r["live"] and r["why"] == {"node_outside", "no_usable_edge"} and r["node"] == node
    assert step(peaked(4, [7]), 2, T=4, trie=broken)["why"] == {"no_usable_edge"}    # a node without edges
    # several edges of which ONE is usable: left to the pick, never chained
    wide = (np.array([0, 1, 3, 3]), np.array([5, -4, 6]), np.array([1, 2, 2]))
    r = step(peaked(4, [5]), 0, T=4, trie=wide)
    assert r["tokens"] == [5] and r["why"] == {"branch"}
    assert step(peaked(4, [None]), 1, T=4, trie=wide)["tokens"] == [6]


def test_the_fed_log_probabilities_come_from_the_row_in_front():
    rng = np.random.default_rng(0)
    lg = rng.standard_normal((4, V_))
    root = int(TRIE.root[0])
    r = step(lg, walk_node([5, 6, 7]), T=4, w=[5, 6, 7, -1], m=3, pos=6, ngen=3, want_logprobs=True, chain_eos=False)
    ref = lg - np.log(np.exp(lg).sum(1, keepdims=True))
    assert r["logprob_fed"][0] == 0.0 and r["logprob_fed"][3] == 0.0
    assert abs(r["logprob_fed"][1] - ref[0, 6]) < 1e-12 and abs(r["logprob_fed"][2] - ref[1, 7]) < 1e-12
    assert abs(r["logprob_pick"] - ref[2, r["tokens"][0]]) < 1e-12 and r["tokens"][0] in (8, 9)
    assert step(lg, root, T=4, w=[5, 6, 7, -1], m=3, want_logprobs=False)["logprob_fed"] == [0.0] * 4
    assert step(lg, root, T=4, w=[5, 6, 7, -1], m=3, done=1, want_logprobs=True)["logprob_fed"] == [0.0] * 4


@pytest.mark.parametrize("T", [1, 2, 3, 16])
@pytest.mark.parametrize("want_logprobs", [False, True])
def test_predict_steps_is_what_the_rule_does(T, want_logprobs):
    """Every member of a few sets, decoded step by step with the restatement on logits that prefer the member's tokens: the
    committed counts are predict_steps' — and their number is the number of passes."""
    sets = SETS + [[12, 13, 14, 15, 16, 17, 18], [12, 13, 14, 15, 16, 17, 19], [12, 13, 14, 15, 16, 17, 20, 21], []]
    trie = TokenTrie.from_sequences(sets, EOS, V_)
    for member in sets:
        path = member + [EOS]
        node, pos, ngen, w, m, done, got = int(trie.root[0]), 3, 0, [-1] * T, 1, 0, []
        ids = np.zeros(40, dtype=np.int64)
        while not done:
            lg = peaked(T, [None] * (m - 1) + [path[ngen]])
            r = jump_step_ref(lg, w, m, ids, pos, done, ngen, node, arrays(trie), T=T, max_new_tokens=20,
                              chain_eos=not want_logprobs, want_logprobs=want_logprobs)
            got.append(r["n_committed"])
            node, pos, ngen, w, m, done, ids = r["node"], r["pos"], r["n_generated"], r["w"], r["len"], r["done"], r["ids"]
        assert ids[4:4 + ngen].tolist() == path and got == predict_steps(trie, trie.root[0], path, T, want_logprobs), (member, got)
    assert predict_steps(trie, trie.root[0], [12, 13, 14, 15, 16, 17, 20, 21, EOS], 4, False) == [4, 2, 3]
    assert predict_steps(trie, trie.root[0], [12, 13, 14, 15, 16, 17, 20, 21, EOS], 4, True) == [4, 2, 2, 1]
    assert predict_steps(trie, trie.root[0], [12, 13, 14, 15, 16, 17, 20, 21, EOS], 16, False) == [6, 3]
    assert predict_steps(trie, trie.root[0], [EOS], 16, True) == [1]


# ------------------------------------------------------------------------------------------------ the C entry
def _jump_args(dt, n_seq=3, T=4, max_new=8, n_nodes=4, n_edges=3, trie=True):
    t = A if trie else None
    #       logits emb nf et ec                     eos max_new chain lp ids pos done ngen node w len start pos64 x tok pick fed nc act cnt
    return [A, A, t, t, t, n_nodes, n_edges, 2, max_new, 1, 1, A, A, A, A, t, A, A, A, A, A, A, A, A, A, A, A,
            n_seq, T, 509, 128, 16, dt, None]                        # B T V D S dtype stream


@pytest.mark.parametrize("which,h16", BUILDS)
def test_the_entry_is_exported_and_checks_its_operands_on_the_host(which, h16):
    """Every call here must be refused: one that passed validation would launch a kernel on fake addresses."""
    lib = _lib.load(which)
    assert lib.fvqa_version() == _lib.ABI_VERSION == 18          # an added entry changes no signature
    fn = lib.fvqa_trie_jump_step
    assert len(_jump_args(h16)) == len(_lib.SIGNATURES["fvqa_trie_jump_step"][1])
    assert callable(ops.trie_jump_step)
    for dt in (h16, _lib.F32):
        base = _jump_args(dt)
        for at in (0, 1, 11, 12, 13, 14, 16, 17, 18, 20, 21, 22, 23, 24, 25, 26):        # every required pointer
            a = list(base)
            a[at] = None
            assert fn(*a) == -1, at
        for at in (2, 3, 4, 15):                                     # a trie given in part
            a = list(base)
            a[at] = None
            assert fn(*a) == -1, at
            a = list(_jump_args(dt, trie=False))
            a[at] = A
            assert fn(*a) == -1, at
        assert fn(*_jump_args(dt, trie=False, T=17)) == -2          # no trie at all is legal: the call gets as far as its sizes
        for n_seq, T, want in ((0, 4, -2), (3, 0, -2), (3, 17, -2), (65536, 1, -2), (16384, 4, -2), (4096, 16, -2)):
            assert fn(*_jump_args(dt, n_seq=n_seq, T=T)) == want, (n_seq, T)
        assert fn(*_jump_args(dt, max_new=0)) == -2
        assert fn(*_jump_args(dt, n_nodes=0)) == -2 and fn(*_jump_args(dt, n_edges=-1)) == -2
        for at in (29, 30, 31):                                      # V, D, S <= 0
            a = list(base)
            a[at] = 0
            assert fn(*a) == -2, at
        for at in (0, 2, 3, 4, 12, 13, 14, 15, 16, 17, 18, 21, 22, 23, 24, 25, 26):      # the 4-byte operands off their boundary
            a = list(base)
            a[at] = C.c_void_p(258)
            assert fn(*a) == -3, at
        for at in (11, 19):                                          # ids, pos64 off 8 bytes
            a = list(base)
            a[at] = C.c_void_p(260)
            assert fn(*a) == -3, at
        for at in (1, 20):                                           # emb, x_next off their element
            a = list(base)
            a[at] = C.c_void_p(257)
            assert fn(*a) == -3, at
    other = _lib.F16 if h16 == _lib.BF16 else _lib.BF16
    assert fn(*_jump_args(other)) == -1 and fn(*_jump_args(7)) == -1                 # the other build's 16-bit code; no code at all


# ------------------------------------------------------------------------------------------------ generate
def test_generate_refuses_what_jump_forward_cannot_serve():
    """All refused before the engine is touched (there is none here)."""
    sets = [[5, 6], [7]]
    for kw in (dict(jump_forward=4), dict(jump_forward=4, constraints=sets, temperature=0.7),
               dict(jump_forward=4, constraints=sets, num_beams=2), dict(jump_forward=2, constraints=sets, top_k=5),
               dict(jump_forward=4, constraints=sets, repetition_penalty=1.2),
               dict(jump_forward=4, constraints=sets, temperature=0.7, num_return_sequences=2),
               dict(jump_forward=4, constraints=sets, num_return_sequences=2), dict(jump_forward=4, constraints=sets, contrast="blind"),
               dict(jump_forward=4, constraints=sets, lookahead=4), dict(jump_forward=4, constraints=sets, lookahead=2),
               dict(jump_forward=17, constraints=sets), dict(jump_forward=-1, constraints=sets), dict(jump_forward=2.5, constraints=sets),
               dict(jump_forward=17), dict(jump_forward=-1)):
        with pytest.raises(ValueError):
            generate.generate(_eng(), _data(), **kw)
    with pytest.raises(ValueError, match="needs constraints"):
        generate.generate(_eng(), _data(), jump_forward=2)
    with pytest.raises(ValueError, match="stop_at_eos"):
        generate.generate(_eng(), _data(), jump_forward=4, constraints=sets, stop_at_eos=False)
    with pytest.raises(ValueError, match="65535"):
        generate.generate(_eng(), _data(S=4, prefix=(1,) * 4096), jump_forward=16, constraints=[[5]])
    with pytest.raises(ValueError, match="prefix_index"):
        generate.generate(_eng(), {}, jump_forward=4, constraints=sets)
    with pytest.raises(ValueError, match="max_new_tokens"):                         # the constraints' own refusals come through
        generate.generate(_eng(), _data(), jump_forward=4, constraints=sets, max_new_tokens=2)
    with pytest.raises(ValueError, match="does not fit"):
        generate.generate(_eng(), _data(prefix=(10, 14)), jump_forward=4, constraints=sets)
    # what can be served passes these checks and goes on to the prefill's first read of the batch
    for kw in (dict(jump_forward=2), dict(jump_forward=16, return_logprobs=True), dict(jump_forward=4, max_new_tokens=3),
               dict(jump_forward=4, constraints=TokenTrie.from_sequences(sets, EOS, 509))):
        with pytest.raises(KeyError, match="label"):
            generate.generate(_eng(), _data(prefix=(10, 13)), **{"constraints": sets, **kw})


def test_without_the_keyword_nothing_changes(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("a call without jump_forward went to the jump-forward path")
    monkeypatch.setattr(generate, "_generate_jump", boom)
    monkeypatch.setattr(ops, "trie_jump_step", boom)
    eng = types.SimpleNamespace(model=None, pack=None, device="cpu")
    for kw in ({}, {"jump_forward": 0}, {"jump_forward": 1}, {"temperature": 0.7, "jump_forward": 0}, {"lookahead": 1, "jump_forward": 1}):
        with pytest.raises(ValueError, match="prefix_index"):        # the first thing the existing path asks for
            generate.generate(eng, {}, **kw)
    for jf in (0, 1):                                               # with constraints: the plain constrained call, up to the prefill
        with pytest.raises(KeyError, match="label"):
            generate.generate(_eng(), _data(prefix=(10, 13)), constraints=[[5, 6], [7]], jump_forward=jf)
    seen = {}
    monkeypatch.setattr(generate, "beam_search", lambda *a, **k: seen.update(k))
    generate.generate(eng, {}, num_beams=2, jump_forward=1)
    assert seen and not any(k.startswith("jump") for k in seen)     # beam search is called as it was


# ------------------------------------------------------------------------------------------------ the flags
def test_the_parsers_accept_the_flags_and_refuse_what_is_not_built(tmp_path):
    import train
    assert train.get_args_parser().parse_args([]).gen_jump_forward == 0
    a = train.get_args_parser().parse_args(["--gen_constrain", "options", "--gen_jump_forward", "8", "--is_generation_task"])
    assert a.gen_jump_forward == 8 and a.gen_constrain == "options"
    vocab = tmp_path / "answers.txt"
    vocab.write_text("yes\nno\n")
    a = train.get_args_parser().parse_args(["--gen_constrain", "vocab", "--answer_vocab", str(vocab), "--gen_jump_forward", "16"])
    assert a.gen_jump_forward == 16
    a = train.get_args_parser().parse_args(["--gen_jump_forward", "1", "--num_beams", "3"])                # 1: off
    assert a.num_beams == 3 and a.gen_jump_forward == 1
    assert train.get_args_parser().parse_args(["--gen_jump_forward", "0", "--lookahead", "4"]).lookahead == 4
    con = ["--gen_constrain", "options"]
    for bad in (["--gen_jump_forward", "4"], con + ["--gen_jump_forward", "17"], con + ["--gen_jump_forward", "-2"],
                con + ["--gen_jump_forward", "4", "--num_beams", "2"], con + ["--gen_jump_forward", "4", "--contrast", "blind"],
                con + ["--gen_jump_forward", "4", "--lookahead", "4"], ["--lookahead", "4"] + con):
        with pytest.raises(SystemExit):
            train.get_args_parser().parse_args(bad)
    sys.path.insert(0, os.path.join(ROOT, "flipped-vqa_amd"))
    import answer
    base = ["--random_init", "--synthetic", "--question", "why"]
    assert answer.get_args_parser().parse_args(base).jump_forward == 0
    a = answer.get_args_parser().parse_args(base + ["--options", "a", "b", "--constrain", "--jump_forward", "8"])
    assert a.jump_forward == 8 and a.constrain is True
    assert answer.get_args_parser().parse_args(base + ["--answer_vocab", str(vocab), "--jump_forward", "2"]).jump_forward == 2
    for bad in (["--jump_forward", "4"], ["--options", "a", "b", "--jump_forward", "4"],
                ["--options", "a", "b", "--constrain", "--jump_forward", "17"],
                ["--options", "a", "b", "--constrain", "--jump_forward", "4", "--num_beams", "4"],
                ["--options", "a", "b", "--constrain", "--jump_forward", "4", "--contrast", "blind"]):
        with pytest.raises(SystemExit):
            answer.get_args_parser().parse_args(base + bad)


def test_the_model_passes_the_keyword_through(monkeypatch):
    from llama.model import Transformer
    seen = {}
    ids = torch.tensor([[7, 8, 9, EOS, 0, 0]])

    def fake(eng, data, **kw):
        seen.clear()
        seen.update(kw)
        out = {"ids": ids, "n_generated": torch.tensor([3]), "steps": 2, "tokens": ids[:, 1:4].int()}
        if "constraints" in kw:
            out["choice"] = torch.tensor([0])
        if kw.get("jump_forward", 0) > 1:
            out["n_committed"] = torch.tensor([[1, 2]])
        return out
    monkeypatch.setattr(generate, "generate", fake)
    tok = types.SimpleNamespace(eos_id=EOS, sp_model=None, a_token_id=7)
    me = types.SimpleNamespace(ensure_engine=lambda: types.SimpleNamespace(V=509), tokenizer=tok)
    data = {"prefix_index": {"vqa": [1]}, "text_id": {"vqa": torch.tensor([[[1, 7, 1, 1, 1, 1, 8, 9, EOS, 0],
                                                                            [1, 7, 1, 1, 1, 1, 8, EOS, 0, 0]]])}}
    sets = [[8, 9]]
    assert Transformer.generate.__wrapped__(me, data, max_new_tokens=3, constraints=sets, jump_forward=4) == [[8, 9]]
    assert seen == {"max_new_tokens": 3, "constraints": sets, "jump_forward": 4}
    assert set(me.last_generation) == {"ids", "n_generated", "steps", "choice", "n_committed"}
    Transformer.generate.__wrapped__(me, data, max_new_tokens=3, constraints=sets)
    assert "jump_forward" not in seen and set(me.last_generation) == {"ids", "n_generated", "steps", "choice"}       # as it was
    # the validation path: --gen_constrain options --gen_jump_forward T
    monkeypatch.setattr(generate, "match_answers", lambda model, d, i: (torch.tensor([1]), "sims", "extracted"))
    me._constrained_inference = types.MethodType(Transformer._constrained_inference, me)
    me._contrast_kw = lambda: {}
    me.args = types.SimpleNamespace(gen_constrain="options", gen_jump_forward=8)
    best, extracted = Transformer.inference.__wrapped__(me, data)
    assert seen["jump_forward"] == 8 and isinstance(seen["constraints"], TokenTrie) and seen["temperature"] == 0.0
    assert int(best[0]) == 0 and extracted == "extracted"
    assert set(me.last_generation) == {"ids", "similarities", "choice", "n_committed"}
    for off in (types.SimpleNamespace(gen_constrain="options"), types.SimpleNamespace(gen_constrain="options", gen_jump_forward=1)):
        me.args = off
        Transformer.inference.__wrapped__(me, data)
        assert "jump_forward" not in seen and set(me.last_generation) == {"ids", "similarities", "choice"}
