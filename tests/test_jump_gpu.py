"""Jump-forward constrained decoding on the GPU: the token step (fvqa_trie_jump_step, csrc/jump.hip) against the numpy restatement
of tests/test_jump_cpu.py and, at T = 1, against fvqa_decode_next_trie bit for bit; then `generate(constraints=C, jump_forward=T)`
end to end on the fixtures of tests/test_beam_gpu.py: the plain constrained call's ids, token for token, in the passes
`predict_steps` names."""
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from fvqa import generate, ops, score
from fvqa.constrain import TokenTrie
from tests.test_beam_gpu import GAP, ROWS, dense_logits, eos_batch, tiny  # noqa: F401  (tiny: the fixture and its tolerance)
from tests.test_constrained_cpu import allowed_of, walk
from tests.test_constrained_gpu import logprob_bound, members_for, step_trie
from tests.test_generate_gpu import model_of
from tests.test_jump_cpu import jump_step_ref, predict_steps
from tests.test_lookahead_gpu import trimmed
from tests.test_sampling_gpu import make_emb

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
EOS = 2
S_K, D_K = 16, 128
MAX_NEW = 40
VOCABS = {509: 3.0, 32000: 6.0, 40003: 6.0}         # ragged strided tails | tests/test_sampling_gpu.py's row in LDS | beyond it
BITS = lambda t: t.contiguous().view(torch.uint8)   # noqa: E731


# ------------------------------------------------------------------------------------------------ the token step alone
def jump_trie(V):
    """One trie for every row case of a vocabulary. Root A: a 20-token chain `a`, a one-token answer `b`, and two answers that share
    c0 c1 and then part. Root W: 300 one-token answers, the largest of them V - 1 (an edge list the 256 threads wrap around).
    Behind the compiled trie, hand-made nodes no builder would emit: X0 a child outside the trie, X1 a single edge whose token is
    V, X2 two edges of which one is usable, X3 no edge, X4 / X5 single edges into X1 / X2, X6 an edge range that runs past
    n_edges. -> (TokenTrie, names: node numbers and tokens)."""
    rng = np.random.default_rng(V)
    toks = [int(t) for t in rng.choice(np.arange(3, V - 1), size=340, replace=False)]
    a, b, c, g = toks[:20], toks[20], toks[21:26], toks[26:32]
    wide = sorted(toks[40:339] + [V - 1])
    good = TokenTrie.from_sequences([[a, [b], c[:3], c[:2] + c[3:]], [[t] for t in wide]], EOS, V)
    n0, e0 = good.n_nodes, good.n_edges
    X = [n0 + i for i in range(7)]
    #        X0            X1         X2                       X3  X4            X5            X6
    extra = [[(g[0], 10 ** 6)], [(V, X[3])], [(-4, X[3]), (g[1], X[3])], [], [(g[2], X[1])], [(g[3], X[2])], [(g[4], X[3])]]
    nf, et, ec = good.node_first.tolist(), good.edge_token.tolist(), good.edge_child.tolist()
    for edges in extra:
        et += [t for t, _ in edges]
        ec += [k for _, k in edges]
        nf.append(len(et))
    nf[-1] = len(et) + 7                                           # X6's range runs past the arrays: clamped to its one edge
    trie = TokenTrie(np.asarray(nf, np.int32), np.asarray(et, np.int32), np.asarray(ec, np.int32), good.root, {}, False, EOS, V,
                     [], [])
    assert trie.n_nodes == n0 + 7 and trie.n_edges == e0 + 7
    rootA, rootW = int(good.root[0]), int(good.root[1])
    return trie, types.SimpleNamespace(a=a, b=b, c=c, g=g, wide=wide, A=rootA, W=rootW, X=X, good=good, n_nodes=trie.n_nodes)


def make_rows(T, V, seed=0):
    """Row cases for one (T, V): dicts of logits (T, V) fp32, w (T,), m, ids (S,), pos, done, ngen, node and a name."""
    rng = np.random.default_rng(1000 * T + seed)
    trie, n = jump_trie(V)
    scale = VOCABS[V]
    rows = []

    def new(name, node, prefer=None, *, m=1, pos=3, done=0, ngen=0, w=None, tie=None):
        m = min(m, T)
        lg = (scale * rng.standard_normal((T, V))).astype(np.float32)
        top = np.float32(np.abs(lg).max() + 3)
        if prefer is not None:
            lg[m - 1, prefer] = top                                # the deciding row is the LAST fed row
        for t in tie or ():
            lg[m - 1, t] = top
        wr = np.full(T, -1, dtype=np.int32)
        if w is not None:
            wr[:min(len(w), T)] = w[:T]
        r = dict(name=name, logits=lg, m=m, pos=pos, done=done, ngen=ngen, node=node, w=wr,
                 ids=rng.integers(3, 400, S_K).astype(np.int64))
        rows.append(r)
        return r

    A, W, X, a, c = n.A, n.W, n.X, n.a, n.c
    new("leaf", A, n.b)                                            # b, then the EOS by the chain (or, chain_eos == 0, not)
    new("cut", A, a[0], pos=-1)                                    # the 20-token chain: cut at T (T = 16 fills the row)
    new("branch", A, c[0])                                         # c0 c1, then two children
    new("budget", A, a[0], ngen=MAX_NEW - 2)                       # two tokens are left of max_new_tokens
    new("budget_at_the_pick", A, a[0], ngen=MAX_NEW - 1)
    new("row_end", A, a[0], pos=S_K - 3)                           # two positions are left
    new("last_position", A, a[0], pos=S_K - 2)
    new("free", -1, m=2, w=[5, 6])
    new("free_tie", -1, tie=(7, 300))
    new("edge_tie", A, tie=(a[0], n.b))
    new("child_outside", X[0], n.g[0])
    new("single_edge_outside", X[1])
    new("one_usable_of_two", X[2])
    new("no_edges", X[3])
    new("chain_to_an_edge_outside", X[4], n.g[2])
    new("chain_to_one_usable_of_two", X[5], n.g[3])
    new("clamped_range", X[6], n.g[4])
    new("node_outside", n.n_nodes)
    new("node_far_outside", n.n_nodes + 5)
    new("node_minus_two", -2)
    new("wide", W, V - 1)                                          # the last of 300 edges
    new("wide_tie", W, tie=(n.wide[3], n.wide[290]))
    new("len_T", walk(n.good, A, a[:T]), a[T], m=T, pos=5, ngen=T, w=a[:T])     # every row was fed; the last one decides
    new("two_fed", walk(n.good, A, a[:2]), a[2], m=2, pos=5, ngen=2, w=a[:2])
    new("fed_token_outside", walk(n.good, A, a[:3]), a[3], m=3, pos=5, ngen=3, w=[a[0], V + 3, a[2]])
    new("eos_pick", walk(n.good, A, [n.b]))                        # one edge, the EOS: picked, whatever the logits say
    r = new("done_row", A, a[0], done=1, pos=6)
    r["ids"][6] = V + 11                                           # ... on an id outside the vocabulary: clamped
    new("budget_spent", A, a[0], ngen=MAX_NEW)
    new("no_room", A, a[0], pos=S_K - 1)
    new("starts_at_zero", A, c[0], pos=-1)
    new("pos_minus_two", A, a[0], pos=-2)
    return rows, trie, n


def ref_of(r, trie, T, chain_eos, want_lp):
    return jump_step_ref(r["logits"], r["w"], r["m"], r["ids"], r["pos"], r["done"], r["ngen"], r["node"],
                         (trie.node_first, trie.edge_token, trie.edge_child), T=T, eos_id=EOS, max_new_tokens=MAX_NEW,
                         chain_eos=chain_eos, want_logprobs=want_lp)


def assert_cases_are_what_they_say(rows, trie, n, T, chain_eos):
    """What the row cases are there for does happen, by the restatement (no device needed)."""
    by = {r["name"]: ref_of(r, trie, T, chain_eos, False) for r in rows}
    V = rows[0]["logits"].shape[1]
    assert by["cut"]["why"] >= {"cut_at_T"} and by["cut"]["tokens"] == n.a[:T] and by["cut"]["len"] == T
    assert by["free"]["why"] == {"free"} and by["free_tie"]["why"] == {"free", "tie"} and by["free_tie"]["tokens"] == [7]
    assert "tie" in by["edge_tie"]["why"] and by["edge_tie"]["tokens"][0] == min(n.a[0], n.b)
    assert by["single_edge_outside"]["why"] == {"no_usable_edge"} == by["no_edges"]["why"]
    for k in ("node_outside", "node_far_outside", "node_minus_two"):
        assert by[k]["why"] == {"node_outside", "no_usable_edge"} and by[k]["done"] == 1 and not by[k]["tokens"]
    assert "wide" in by["wide"]["why"] and by["wide"]["tokens"][0] == V - 1 and len(n.wide) > 256
    assert by["wide_tie"]["why"] >= {"wide", "tie"} and by["wide_tie"]["tokens"][0] == n.wide[3]
    assert by["one_usable_of_two"]["tokens"] == [n.g[1]] and by["clamped_range"]["tokens"] == [n.g[4]]
    assert by["eos_pick"]["tokens"] == [EOS] and by["eos_pick"]["done"] == 1
    assert by["budget_at_the_pick"]["tokens"] == [n.a[0]] and by["budget_at_the_pick"]["done"] == 1
    assert by["last_position"]["tokens"] == [n.a[0]] and by["last_position"]["done"] == 0
    for k in ("done_row", "budget_spent", "no_room", "pos_minus_two"):
        assert by[k]["why"] == {"dead"}
    assert by["done_row"]["feed"] == [V - 1] and by["starts_at_zero"]["start"] == 0
    len_T = next(r for r in rows if r["name"] == "len_T")
    assert len_T["m"] == T and by["len_T"]["tokens"][0] == n.a[T]
    if T >= 2:
        assert by["leaf"]["why"] == ({"leaf"} if chain_eos else {"before_eos"})
        assert by["leaf"]["tokens"] == ([n.b, EOS] if chain_eos else [n.b])
        assert by["child_outside"]["why"] == {"child_outside"} and by["child_outside"]["node"] == n.n_nodes
        assert by["chain_to_an_edge_outside"]["why"] == {"edge_outside"} and by["chain_to_one_usable_of_two"]["why"] == {"branch"}
        assert "len_T" in by["len_T"]["why"] and by["two_fed"]["tokens"][0] == n.a[2]
    if T >= 3:
        assert by["branch"]["why"] == {"branch"} and by["branch"]["tokens"] == n.c[:2]
        assert by["budget"]["why"] == {"budget"} and by["budget"]["n_committed"] == 2 and by["budget"]["done"] == 1
        assert by["row_end"]["why"] == {"row_end"} and by["row_end"]["n_committed"] == 2 and by["row_end"]["done"] == 0
    if T == 16:
        assert by["len_T"]["tokens"] == n.a[16:] + ([EOS] if chain_eos else [])


def run_rows(rows, trie, T, emb, *, chain_eos, want_lp, counter=None, sync=True, nan_unread=False):
    """One launch on B = len(rows) row cases -> dict of host tensors (the in/out operands after the step included)."""
    B, V = len(rows), rows[0]["logits"].shape[1]
    t = lambda a, dt: torch.as_tensor(np.asarray(a), dtype=dt, device=DEV).contiguous()   # noqa: E731
    i32 = lambda *s: torch.full(s, -7, dtype=torch.int32, device=DEV)                      # noqa: E731
    lg = np.stack([r["logits"] for r in rows])
    if nan_unread:                                                 # the rows in front of the deciding one
        for b, r in enumerate(rows):
            lg[b, :r["m"] - 1] = np.nan
    st = dict(logits=t(lg.reshape(B * T, V), torch.float32), ids=t(np.stack([r["ids"] for r in rows]), torch.int64),
              pos=t([r["pos"] for r in rows], torch.int32), done=t([r["done"] for r in rows], torch.int32),
              ngen=t([r["ngen"] for r in rows], torch.int32), node=t([r["node"] for r in rows], torch.int32),
              w=t(np.stack([r["w"] for r in rows]), torch.int32), len=t([r["m"] for r in rows], torch.int32), start=i32(B),
              x=torch.full((B * T, emb.shape[1]), float("nan"), dtype=emb.dtype, device=DEV), token=i32(B, T),
              lp_pick=torch.full((B,), float("nan"), device=DEV), lp_fed=torch.full((B, T), float("nan"), device=DEV),
              n_committed=i32(B), n_active=i32(1),
              counter=torch.zeros(1, dtype=torch.int32, device=DEV) if counter is None else counter,
              pos64=torch.full((B,), -7, dtype=torch.int64, device=DEV))
    ops.trie_jump_step(st["logits"], emb, st["ids"], st["pos"], st["done"], st["ngen"], st["node"], st["w"], st["len"], st["start"],
                       st["x"], st["token"], st["lp_pick"], st["lp_fed"], st["n_committed"], st["n_active"], st["counter"],
                       trie.to(DEV), max_new_tokens=MAX_NEW, chain_eos=chain_eos, want_logprobs=want_lp, pos64=st["pos64"],
                       eos_id=EOS)
    if not sync:
        return st
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in st.items() if k != "logits"}


def check_rows(rows, got, trie, T, emb, *, chain_eos, want_lp):
    """Every row of a launch against the restatement; -> (rows still running, largest log-probability error, its bound)."""
    emb_h = emb.cpu()
    running, worst, bound_all = 0, 0.0, 0.0
    for b, r in enumerate(rows):
        want = ref_of(r, trie, T, chain_eos, want_lp)
        what = (r["name"], T, chain_eos, want_lp)
        nc = want["n_committed"]
        assert got["token"][b].tolist() == want["tokens"] + [-1] * (T - nc), (what, got["token"][b].tolist(), want["tokens"])
        assert int(got["n_committed"][b]) == nc, what
        assert np.array_equal(got["ids"][b].numpy(), want["ids"]), what
        assert int(got["pos"][b]) == want["pos"] and int(got["ngen"][b]) == want["n_generated"], what
        assert int(got["done"][b]) == want["done"] and int(got["node"][b]) == want["node"], what
        assert int(got["start"][b]) == want["start"] == int(got["pos64"][b]), what
        assert int(got["len"][b]) == want["len"], what
        assert got["w"][b].tolist() == want["w"], (what, got["w"][b].tolist(), want["w"])
        x = got["x"][b * T:(b + 1) * T]
        for j in range(T):
            ref = emb_h[want["feed"][j]] if j < len(want["feed"]) else torch.zeros_like(emb_h[0])
            assert torch.equal(BITS(x[j]), BITS(ref)), (what, j)
        m = r["m"]
        if want["live"]:
            ref64, bound = logprob_bound(r["logits"][m - 1])
            err = abs(float(got["lp_pick"][b]) - want["logprob_pick"])
            assert abs(want["logprob_pick"] - float(ref64[want["tokens"][0]])) < 1e-9
            worst, bound_all = max(worst, err), max(bound_all, bound)
            assert err <= bound, (what, err, bound)
        else:
            assert float(got["lp_pick"][b]) == 0.0, what
        for j in range(T):
            lp = float(got["lp_fed"][b, j])
            if want["logprob_fed"][j] != 0.0:
                _, bound = logprob_bound(r["logits"][j - 1])
                worst, bound_all = max(worst, abs(lp - want["logprob_fed"][j])), max(bound_all, bound)
                assert abs(lp - want["logprob_fed"][j]) <= bound, (what, j, lp, want["logprob_fed"][j], bound)
            else:
                assert lp == 0.0, (what, j, lp)
        running += want["done"] == 0
    return running, worst, bound_all


CASES_K = [(T, V, torch.float32) for T in (1, 4, 16) for V in VOCABS] + [(4, 509, torch.bfloat16), (4, 509, torch.float16)]


@pytest.mark.parametrize("T,V,dtype", CASES_K)
def test_jump_step_follows_the_rule(T, V, dtype):
    rows, trie, n = make_rows(T, V)
    emb = make_emb(V, D_K, dtype)
    worst = bound = 0.0
    for chain_eos, want_lp in ((True, False), (False, True), (True, True)):
        assert_cases_are_what_they_say(rows, trie, n, T, chain_eos)
        got = run_rows(rows, trie, T, emb, chain_eos=chain_eos, want_lp=want_lp)
        running, w_, b_ = check_rows(rows, got, trie, T, emb, chain_eos=chain_eos, want_lp=want_lp)
        worst, bound = max(worst, w_), max(bound, b_)
        assert int(got["n_active"]) == running and int(got["counter"]) == 0, (chain_eos, want_lp)
        if want_lp:
            fed = sum(float(v) != 0.0 for v in got["lp_fed"].flatten())
            assert fed >= (0 if T == 1 else T - 1 + 1 + 1), fed     # len_T's, two_fed's, fed_token_outside's one
        else:                                                      # the rows in front of the deciding one are never read
            nan = run_rows(rows, trie, T, emb, chain_eos=chain_eos, want_lp=False, nan_unread=True)
            for k in got:
                assert torch.equal(BITS(got[k]), BITS(nan[k])), k
    print(f"T={T} V={V} {dtype}: {len(rows)} row cases, largest log-probability error {worst:.3e} (largest bound {bound:.3e})")


@pytest.mark.parametrize("V,dtype", [(V, torch.float32) for V in VOCABS] + [(509, torch.bfloat16)])
def test_one_row_per_pass_is_decode_next_trie_bit_for_bit(V, dtype):
    """The row cases at T = 1 with the budget out of reach — rows at nodes, unconstrained rows, done rows, broken nodes, the wide
    node — through both entries."""
    rows, trie, n = make_rows(1, V)
    rows = [r for r in rows if r["ngen"] < MAX_NEW - 2]
    assert sum(r["node"] == -1 for r in rows) >= 2 and sum(r["node"] >= 0 for r in rows) >= 15
    emb = make_emb(V, D_K, dtype)
    old = step_trie(np.stack([r["logits"][0] for r in rows]), [r["node"] for r in rows], trie, emb=emb,
                    ids=np.stack([r["ids"] for r in rows]), pos=[r["pos"] for r in rows], done=[r["done"] for r in rows], S=S_K,
                    eos_id=EOS, temperature=0.0)
    new = run_rows(rows, trie, 1, emb, chain_eos=True, want_lp=False)
    for k_old, k_new in (("ids", "ids"), ("pos", "pos"), ("done", "done"), ("node", "node"), ("token", "token"),
                         ("pos64", "pos64"), ("logprob", "lp_pick")):
        a, b = torch.as_tensor(old[k_old]), new[k_new] if k_new == "ids" else new[k_new].view(len(rows))
        assert a.dtype == b.dtype and torch.equal(BITS(a), BITS(b)), (k_old, a, b)
    assert torch.equal(BITS(old["x"]), BITS(new["x"])) and old["n_active"] == int(new["n_active"])
    assert old["counter"] == 0 == int(new["counter"])
    assert int((new["token"] >= 0).sum()) >= 15 and int((new["done"] == 0).sum()) >= 10


def test_two_launches_back_to_back_on_one_counter():
    T, V = 4, 32000
    rows, trie, n = make_rows(T, V)
    emb = make_emb(V, D_K, torch.float32)
    counter = torch.zeros(1, dtype=torch.int32, device=DEV)
    a = run_rows(rows, trie, T, emb, chain_eos=False, want_lp=True, counter=counter, sync=False)   # queued with nothing between
    b = run_rows(rows, trie, T, emb, chain_eos=False, want_lp=True, counter=counter, sync=False)
    torch.cuda.synchronize()
    assert int(counter) == 0 and int(a["n_active"]) == int(b["n_active"]) == int((a["done"] == 0).sum())
    for k in a:
        assert torch.equal(BITS(a[k]), BITS(b[k])), k
    check_rows(rows, {k: v.cpu() for k, v in a.items()}, trie, T, emb, chain_eos=False, want_lp=True)


def test_the_wrapper_refuses_bad_operands():
    T, V = 4, 509
    rows, trie, n = make_rows(T, V)
    emb = make_emb(V, D_K, torch.float32)
    with pytest.raises(ValueError):
        run_rows(rows, trie, T, make_emb(V + 1, D_K, torch.float32), chain_eos=True, want_lp=False)
    rows17 = [dict(r, logits=np.zeros((17, V), np.float32), w=np.full(17, -1, np.int32)) for r in rows]
    with pytest.raises(ValueError):
        run_rows(rows17, trie, 17, emb, chain_eos=True, want_lp=False)


# ------------------------------------------------------------------------------------------------ end to end
MAX_NEW_E2E = 31
# the member sets' seeds: chosen on an MI355X so that the PLAIN constrained call alone leaves at most a quarter of the rows out
# (test_the_member_seeds_leave_few_rows_out asserts it) and so that the long members are the ones a row generates
SEEDS = {"branchy": 0, "split": 2, "long": 2, "row_end": 7}


def _tokens(rng, V, n):
    return [int(t) for t in rng.choice(np.arange(3, V), size=n, replace=False)]


def split_sets(fx, seed):
    """Per sample three members that share their first six tokens and then part three ways (tails of 1, 2 and 3 tokens)."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in fx.prefix:
        t = _tokens(rng, fx.eng.V, 12)
        out.append([t[:6] + [t[6]], t[:6] + t[7:9], t[:6] + t[9:12]])
    return out


def long_sets(fx, seed, n_long=20):
    """Per sample one member of n_long tokens beside two short ones, all with first tokens of their own."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in fx.prefix:
        t = _tokens(rng, fx.eng.V, n_long + 3)
        out.append([t[:n_long], [t[n_long]], t[n_long + 1:]])
    return out


def sets_of(fx, name):
    if name == "branchy":
        return members_for(fx, seed=SEEDS[name]), MAX_NEW_E2E       # branches at depth 0 and at depth 1
    if name == "split":
        return split_sets(fx, SEEDS[name]), MAX_NEW_E2E
    if name == "long":
        return long_sets(fx, SEEDS[name]), MAX_NEW_E2E
    n_long = 128 - max(fx.prefix) - 2                               # its EOS lands on position S - 2 of the longest prompt's row
    return long_sets(fx, SEEDS[name], n_long), n_long + 1


SET_NAMES = ("branchy", "split", "long", "row_end")


def close_rows(fx, trie, plain):
    """-> per row: did some pick of the plain call have a dense top-two gap among its ALLOWED tokens at or below GAP?"""
    dense = dense_logits(fx.eng, fx.batch, plain["ids"]).float()
    out = []
    for b, p in enumerate(fx.prefix):
        node, close = int(trie.roots(len(fx.prefix))[b]), False
        for t in range(int(plain["n_generated"][b])):
            al, kids = allowed_of(trie, node, fx.eng.V)
            tok = int(plain["ids"][b, p + t])
            if len(al) >= 2:
                top = dense[b, p - 1 + t][torch.from_numpy(al).to(dense.device)].topk(2).values
                close = close or float(top[0] - top[1]) <= GAP
            node = int(kids[al.tolist().index(tok)])
        out.append(close)
    return out


@pytest.fixture(scope="module")
def plains(tiny):  # noqa: F811
    """The plain constrained call of every member set, with its log-probabilities, once for the module."""
    out = {}
    for name in SET_NAMES:
        sets, max_new = sets_of(tiny, name)
        trie = TokenTrie.from_sequences(sets, EOS, tiny.eng.V)
        plain = generate.generate(tiny.eng, tiny.batch, temperature=0.0, constraints=trie, max_new_tokens=max_new,
                                  return_logprobs=True)
        out[name] = types.SimpleNamespace(sets=sets, trie=trie, plain=plain, max_new=max_new, close=close_rows(tiny, trie, plain))
    return out


def member_check(fx, s, out, b, what):
    """tests/test_constrained_gpu.py::test_greedy_under_five_members_per_sample's: the row is a member, `choice` names it, and
    every token is within 2 * tol of the most likely allowed token of one dense forward."""
    lp = dense_logits(fx.eng, fx.batch, out["ids"]).double().log_softmax(-1)
    p, n = fx.prefix[b], int(out["n_generated"][b])
    row = out["ids"][b, p:p + n].tolist()
    assert row[-1] == EOS and row[:-1] in s.sets[b] and s.sets[b].index(row[:-1]) == int(out["choice"][b]), what
    node = int(s.trie.roots(len(fx.prefix))[b])
    for t, tok in enumerate(row):
        al, kids = allowed_of(s.trie, node, fx.eng.V)
        at = lp[b, p - 1 + t]
        assert float(at[tok]) >= float(at[torch.from_numpy(al).to(at.device)].max()) - 2 * fx.tol, (what, t)
        node = int(kids[al.tolist().index(tok)])


def same_answer(fx, s, out, T, want_lp, what):
    plain = s.plain
    B = len(fx.prefix)
    assert set(out) == (set(plain) | {"n_committed"}) - (set() if want_lp else {"logprobs", "sum_logprob"}), what
    assert out["tokens"].dtype == out["n_committed"].dtype == torch.int32 and tuple(out["n_committed"].shape) == (B, out["steps"])
    assert torch.equal(out["n_committed"].sum(1).to(torch.int64), out["n_generated"]), what
    tk = trimmed(plain["tokens"])
    longest = 0
    for b, p in enumerate(fx.prefix):
        if s.close[b]:                                             # a one-row pass and a multi-row pass round differently
            member_check(fx, s, out, b, what)
            continue
        assert torch.equal(out["ids"][b], plain["ids"][b]) and int(out["n_generated"][b]) == int(plain["n_generated"][b]), (what, b)
        assert int(out["choice"][b]) == int(plain["choice"][b]) >= 0, (what, b)
        n = int(plain["n_generated"][b])
        assert out["tokens"][b, :n].tolist() == tk[b, :n].tolist() and bool((out["tokens"][b, n:] == -1).all()), (what, b)
        want = predict_steps(s.trie, s.trie.roots(B)[b], tk[b, :n].tolist(), T, want_lp)
        got = out["n_committed"][b].tolist()
        assert got == want + [0] * (len(got) - len(want)), (what, b, got, want)
        longest = max(longest, len(want))
    if not any(s.close):
        assert out["steps"] <= longest + 2 and out["steps"] < plain["steps"], (what, out["steps"], longest, plain["steps"])


def test_the_member_seeds_leave_few_rows_out(tiny, plains):  # noqa: F811
    left = {name: plains[name].close for name in SET_NAMES}
    total = sum(len(v) for v in left.values())
    n_left = sum(sum(v) for v in left.values())
    print(f"rows of the plain constrained call with a pick within {GAP} of a tie among its allowed tokens: {n_left} of {total} {left}")
    assert 4 * n_left <= total
    picked = {name: plains[name].plain["choice"].tolist() for name in SET_NAMES}
    print(f"members generated: {picked}")
    for name in ("long", "row_end"):                               # the long member (index 0) is generated by some row ...
        assert 0 in picked[name], (name, picked[name])
    assert picked["row_end"][int(np.argmax(tiny.prefix))] == 0     # ... in "row_end" by the row with the longest prompt
    b = int(np.argmax(tiny.prefix))
    assert tiny.prefix[b] + int(plains["row_end"].plain["n_generated"][b]) == 128 - 1       # its EOS sits at position S - 2


@pytest.mark.parametrize("T", [2, 4, 16])
@pytest.mark.parametrize("name", SET_NAMES)
def test_jump_forward_gives_the_plain_constrained_answer(tiny, plains, name, T):  # noqa: F811
    s = plains[name]
    out = generate.generate(tiny.eng, tiny.batch, temperature=0.0, constraints=s.sets, max_new_tokens=s.max_new, jump_forward=T)
    same_answer(tiny, s, out, T, False, f"{name} T={T}")
    print(f"{name} T={T}: {out['steps']} steps against the plain call's {s.plain['steps']}, committed per step "
          f"{out['n_committed'].tolist()}")


@pytest.mark.parametrize("T", [2, 4, 16])
def test_logprobs_are_the_plain_calls_and_the_dense_forwards(tiny, plains, T):  # noqa: F811
    eng, batch = tiny.eng, tiny.batch
    tol = 4.0 * tiny.tol
    full = eos_batch("tiny_peakedperm", ROWS)
    plan = score.plan_options(full["text_id"]["vqa"], full["label"]["vqa"], None, full["video_start"]["vqa"], eng.F)
    if plan.shared:     # the suffix attention reduces in another order than the one-row kernel: what that costs EXISTING code
        il = [score.score_options(eng, full, route=r)["individual_losses"].double() for r in ("shared", "dense")]
        routes = float((il[0] - il[1]).abs().max())
        tol = max(tol, 4.0 * routes)
        print(f"score_options shared route against dense on this fixture: largest per-token difference {routes:.3e}")
    print(f"per-token tolerance {tol:.3e} (4 x the fixture's {tiny.tol:.3e})")
    worst = 0.0
    for name in SET_NAMES:
        s = plains[name]
        out = generate.generate(eng, batch, temperature=0.0, constraints=s.trie, max_new_tokens=s.max_new, jump_forward=T,
                                return_logprobs=True)
        same_answer(tiny, s, out, T, True, f"logprobs {name} T={T}")
        assert tuple(out["logprobs"].shape) == tuple(out["tokens"].shape) and out["logprobs"].dtype == torch.float32
        assert bool((out["logprobs"][out["tokens"] < 0] == 0).all()) and bool((out["logprobs"][out["tokens"] >= 0] < 0).all())
        assert torch.allclose(out["sum_logprob"], out["logprobs"].sum(1), rtol=0, atol=1e-6)
        lp = dense_logits(eng, batch, out["ids"]).double().log_softmax(-1)
        for b, p in enumerate(tiny.prefix):
            for t in range(int(out["n_generated"][b])):
                got = float(out["logprobs"][b, t])
                d = abs(float(lp[b, p - 1 + t, int(out["ids"][b, p + t])]) - got)
                if not s.close[b]:
                    d = max(d, abs(float(s.plain["logprobs"][b, t]) - got))
                worst = max(worst, d)
                assert d <= tol, (name, b, t, d, tol)
    print(f"T={T}: largest difference of a log-probability to the plain call / the dense forward {worst:.3e}")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_sixteen_bit_builds(dtype):
    """Every row returns a member, `choice` names it, and every pick is the dense best allowed token wherever that gap exceeds GAP."""
    eng = model_of("tiny_peakedperm", dtype).ensure_engine()
    batch = eos_batch("tiny_peakedperm")
    fx = types.SimpleNamespace(eng=eng, batch=batch, prefix=batch["prefix_index"]["vqa"])
    B = len(fx.prefix)
    rows = left_out = 0
    for name in ("branchy", "split", "long"):
        sets, max_new = sets_of(fx, name)
        trie = TokenTrie.from_sequences(sets, EOS, eng.V)
        for T in (4, 16):
            out = generate.generate(eng, batch, temperature=0.0, constraints=sets, max_new_tokens=max_new, jump_forward=T)
            dense = dense_logits(eng, batch, out["ids"]).float()
            for b, p in enumerate(fx.prefix):
                n, c = int(out["n_generated"][b]), int(out["choice"][b])
                row = out["ids"][b, p:p + n].tolist()
                assert c >= 0 and row == sets[b][c] + [EOS] and out["tokens"][b, :n].tolist() == row, (name, T, b)
                node, close = int(trie.roots(B)[b]), False
                for t, tok in enumerate(row):
                    al, kids = allowed_of(trie, node, eng.V)
                    if len(al) >= 2:
                        top = dense[b, p - 1 + t][torch.from_numpy(al).to(dense.device)].topk(2)
                        if float(top.values[0] - top.values[1]) > GAP:
                            assert tok == int(al[int(top.indices[0])]), (name, T, b, t)
                        else:
                            close = True
                    node = int(kids[al.tolist().index(tok)])
                rows, left_out = rows + 1, left_out + close
                want = predict_steps(trie, trie.roots(B)[b], row, T, False)
                got = out["n_committed"][b].tolist()
                assert got == want + [0] * (len(got) - len(want)), (name, T, b, got, want)
    print(f"{dtype}: {rows} rows, {left_out} with a pick within {GAP} of a tie among the allowed tokens")
    assert 4 * left_out <= rows


def test_the_public_surface():
    from fvqa.constrain import options_of
    m = model_of("tiny_peakedperm", torch.float32)
    batch = eos_batch("tiny_peakedperm")
    m.args.gen_constrain = "options"
    try:
        best0, _ = m(batch, inference=True)
        g0 = m.last_generation
        m.args.gen_jump_forward = 8
        try:
            best, extracted = m(batch, inference=True)
        finally:
            del m.args.gen_jump_forward
    finally:
        del m.args.gen_constrain
    g = m.last_generation
    assert "n_committed" in g and "n_committed" not in g0 and len(extracted) == 4
    assert torch.equal(best.cpu(), best0.cpu()) and torch.equal(g["ids"], g0["ids"]) and torch.equal(g["choice"], g0["choice"])
    opts = options_of(batch, m.tokenizer)
    ans = m.generate(batch, constraints=opts, jump_forward=4)
    assert "n_committed" in m.last_generation and [ans[b] == opts[b][int(m.last_generation["choice"][b])] for b in range(4)] == [True] * 4
    m.generate(batch, constraints=opts)
    assert "n_committed" not in m.last_generation


def test_answer_cli_with_jump_forward():
    base = [sys.executable, "answer.py", "--random_init", "--synthetic", "--question", "what is the man doing", "--options",
            "a red ball", "a red car", "dancing", "--constrain"]
    seen = []
    for extra in ([], ["--jump_forward", "8"]):
        r = subprocess.run(base + extra, cwd=os.path.join(ROOT, "flipped-vqa_amd"), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        hit = re.search(r"^choice (\d): (.+)$", r.stdout, re.M)
        assert hit, r.stdout[-500:]
        seen.append((hit.group(1), hit.group(2)))
        assert ("committed per step" in r.stdout) == bool(extra), r.stdout[-500:]
    assert seen[0] == seen[1] and seen[0][1] in ("a red ball", "a red car", "dancing")
