"""Constrained decoding without a GPU: the trie builder (fvqa/constrain.py) against brute force, the two rules of
include/fvqa.h (fvqa_decode_next_trie, fvqa_beam_step_trie) restated in fp64 and checked on planted cases — `allowed_of`,
`kept_set_trie` and `beam_step_trie_ref` are also the yardsticks of tests/test_constrained_gpu.py —, the two C entries exported
by both builds at ABI 18 and refusing bad operands before any launch, and the host surface (generate's keyword, the flags)."""
import ctypes as C
import os
import sys
import types

import numpy as np
import pytest
import torch

from fvqa import _lib, constrain, generate, ops
from fvqa.constrain import TokenTrie, choice_of
from tests.test_sampling_cpu import kept_set_ex, penalised

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A = C.c_void_p(256)
A2 = C.c_void_p(512)
BUILDS = [("bf16", _lib.BF16), ("f16", _lib.F16)]
NEG = float("-inf")
EOS = 2


# ------------------------------------------------------------------------------------------------ the builder
def random_sets(rng, n_samples, V=509, eos=EOS):
    """Per sample up to 12 sequences of length 0-5 with a duplicate and a sequence that is a prefix of another planted."""
    out = []
    for _ in range(n_samples):
        n = int(rng.integers(3, 11))
        seqs = [[int(t) for t in rng.choice(np.setdiff1d(np.arange(V), [eos]), size=int(rng.integers(0, 6)))] for _ in range(n)]
        longest = max(seqs, key=len)
        if len(longest) < 2:
            longest = longest + [7, 9]
            seqs.append(longest)
        seqs.insert(int(rng.integers(0, len(seqs) + 1)), list(longest[:-1]))      # a prefix of another member
        seqs.append(list(seqs[int(rng.integers(0, len(seqs)))]))                 # a duplicate
        out.append(seqs[:12])
    return out


def walk(trie, root, prefix):
    """The node reached from `root` along `prefix` through the CSR arrays (None: the path leaves the trie)."""
    at = int(root)
    for t in prefix:
        toks, kids = trie.children(at)
        hit = np.nonzero(toks == t)[0]
        if hit.size != 1:
            return None
        at = int(kids[hit[0]])
    return at


def check_against_brute_force(trie, per_sample, B, eos=EOS):
    roots = trie.roots(B)
    for b in range(B):
        members = [list(m) + [eos] for m in per_sample[b]]
        for m in members:
            for cut in range(len(m) + 1):
                prefix = m[:cut]
                node = walk(trie, roots[b], prefix)
                assert node is not None
                want = sorted({x[cut] for x in members if len(x) > cut and x[:cut] == prefix})
                toks, kids = trie.children(node)
                assert toks.tolist() == want, (b, prefix)                           # ascending token order, nothing else
                assert all(0 <= int(k) < trie.n_nodes for k in kids)
                if cut == len(m):                                                   # a leaf: no children, the lowest index
                    assert want == [] and trie.leaf_choice[node] == members.index(m)
                else:
                    assert node not in trie.leaf_choice
        assert trie.n_members[0 if trie.shared else b] == len({tuple(m) for m in members})
        assert trie.max_len[0 if trie.shared else b] == max(len(m) for m in members)


@pytest.mark.parametrize("seed", range(4))
def test_builder_against_brute_force(seed):
    rng = np.random.default_rng(seed)
    B, V = 3, 509
    sets = random_sets(rng, B, V)
    trie = TokenTrie.from_sequences(sets, EOS, V)
    assert not trie.shared and trie.root.shape == (B,) and len(set(trie.root.tolist())) == B
    for a in (trie.node_first, trie.edge_token, trie.edge_child, trie.root):
        assert a.dtype == np.int32
    assert trie.node_first.shape == (trie.n_nodes + 1,) and trie.edge_token.shape == trie.edge_child.shape == (trie.n_edges,)
    assert trie.node_first[0] == 0 and trie.node_first[-1] == trie.n_edges and (np.diff(trie.node_first) >= 0).all()
    check_against_brute_force(trie, sets, B)
    shared = TokenTrie.from_sequences(sets[0], EOS, V)
    assert shared.shared and shared.roots(B).tolist() == [int(shared.root[0])] * B
    check_against_brute_force(shared, [sets[0]] * B, B)
    # choice_of inverts the mapping: every member's tokens (+ EOS, padded with -1) -> its lowest index; a row cut short -> -1
    for tr, per in ((trie, sets), (shared, [sets[0]] * B)):
        n = max(len(s) for s in per)
        width = 7
        toks = np.full((B, n, width), -1, dtype=np.int32)
        want = np.full((B, n), -1, dtype=np.int64)
        for b in range(B):
            for k, m in enumerate(per[b]):
                toks[b, k, :len(m) + 1] = list(m) + [EOS]
                want[b, k] = [list(x) for x in per[b]].index(list(m))
        assert np.array_equal(choice_of(tr, toks), want)
        assert np.array_equal(choice_of(tr, toks[:, 0]), want[:, 0])                # (B, steps) as well
        assert np.array_equal(choice_of(tr, torch.from_numpy(toks)), want)
        cut = toks.copy()
        for b in range(B):
            for k, m in enumerate(per[b]):
                cut[b, k, len(m)] = -1                                              # the EOS never came: no leaf
        assert (choice_of(tr, cut) == -1).all()
    off = np.full((B, 1, 3), -1, dtype=np.int32)
    off[:, 0, 0] = 1                                                                # (a token no member starts with)
    assert (choice_of(trie, off) == -1).all()


def test_builder_edges_and_errors():
    t = TokenTrie.from_sequences([[]], EOS, 10)                                     # the answer is the EOS alone
    assert t.shared and t.n_nodes == 2 and t.edge_token.tolist() == [EOS] and t.leaf_choice == {1: 0} and t.max_len == [1]
    t = TokenTrie.from_sequences([[5, 6], [5], [7, 8, 9], [5, 6], []], EOS, 100)
    assert t.children(int(t.root[0]))[0].tolist() == [EOS, 5, 7] and sorted(t.leaf_choice.values()) == [0, 1, 2, 4]
    assert TokenTrie.from_sequences(np.array([[5, 6], [7, 8]]), EOS, 100).shared
    assert not TokenTrie.from_sequences([[[5, 6]], [[7], []]], EOS, 100).shared
    for bad in ([], [[], [[1, 3]]], [[[4]], []]):                                   # an empty set (whole, or one sample's)
        with pytest.raises(ValueError, match="empty"):
            TokenTrie.from_sequences(bad, EOS, 10)
    for bad in ([[3, 10]], [[-1]], [[[3]], [[4, 99]]]):                             # a token outside [0, vocab)
        with pytest.raises(ValueError, match="outside"):
            TokenTrie.from_sequences(bad, EOS, 10)
    for bad in ([[3, EOS, 4]], [[EOS]], [[[3]], [[4, EOS]]]):                       # an EOS inside a sequence
        with pytest.raises(ValueError, match="EOS"):
            TokenTrie.from_sequences(bad, EOS, 10)
    with pytest.raises(ValueError):
        TokenTrie.from_sequences([[[3]], [[4]]], EOS, 10).roots(3)                  # built for two samples


class WordIds:
    """A stand-in sp_model: one id per distinct word."""
    def __init__(self):
        self.ids = {}

    def encode(self, s):
        return [self.ids.setdefault(w, 3 + len(self.ids)) for w in s.replace(":", " :").split()]


def test_option_and_answer_helpers():
    from llama.tokenizer import Tokenizer
    tok = Tokenizer("", types.SimpleNamespace(synthetic=True, vocab_size=509))
    tok.sp_model = WordIds()
    got = constrain.encode_answers(tok, ["a red ball", "ball", ""])
    head = tok._enc("Answer: The answer is ")
    assert len(head) == 5 and got == [tok._enc("a red ball"), tok._enc("ball"), []]

    class Glue(WordIds):                                                            # an answer that merges into the prompt's tail
        def encode(self, s):
            return super().encode(s.replace("is x", "isx"))
    tok.sp_model = Glue()
    with pytest.raises(ValueError, match="changes the tokens"):
        constrain.encode_answers(tok, ["x ray"])
    # options_of cuts what match_answers cuts: from the a_token + 5 up to the EOS, or to the end of a row that holds none
    S, a_id = 16, tok.a_token_id
    ids = torch.zeros(2, 3, S, dtype=torch.int64)
    ids[:, :, 2] = a_id
    ids[0, 0, 7:10] = torch.tensor([40, 41, EOS])
    ids[0, 1, 7:9] = torch.tensor([42, EOS])
    ids[0, 2, 7] = EOS
    ids[1, :, 2], ids[1, :, 4] = 9, a_id
    ids[1, 0, 9:16] = torch.arange(50, 57)                                          # no EOS: to the end of the row
    ids[1, 1, 9:11] = torch.tensor([60, EOS])
    ids[1, 2, 9:12] = torch.tensor([61, 62, EOS])
    want = [[[40, 41], [42], []], [list(range(50, 57)), [60], [61, 62]]]
    assert constrain.options_of({"text_id": {"vqa": ids}}, tok) == want
    path = os.path.join(ROOT, "tests", "golden", "_no_such_vocab.txt")
    with pytest.raises(OSError):
        constrain.read_answer_vocab(path)


# ------------------------------------------------------------------------------------------------ the token step in fp64
def allowed_of(trie, node, V):
    """-> (allowed tokens ascending, their children), or None for a node outside [0, n_nodes) — as the kernel reads the trie:
    edge tokens outside [0, V) are skipped."""
    if not 0 <= node < trie.n_nodes:
        return None
    toks, kids = trie.children(node)
    keep = (toks >= 0) & (toks < V)
    return toks[keep].astype(np.int64), kids[keep].astype(np.int64)


def kept_set_trie(logits, allowed, R, r, T, top_k, top_p):
    """Rules 1-3 of fvqa_decode_next_ex with "every token" read as "every allowed token", fp64: the penalty on the row, then
    kept_set_ex on the allowed logits alone (their maximum, their Z, k against their number, the order (e descending, token
    ascending) — `allowed` ascends, so sub-index order is token order). -> (kept TOKENS ascending, p over the allowed tokens)."""
    allowed = np.asarray(allowed, dtype=np.int64)
    sub = penalised(logits, R, r)[allowed]
    kept, p = kept_set_ex(sub, [], 1.0, T, top_k, top_p)
    return allowed[kept], p


def pick_trie(logits, allowed, R, r, T, top_k, top_p, u):
    """Rule 4 on top: the first kept token in token order whose running kept mass exceeds u * M, else the last kept one.
    T == 0: the largest penalised allowed logit, the lowest token on ties."""
    allowed = np.asarray(allowed, dtype=np.int64)
    if T == 0:
        sub = penalised(logits, R, r)[allowed]
        return int(allowed[int(np.argmax(sub))]), 1
    kept, p = kept_set_trie(logits, allowed, R, r, T, top_k, top_p)
    pk = p[np.searchsorted(allowed, kept)]
    cdf = np.cumsum(pk)
    over = np.nonzero(cdf > u * cdf[-1])[0]
    return int(kept[over[0]] if over.size else kept[-1]), int(kept.size)


def test_token_rule_on_planted_rows():
    lg = np.array([9.0, 2.0, 1.0, 0.0, -1.0, 8.0], dtype=np.float32)
    al = [1, 2, 3, 4]                                                              # tokens 0 and 5 (the largest) are not allowed
    assert pick_trie(lg, al, [], 1.0, 0.0, 0, 1.0, 0.0) == (1, 1)
    kept, p = kept_set_trie(lg, al, [], 1.0, 1.0, 0, 1.0)
    assert kept.tolist() == al and p.sum() == pytest.approx(1.0) and p[0] == pytest.approx(1 / (1 + np.e ** -1 + np.e ** -2 + np.e ** -3))
    assert kept_set_trie(lg, al, [], 1.0, 1.0, 2, 1.0)[0].tolist() == [1, 2]
    assert kept_set_trie(lg, al, [], 1.0, 1.0, 9, 1.0)[0].tolist() == al             # top_k beyond the number allowed: off
    # e = (1, 1/e, ...) over the allowed: Z_2 = 1.3679, the mass in front of rank 1 is 0.731 of it
    assert kept_set_trie(lg, al, [], 1.0, 1.0, 2, 0.74)[0].tolist() == [1, 2]
    assert kept_set_trie(lg, al, [], 1.0, 1.0, 2, 0.72)[0].tolist() == [1]
    # the maximum is the allowed one: 100 below the row's maximum nothing underflows
    far = np.full(50, 0.0, dtype=np.float32)
    far[7], far[11], far[13] = 100.0, 0.5, 0.25
    kept, p = kept_set_trie(far, [11, 13, 20], [], 1.0, 0.5, 0, 1.0)
    assert kept.tolist() == [11, 13, 20] and p.min() > 0.1
    # the penalty reaches allowed tokens only through R, and flips the greedy pick when it should
    assert pick_trie(lg, al, [1], 1.9, 0.0, 0, 1.0, 0.0)[0] == 1 and pick_trie(lg, al, [1], 2.1, 0.0, 0, 1.0, 0.0)[0] == 2
    # the walk: u * M at the two ends, and the last kept token where nothing exceeds it
    assert pick_trie(lg, al, [], 1.0, 1.0, 0, 1.0, 0.0)[0] == 1
    assert pick_trie(lg, al, [], 1.0, 1.0, 0, 1.0, 1.0)[0] == 4
    assert pick_trie(lg, al, [], 1.0, 1.0, 3, 1.0, 1.0) == (3, 3)


def test_allowed_of_skips_what_the_kernel_skips():
    t = TokenTrie.from_sequences([[5, 6], [7], [300]], EOS, 509)
    root = int(t.root[0])
    assert allowed_of(t, root, 509)[0].tolist() == [5, 7, 300] and allowed_of(t, root, 100)[0].tolist() == [5, 7]
    assert allowed_of(t, t.n_nodes, 509) is None and allowed_of(t, -2, 509) is None
    leaf = [n for n in t.leaf_choice][0]
    assert allowed_of(t, leaf, 509)[0].size == 0


# ------------------------------------------------------------------------------------------------ the beam step in fp64
def beam_step_trie_ref(logits, score, done, pos, ids, n_generated, node, trie, *, eos_id=EOS, stop_at_eos=True):
    """tests/test_beam_cpu.py::beam_step_ref under a trie, ONE sample, fp64: a live slot at a node >= 0 offers its allowed tokens
    only (lse over the whole row), a live slot without a usable edge or at a node outside [-1, n_nodes) is finished first, a slot
    at node -1 offers every token. -> beam_step_ref's dict plus "node": a child takes the child of its edge, a carried slot its
    parent's node."""
    logits = torch.as_tensor(logits, dtype=torch.float64)
    score = torch.as_tensor(score, dtype=torch.float64)
    ids = torch.as_tensor(ids, dtype=torch.int64)
    K, V = logits.shape
    S = ids.shape[1]
    done = [bool(d) or int(p) + 1 >= S for d, p in zip(done, pos)]
    offers = []
    for j in range(K):
        al = None
        if not done[j] and int(node[j]) != -1:
            al = allowed_of(trie, int(node[j]), V)
            if al is None or al[0].size == 0:
                done[j] = True
        offers.append(al)
    vals, pars, toks, kids = [], [], [], []
    for j in range(K):
        if done[j]:
            vals.append(score[j:j + 1]); pars.append(torch.tensor([j])); toks.append(torch.tensor([-1]))
            kids.append(torch.tensor([int(node[j])]))
            continue
        l = logits[j]
        m = l.max()
        lse = m + torch.log(torch.exp(l - m).sum())
        if offers[j] is None:
            t, c = torch.arange(V), torch.full((V,), -1)
        else:
            t, c = torch.from_numpy(offers[j][0]), torch.from_numpy(offers[j][1])
        vals.append(score[j] + (l[t] - lse)); pars.append(torch.full((t.numel(),), j)); toks.append(t); kids.append(c)
    vals, pars, toks, kids = torch.cat(vals), torch.cat(pars), torch.cat(toks), torch.cat(kids)
    order = torch.sort(vals, descending=True, stable=True).indices[:K + 1]
    ranked = [(float(vals[o]), int(pars[o]), int(toks[o])) for o in order]
    out = {"parent": [], "token": [], "ids": [], "pos": [], "score": [], "done": [], "n_generated": [], "node": [],
           "ranked": ranked}
    for o in order[:K]:
        val, j, v = float(vals[o]), int(pars[o]), int(toks[o])
        row = ids[j].clone()
        if v < 0:
            out["pos"].append(int(pos[j])); out["done"].append(1); out["n_generated"].append(int(n_generated[j]))
        else:
            row[int(pos[j]) + 1] = v
            out["pos"].append(int(pos[j]) + 1)
            out["done"].append(1 if stop_at_eos and v == eos_id else 0)
            out["n_generated"].append(int(n_generated[j]) + 1)
        out["parent"].append(j); out["token"].append(v); out["ids"].append(row); out["score"].append(val)
        out["node"].append(int(kids[o]))
    out["ids"] = torch.stack(out["ids"])
    return out


def test_beam_rule_on_planted_cases():
    from tests.test_beam_cpu import beam_step_ref
    S = 8
    ids = torch.arange(3 * S).view(3, S) + 10
    t = TokenTrie.from_sequences([[5, 6], [5, 7], [8]], EOS, 12)
    root = int(t.root[0])
    n5, n8 = walk(t, root, [5]), walk(t, root, [8])
    lg = torch.zeros(3, 12, dtype=torch.float64)
    lg[0, 3], lg[0, 5], lg[0, 8] = 9.0, 2.0, 1.0                                     # token 3 is the model's favourite, not allowed
    # the first step: slot 0 offers 5 and 8 only; the empty slots offer theirs at -inf, in (parent, token) order
    r = beam_step_trie_ref(lg, [0.0, NEG, NEG], [0, 0, 0], [3, 3, 3], ids, [0, 0, 0], [root] * 3, t)
    assert r["parent"] == [0, 0, 1] and r["token"] == [5, 8, 5] and r["node"] == [n5, n8, n5]
    lse = float(torch.logsumexp(lg[0], 0))
    assert r["score"][:2] == pytest.approx([2.0 - lse, 1.0 - lse], abs=1e-12) and r["score"][2] == NEG   # lse of the WHOLE row
    assert r["done"] == [0, 0, 0] and r["pos"] == [4, 4, 4]
    # slots at different nodes; the parents swap and the nodes follow; a done slot is carried with its node
    leaf = walk(t, root, [8, EOS])
    lg2 = torch.zeros(3, 12, dtype=torch.float64)
    lg2[0, 6], lg2[0, 7] = 1.0, 3.0
    r = beam_step_trie_ref(lg2, [-3.0, -1.0, -2.0], [0, 1, 0], [4, 5, 4], ids, [1, 2, 1], [n5, leaf, n8], t)
    # (values: slot 1 carried -1.0; (0, 7) -3 + 3 - log(e + e^3 + 10) = -3.49; (2, EOS) -2 - log 12 = -4.48; (0, 6) -5.49)
    assert r["parent"] == [1, 0, 2] and r["token"] == [-1, 7, EOS] and r["node"] == [leaf, walk(t, root, [5, 7]), leaf]
    assert r["done"] == [1, 0, 1] and r["ranked"][3][1:] == (0, 6) and r["n_generated"] == [2, 2, 2]
    # a live slot at a leaf, and one at a node outside the trie, are finished first and carried with their node
    r = beam_step_trie_ref(lg2, [-1.0, -2.0, -0.5], [0, 0, 0], [4, 4, 4], ids, [1, 1, 1], [leaf, t.n_nodes + 5, n8], t)
    assert r["token"] == [-1, -1, EOS] and r["parent"] == [0, 1, 2] and r["node"] == [leaf, t.n_nodes + 5, leaf]
    assert r["score"][:2] == [-1.0, -2.0] and r["done"] == [1, 1, 1] and r["pos"] == [4, 4, 5]
    # every node -1: the rule of fvqa_beam_step
    g = torch.Generator().manual_seed(0)
    lg3 = torch.randn(3, 12, generator=g, dtype=torch.float64)
    a = beam_step_trie_ref(lg3, [-1.0, -2.0, NEG], [0, 1, 0], [4, 5, 4], ids, [1, 2, 1], [-1, -1, -1], t)
    b = beam_step_ref(lg3, [-1.0, -2.0, NEG], [0, 1, 0], [4, 5, 4], ids, [1, 2, 1], eos_id=EOS)
    for k in ("parent", "token", "pos", "score", "done", "n_generated", "ranked"):
        assert a[k] == b[k], k
    assert torch.equal(a["ids"], b["ids"]) and a["node"] == [-1, -1, -1]


# ------------------------------------------------------------------------------------------------ ABI
def _tok_args(dt, temperature=0.7, n_nodes=4, n_edges=3):
    #      logits u emb T          top_p top_k r  eos stop ids pos done gen x tok kept lp act cnt pos64 node nf et ec
    return [A, A, A, temperature, 0.9, 8, 1.2, 2, 1, A, A, A, A, A, A, A, A, A, A, A, A, A, A, A,
            n_nodes, n_edges, 3, 509, 128, 16, dt, None]                            # n_nodes n_edges B V D S dtype stream


def _beam_args(dt, n_nodes=4, n_edges=3):
    #      logits emb eos stop any ids_in ids_out pos score done ngen pos64 parent token x act counter node nf et ec
    return [A, A, 2, 1, 0, A, A2, A, A, A, A, A, A, A, A, A, A, A, A, A, A,
            n_nodes, n_edges, 2, 3, 509, 128, 16, dt, None]                         # n_nodes n_edges B K V D S dtype stream


@pytest.mark.parametrize("which,h16", BUILDS)
def test_the_trie_entries_are_exported_and_check_their_operands_on_the_host(which, h16):
    """Every call here must be refused: one that passed validation would launch a kernel on fake addresses."""
    lib = _lib.load(which)
    assert lib.fvqa_version() == _lib.ABI_VERSION == 18          # an added entry changes no signature
    tok, beam = lib.fvqa_decode_next_trie, lib.fvqa_beam_step_trie
    assert len(_tok_args(h16)) == len(_lib.SIGNATURES["fvqa_decode_next_trie"][1])
    assert len(_beam_args(h16)) == len(_lib.SIGNATURES["fvqa_beam_step_trie"][1])
    assert callable(ops.decode_next_trie) and callable(ops.beam_step_trie)
    for dt in (h16, _lib.F32):
        for fn, base, ptrs, sizes in ((tok, _tok_args(dt), (20, 21, 22, 23), (24, 25)),
                                      (beam, _beam_args(dt), (17, 18, 19, 20), (21, 22))):
            for at in ptrs:                                       # node, node_first, edge_token, edge_child
                a = list(base)
                a[at] = None
                assert fn(*a) == -1, at
                a[at] = C.c_void_p(258)                           # off its 4-byte boundary
                assert fn(*a) == -3, at
            for bad in (0, -3):
                a = list(base)
                a[sizes[0]] = bad                                 # n_nodes <= 0
                assert fn(*a) == -2, bad
            a = list(base)
            a[sizes[1]] = -1                                      # n_edges < 0 (0 is a trie of leaves)
            assert fn(*a) == -2
        # the checks of the entries they extend still hold
        a = _tok_args(dt)
        a[0] = None
        assert tok(*a) == -1
        a = _tok_args(dt)
        a[5] = -1                                                 # top_k < 0
        assert tok(*a) == -1
        a = _tok_args(dt)
        a[26] = 65536                                             # B beyond the counter's 16 bits
        assert tok(*a) == -2
        a = _tok_args(dt)
        a[1] = None                                               # sampling without u
        assert tok(*a) == -1
        a = _beam_args(dt)
        a[6] = a[5]                                               # ids_out is ids_in
        assert beam(*a) == -1
        a = _beam_args(dt)
        a[24] = 9                                                 # K > 8
        assert beam(*a) == -2
    other = _lib.F16 if h16 == _lib.BF16 else _lib.BF16
    assert tok(*_tok_args(other)) == -1 and beam(*_beam_args(other)) == -1          # the other build's 16-bit code


# ------------------------------------------------------------------------------------------------ host
def _eng():
    return types.SimpleNamespace(model=types.SimpleNamespace(tokenizer=types.SimpleNamespace(eos_id=EOS)), pack=None,
                                 device="cpu", V=509)


def _data(S=16, prefix=(10, 12)):
    return {"text_id": {"vqa": torch.zeros(len(prefix), 1, S, dtype=torch.int64)}, "prefix_index": {"vqa": list(prefix)}}


def test_generate_refuses_what_constraints_cannot_serve():
    """All refused before the engine is touched (there is none here)."""
    sets = [[5, 6], [7]]
    with pytest.raises(ValueError, match="stop_at_eos"):
        generate.generate(_eng(), _data(), constraints=sets, stop_at_eos=False)
    with pytest.raises(ValueError, match="max_new_tokens"):
        generate.generate(_eng(), _data(), constraints=sets, max_new_tokens=2)      # [5, 6, EOS] takes three steps
    with pytest.raises(ValueError, match="does not fit"):
        generate.generate(_eng(), _data(prefix=(10, 14)), constraints=sets)         # 14 + 3 > 16
    with pytest.raises(ValueError, match="does not fit"):                           # per sample: the long answer behind the long prompt
        generate.generate(_eng(), _data(prefix=(10, 14)), constraints=[[[7]], [[5, 6]]], num_beams=2)
    with pytest.raises(ValueError, match="does not fit"):
        generate.generate(_eng(), _data(prefix=(10, 14)), constraints=TokenTrie.from_sequences(sets, EOS, 509), temperature=0.8)
    with pytest.raises(ValueError, match="EOS"):
        generate.generate(_eng(), _data(), constraints=[[5, EOS]])                  # the builder's errors come through
    with pytest.raises(ValueError, match="samples"):
        generate.generate(_eng(), _data(), constraints=[[[5]], [[6]], [[7]]])       # three sets, two samples
    # what fits passes these checks and goes on to the engine (None here)
    with pytest.raises(KeyError, match="label"):                                    # (the prefill's first read of the batch)
        generate.generate(_eng(), _data(prefix=(10, 13)), constraints=sets, max_new_tokens=3)


def test_without_the_keyword_nothing_changes(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("constraints=None went to the trie")
    monkeypatch.setattr(generate, "_compiled", boom)
    eng = types.SimpleNamespace(model=None, pack=None, device="cpu")
    for kw in ({}, {"constraints": None}, {"num_beams": 1, "temperature": 0.7, "constraints": None}):
        with pytest.raises(ValueError, match="prefix_index"):    # the first thing the existing path asks for
            generate.generate(eng, {}, **kw)
    seen = {}
    monkeypatch.setattr(generate, "beam_search", lambda *a, **k: seen.update(k))
    generate.generate(eng, {}, num_beams=2)
    assert "constraints" not in seen                              # beam search is called as it was


def test_the_parsers_accept_the_flags(tmp_path):
    import train
    a = train.get_args_parser().parse_args([])
    assert a.gen_constrain is None and a.answer_vocab is None
    assert train.get_args_parser().parse_args(["--gen_constrain", "options", "--num_beams", "3"]).gen_constrain == "options"
    vocab = tmp_path / "answers.txt"
    vocab.write_text("yes\n\nno\n two words \n")
    a = train.get_args_parser().parse_args(["--gen_constrain", "vocab", "--answer_vocab", str(vocab)])
    assert a.gen_constrain == "vocab" and constrain.read_answer_vocab(a.answer_vocab) == ["yes", "no", "two words"]
    for bad in (["--gen_constrain", "vocab"], ["--gen_constrain", "words"]):
        with pytest.raises(SystemExit):
            train.get_args_parser().parse_args(bad)
    sys.path.insert(0, os.path.join(ROOT, "flipped-vqa_amd"))
    import answer
    base = ["--random_init", "--synthetic", "--question", "why"]
    a = answer.get_args_parser().parse_args(base)
    assert a.constrain is False and a.answer_vocab is None and a.gen_constrain is None
    a = answer.get_args_parser().parse_args(base + ["--options", "a", "b", "--constrain"])
    assert a.constrain is True and a.options == ["a", "b"]
    assert answer.get_args_parser().parse_args(base + ["--answer_vocab", str(vocab)]).answer_vocab == str(vocab)
    with pytest.raises(SystemExit):
        answer.get_args_parser().parse_args(base + ["--gen_constrain", "vocab"])
    # the word-hash vocabulary of a synthetic run encodes answers behind the five tokens of the bare a_text
    tok = types.SimpleNamespace(_enc=answer.WordHashVocabulary(509).encode)
    enc = constrain.encode_answers(tok, ["a red ball", "ball"])
    assert len(enc[0]) == 3 and enc[1] == enc[0][2:] and all(3 <= t < 509 for t in enc[0])
