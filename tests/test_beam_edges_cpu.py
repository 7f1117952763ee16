"""The helpers of tests/test_beam_edges_gpu.py (tests/beam_edges_util.py), checked without a GPU: the extended yardsticks return
what tests/test_beam_cpu.py::beam_step_ref and tests/test_constrained_cpu.py::beam_step_trie_ref return on the cases those
serve, the NaN statement gives the hand-computed answer, every case is decidable (neighbours among the best K + 1 are a planted
exact tie or GAP apart) and is what its builder says — which thread owns which winner, the tie groups, the planted winners —, the
hand-built tries are valid CSR where they are meant to be and broken exactly as stated where not, and the cache move's
reference does what the header says on cases small enough to write down."""
import math

import numpy as np
import pytest
import torch

from tests import beam_edges_util as U
from tests import test_beam_cpu, test_constrained_cpu
from tests.test_beam_gpu import GAP, STEP_SHAPES, step_case
from tests.test_constrained_gpu import beam_trie_case

NEG, NAN = U.NEG, U.NAN


def same(a, b, keys):
    for k in keys:
        if torch.is_tensor(a[k]):
            assert torch.equal(a[k], b[k]), k
        else:
            assert a[k] == b[k], k


# ------------------------------------------------------------------------------------------------ the yardstick
@pytest.mark.parametrize("B,K,V,seed", STEP_SHAPES)
def test_the_extended_reference_is_the_old_one_on_the_old_cases(B, K, V, seed):
    c, _ = step_case(B, K, V, seed)
    for b in range(B):
        sl = slice(b * K, (b + 1) * K)
        a = (c["logits"][sl].double(), c["score"][sl].double(), c["done"][sl].tolist(), c["pos"][sl].tolist(), c["ids"][sl],
             c["ngen"][sl].tolist())
        same(U.beam_step_ref(*a, eos_id=2), test_beam_cpu.beam_step_ref(*a, eos_id=2),
             ("parent", "token", "ids", "pos", "score", "done", "n_generated", "ranked"))


@pytest.mark.parametrize("K,seed", [(3, 1), (8, 2)])
def test_the_extended_trie_reference_is_the_old_one_on_the_old_cases(K, seed):
    c, node, trie = beam_trie_case(K, seed)
    for b in range(3):
        sl = slice(b * K, (b + 1) * K)
        a = (c["logits"][sl].double(), c["score"][sl].double(), c["done"][sl].tolist(), c["pos"][sl].tolist(), c["ids"][sl],
             c["ngen"][sl].tolist(), node[sl], trie)
        same(U.beam_step_trie_ref(*a, eos_id=2), test_constrained_cpu.beam_step_trie_ref(*a, eos_id=2),
             ("parent", "token", "ids", "pos", "score", "done", "n_generated", "node", "ranked"))


IDS = torch.arange(3 * 8).view(3, 8) + 10


def test_nan_by_hand_a_row_with_a_nan_offers_nothing():
    """Slot 1 (the better score) holds one NaN: its lse is NaN and none of its candidates takes part."""
    lg = torch.zeros(3, 4, dtype=torch.float64)
    lg[0] = torch.tensor([0.1, 0.4, 0.2, 0.3], dtype=torch.float64).log()
    lg[1, 2] = NAN
    r = U.beam_step_ref(lg, [-1.0, -0.5, NEG], [0, 0, 0], [3, 3, 3], IDS, [1, 1, 1], eos_id=0)
    assert r["parent"] == [0, 0, 0] and r["token"] == [1, 3, 2] and r["n_comparable"] == 4 + 4      # (slot 2: four at -inf)
    assert r["score"] == pytest.approx([-1.0 + math.log(0.4), -1.0 + math.log(0.3), -1.0 + math.log(0.2)], abs=1e-12)
    assert r["ranked"][3] == (pytest.approx(-1.0 + math.log(0.1)), 0, 0) and r["done"] == [0, 0, 0]


def test_nan_by_hand_every_row_nan_carries_every_slot():
    lg = torch.full((3, 4), NAN, dtype=torch.float64)
    ids = IDS.clone()
    ids[1, 5] = 99                                                             # (a current id past V = 4)
    r = U.beam_step_ref(lg, [-1.0, NAN, NEG], [0, 0, 0], [3, 5, -1], ids, [1, 2, 0])
    assert r["parent"] == [0, 1, 2] and r["token"] == [-1, -1, -1] and r["ranked"] == [] and r["n_comparable"] == 0
    assert r["score"][0] == -1.0 and math.isnan(r["score"][1]) and r["score"][2] == NEG
    assert torch.equal(r["ids"], ids) and r["pos"] == [3, 5, -1] and r["done"] == [1, 1, 1] and r["n_generated"] == [1, 2, 0]
    assert r["x_src"] == [3, 3, 3] and r["pos64"] == [3, 5, 0] and r["running"] == (0, 0)          # ids 13, 99, 26 -> V - 1


def test_nan_by_hand_the_missing_tail_is_the_old_slot_of_the_same_index():
    """K - 1 comparable candidates: a finished slot, one live token (the others of its row at -inf would count: the row is
    NaN instead and slot 1's finished twin carries a NaN score). New slot 2 is old slot 2 as it was."""
    lg = torch.zeros(3, 4, dtype=torch.float64)
    lg[1, 0] = NAN
    r = U.beam_step_ref(lg, [-2.0, -0.1, NAN], [1, 0, 1], [3, 3, 4], IDS, [1, 1, 7])
    assert r["n_comparable"] == 1 and r["ranked"] == [(-2.0, 0, -1)]
    assert r["parent"] == [0, 1, 2] and r["token"] == [-1, -1, -1] and r["done"] == [1, 1, 1]
    assert r["score"][:2] == [-2.0, -0.1] and math.isnan(r["score"][2]) and r["n_generated"] == [1, 1, 7]
    t = U.hand_trie([[(1, 0)]], V=4)
    r = U.beam_step_trie_ref(lg, [-2.0, -0.1, NAN], [1, 0, 1], [3, 3, 4], IDS, [1, 1, 7], [0, 0, 5], t)
    assert r["parent"] == [0, 1, 2] and r["node"] == [0, 0, 5]                 # the tail keeps its node


def test_positions_and_clamps_by_hand():
    lg = torch.zeros(3, 4, dtype=torch.float64)
    lg[0, 2] = lg[2, 1] = 9.0
    ids = IDS.clone()
    ids[1, 0] = -5
    r = U.beam_step_ref(lg, [-0.1, -0.2, -0.3], [0, 0, 0], [-1, -2, 6], ids, [0, 0, 5], eos_id=1, stop_at_eos=False)
    assert r["parent"] == [0, 1, 2] and r["token"] == [2, -1, 1] and r["done"] == [0, 1, 0]
    assert int(r["ids"][0, 0]) == 2 and int(r["ids"][2, 7]) == 1 and r["pos"] == [0, -2, 7] and r["pos64"] == [0, 0, 7]
    assert r["x_src"] == [2, 0, 1] and r["running"] == (1, 1)                  # the carried slot reads column 0: -5 -> row 0
    assert U.beam_step_ref(lg, [-0.1, -0.2, -0.3], [0, 0, 0], [-1, -2, 6], ids, [0, 0, 5], eos_id=2)["done"] == [1, 1, 0]


# ------------------------------------------------------------------------------------------------ the cases
def test_gap_is_the_older_tests_gap():
    assert U.GAP == GAP and U.NT == 256 and U.KMAX == 8


@pytest.mark.parametrize("name", U.STEP_NAMES)
def test_every_step_case_is_decidable_and_what_it_says(name):
    case = U.step_cases()[name]
    refs = U.reference(case)
    U.assert_decidable(case, refs)
    U.assert_premises(case, refs)
    K, V = case["K"], case["logits"].shape[1]
    assert 1 <= K <= U.KMAX and K <= V and case["logits"].numel() <= 400000    # a few hundred thousand logits at the most


@pytest.mark.parametrize("name", U.TRIE_NAMES)
def test_every_trie_case_is_decidable_and_what_it_says(name):
    case = U.trie_cases()[name]
    refs = U.reference(case)
    U.assert_decidable(case, refs)
    U.assert_premises(case, refs)
    assert case["logits"].shape[1] == U.V_TRIE


def test_one_slice_cases_plant_what_they_say():
    for K in (2, 5, 8):
        case = U.one_slice_case(K)
        V = case["logits"].shape[1]
        assert V == 256 * (K + 2) + 3 and len(case["expect"]) == 9
        for b, e in enumerate(case["expect"]):
            r = e["owners"][0]
            assert r == (0, 255, 2)[b // 3] and all(t % 256 == r for _, t in e["winners"] + e["absent"])
            toks = [t for _, t in e["winners"]]
            assert {0: toks == sorted(toks, reverse=True), 1: toks == sorted(toks), 2: True}[b % 3]     # rising, falling, shuffled
        assert len(range(2, V, 256)) == len(range(3, V, 256)) + 1              # thread 2 owns one element more
        shuffled = [t for _, t in case["expect"][2]["winners"]]
        assert K == 2 or (shuffled != sorted(shuffled) and shuffled != sorted(shuffled, reverse=True))
    nine = U.nine_and_one_case()
    for r, e in zip(U.reference(nine), nine["expect"]):
        assert e["owners"] == [2, 2, 2, 2, 77, 2, 2, 2] and len(e["absent"]) == 2
        assert [U.owner(nine, 0, p, t) for p, t in zip(r["parent"], r["token"])] == e["owners"]


def test_one_per_parent_cases_plant_what_they_say():
    case = U.one_per_parent_case()
    refs = U.reference(case)
    for b, r in enumerate(refs):
        assert sorted(r["parent"]) == list(range(8))                           # one winner per parent
        assert len({U.owner(case, b, p, t) for p, t in zip(r["parent"], r["token"])}) == 1
    assert refs[1]["score"][1] == refs[1]["score"][2] and refs[1]["parent"][1:3] == [2, 5]         # the twins, by number
    assert torch.equal(case["logits"][8 + 2], case["logits"][8 + 5])
    assert refs[2]["token"].count(-1) == 2 and sorted(refs[2]["parent"][i] for i in range(8) if refs[2]["token"][i] < 0) == [3, 6]


@pytest.mark.parametrize("K", [4, 8])
def test_the_tie_group_straddles_rank_k(K):
    case = U.wide_tie_case(K)
    r = U.reference(case)[0]
    group = sorted(case["ties"][0], key=lambda c: c[0] * 700 + c[1])
    assert len(group) == 2 * K
    vals = {}
    lg = case["logits"].double()
    for j, t in group:
        vals[(j, t)] = float(case["score"][j].double() + lg[j, t] - torch.logsumexp(lg[j], 0))
    assert len(set(vals.values())) == 1                                        # exactly equal in fp64 ...
    lg32 = case["logits"]
    assert len({float(case["score"][j] + (lg32[j, t] - torch.logsumexp(lg32[j], 0))) for j, t in group}) == 1   # ... and in fp32
    winners = list(zip(r["parent"], r["token"]))
    assert winners[0] not in group and winners[1:] == group[:K - 1] and r["ranked"][K][1:] == group[K - 1]
    threads = {t % 256 for _, t in group}
    assert {t // 64 for t in threads} == {0, 1, 2, 3} and {t % 64 < 32 for t in threads} == {True, False}
    assert len(threads) < len(group)                                           # some share a thread
    if K == 8:                                                                 # a thread pops two members, the lower number first
        assert [c for c in winners if c[1] == 5] == [(1, 5), (4, 5)]


def test_nan_case_is_what_it_says():
    case = U.nan_case()
    refs = U.reference(case)
    assert [4 - min(r["n_comparable"], 4) for r in refs] == [0, 4, 0, 2, 0, 0]
    assert all(p != 1 for p in refs[0]["parent"]) and all(not (p == 1) for p in refs[2]["parent"])
    assert refs[3]["n_comparable"] == 2
    assert all(math.isfinite(s) for s in refs[4]["score"]) and refs[5]["score"][2:] == [NEG, NEG]
    assert [r["running"] for r in refs][1] == (0, 0)


def test_bookkeeping_cases_are_what_they_say():
    first, free, none, past = U.bookkeeping_cases()
    r = U.reference(first)
    assert r[0]["pos"] == [0, -2, 7, 7] and r[0]["pos64"] == [0, 0, 7, 7] and r[0]["done"] == [0, 1, 0, 1]
    assert int(r[0]["ids"][0, 0]) == 20 and r[0]["x_src"][1] == int(first["ids"][1, 0])
    assert r[1]["x_src"][0] == 0 and r[1]["x_src"][2] == 299 and int(r[1]["ids"][0, int(first["pos"][4])]) == -5
    assert r[2]["running"] == (0, 1) and U.reference(free)[2]["running"] == (1, 1)                 # the two counts differ
    assert sum(x["running"][0] for x in r) != sum(x["running"][1] for x in r)
    assert none["eos"] == -1 and past["eos"] == 300 and U.reference(past)[2]["done"] == [0, 0, 0, 0]


def test_the_ticket_reference_is_the_yardstick_at_k_1():
    c = U.ticket_case(65535)
    assert c["logits"].shape == (65535, 4) and int(c["done"].sum()) == 65535 // 3
    want = U.ticket_ref(c)
    assert want["n_active"] == 65535 - 65535 // 3
    for b in list(range(0, 65535, 997)) + [65532, 65533, 65534]:
        r = U.beam_step_ref(c["logits"][b:b + 1].double(), c["score"][b:b + 1].double(), c["done"][b:b + 1].tolist(),
                            c["pos"][b:b + 1].tolist(), c["ids"][b:b + 1], c["ngen"][b:b + 1].tolist(), eos_id=-1)
        assert [int(want[k][b]) for k in ("parent", "token", "pos", "done", "ngen", "x_src")] == \
            [r["parent"][0], r["token"][0], r["pos"][0], r["done"][0], r["n_generated"][0], r["x_src"][0]]
        assert torch.equal(want["ids"][b], r["ids"][0]) and float(want["score"][b]) == pytest.approx(r["score"][0], abs=1e-12)
        assert r["ranked"][0][0] - r["ranked"][1][0] >= GAP if len(r["ranked"]) > 1 else True
    lg = c["logits"]
    assert bool((lg.sort(1).values == torch.arange(4.0)).all())                # every row a permutation: gaps of 1


# ------------------------------------------------------------------------------------------------ the tries
def test_hand_built_tries_are_valid_or_broken_as_stated():
    for case in U.long_list_cases() + [U.node_cases()]:
        assert U.is_valid_csr(case["trie"])
    t = U.long_list_cases()[0]["trie"]
    assert [len(t.children(n)[0]) for n in range(3)] == [0, 600, 2305]
    case, bad_at = U.unusable_token_case()
    t = case["trie"]
    toks, kids = t.children(1)
    assert not U.is_valid_csr(t) and sorted(bad_at) == [0, 130, 255, 256, 299]
    for at in range(300):
        assert (int(toks[at]) == bad_at[at] and int(kids[at]) == 3) if at in bad_at else (0 <= toks[at] < U.V_TRIE and kids[at] == 0)
    assert {int(x) for x in t.children(2)[0]} == {-1, U.V_TRIE, 2 ** 31 - 1}
    good = np.delete(np.asarray(toks), sorted(bad_at))
    assert bool((np.diff(good) > 0).all())                                     # the usable tokens still ascend
    first, twice = U.child_lookup_cases()
    t = first["trie"]
    toks, kids = t.children(1)
    assert t.n_nodes == 6 and len(toks) == 700 and int(kids[300]) == -3 and int(kids[600]) == 6 + 7
    assert bool((np.delete(np.asarray(kids), [300, 600]) == 0).all()) and bool((np.diff(toks) > 0).all())
    toks, kids = t.children(2)
    assert int(toks[300]) == int(toks[556]) and [int(kids[300]), int(kids[556])] == [4, 5]
    assert np.unique(np.delete(np.asarray(toks), 556)).size == 699
    assert first["expect"][0]["winners"] == [(0, int(t.children(1)[0][600])), (0, int(t.children(1)[0][300]))]


def test_the_launch_after_the_lost_children_finishes_them():
    after = U.trie_cases()["the launch after the lost children"]
    assert after["node"] == [6, 6] and after["done"].tolist() == [0, 0]
    r = U.reference(after)[0]
    assert r["token"] == [-1, -1] and r["done"] == [1, 1] and r["node"] == [6, 6]


# ------------------------------------------------------------------------------------------------ the cache move
def test_move_reference_by_hand():
    S, A, D = 4, 1, 2
    src = torch.arange(1 * (2 * S + A) * 3 * D, dtype=torch.float32).view(1, 2 * S + A, 3 * D)
    dst = -torch.ones(1, 3 * S + A, 3 * D)
    out = U.move_ref(dst, src, [1, -1, 0], [-2, 0, 3], [2, 4, 9], S=S, A=A)
    want = dst.clone()
    want[0, 0:2, D:] = src[0, S:S + 2, D:]                                     # lo < 0 -> 0
    want[0, 2 * S + 3, D:] = src[0, 3, D:]                                     # hi > S -> S
    want[0, 3 * S, D:] = src[0, 2 * S, D:]                                     # the adapter row
    assert torch.equal(out, want) and bool((out[:, :, :D] == -1).all())
    cache = torch.arange(1 * (4 * S) * 3 * D, dtype=torch.float32).view(1, 4 * S, 3 * D)
    out = U.move_ref(cache, cache, [1, 0, 0, 0], [0, 1, 0, 0], [4, 4, 4, 4], S=S, A=0, group=2, window_rows=2)
    want = cache.clone()
    want[0, 0:2, D:] = cache[0, S:S + 2, D:]                                   # a swap: both read the cache as it was; two rows
    want[0, S + 1:S + 3, D:] = cache[0, 1:3, D:]
    want[0, 3 * S:3 * S + 2, D:] = cache[0, 2 * S:2 * S + 2, D:]               # slot 3 <- slot 2 (+ the group's first slot)
    assert torch.equal(out, want)                                              # slot 2 is its own source: untouched


@pytest.mark.parametrize("name", U.MOVE_NAMES)
def test_every_move_case_moves_something_or_says_why_not(name):
    spec = U.move_cases()[name]
    dst, src, D = U.move_tensors(spec, torch.float32)
    want = U.move_want(spec, dst, src)
    n = spec.get("N", spec.get("n_dst"))
    assert len(spec["src_seq"]) == len(spec["lo"]) == len(spec["hi"]) == n
    assert torch.equal(want[:, :, :D], dst[:, :, :D])                          # the q third
    moved = not torch.equal(want, dst)
    assert moved != ("every slot its own parent" in name)
    if "window" in spec and spec["A"]:
        assert torch.equal(want[:, n * spec["S"]:], dst[:, n * spec["S"]:])    # adapter rows stay
    for dtype in (torch.float32, torch.bfloat16, torch.float16):
        d16, d48 = U.row_dims(dtype)
        assert d16 * torch.empty(0, dtype=dtype).element_size() == 16 and d48 == 3 * d16
