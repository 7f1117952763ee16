"""Beam search without a GPU: the two new C entries are exported by both builds and refuse bad operands before any launch, the
rule of include/fvqa.h (fvqa_beam_step) restated in fp64 torch gives the hand-computed result on small cases, and the host
surface (keywords, flags, the dispatch of num_beams == 1 to the code that was there before) is what the documents say.
`beam_step_ref` is also the yardstick of tests/test_beam_gpu.py."""
import ctypes as C
import math
import os
import sys
import types

import pytest
import torch

from fvqa import _lib, generate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A = C.c_void_p(256)
A2 = C.c_void_p(512)
BUILDS = [("bf16", _lib.BF16), ("f16", _lib.F16)]
NEG = float("-inf")


# ------------------------------------------------------------------------------------------------ the rule, restated
def beam_step_ref(logits, score, done, pos, ids, n_generated, *, eos_id=2, stop_at_eos=True):
    """One step of the search for ONE sample, in fp64. logits (K, V), score (K,), done / pos / n_generated (K,) ints, ids (K, S).
    -> dict: parent, token (-1: carried), ids, pos, score, done, n_generated of the new slots 0..K-1, and `ranked`: the best
    K + 1 candidates as (value, parent, token) in the order (value descending, parent ascending, token ascending)."""
    logits = torch.as_tensor(logits, dtype=torch.float64)
    score = torch.as_tensor(score, dtype=torch.float64)
    ids = torch.as_tensor(ids, dtype=torch.int64)
    K, V = logits.shape
    S = ids.shape[1]
    done = [bool(d) or int(p) + 1 >= S for d, p in zip(done, pos)]           # no room: the slot is finished first
    vals, pars, toks = [], [], []
    for j in range(K):
        if done[j]:
            vals.append(score[j:j + 1]); pars.append(torch.tensor([j])); toks.append(torch.tensor([-1]))
        else:
            l = logits[j]
            m = l.max()
            lse = m + torch.log(torch.exp(l - m).sum())
            vals.append(score[j] + (l - lse)); pars.append(torch.full((V,), j)); toks.append(torch.arange(V))
    vals, pars, toks = torch.cat(vals), torch.cat(pars), torch.cat(toks)     # (already in parent, token order)
    order = torch.sort(vals, descending=True, stable=True).indices[:K + 1]   # stable: equal values keep that order
    ranked = [(float(vals[o]), int(pars[o]), int(toks[o])) for o in order]
    out = {"parent": [], "token": [], "ids": [], "pos": [], "score": [], "done": [], "n_generated": [], "ranked": ranked}
    for val, j, v in ranked[:K]:
        row = ids[j].clone()
        if v < 0:
            out["pos"].append(int(pos[j])); out["done"].append(1); out["n_generated"].append(int(n_generated[j]))
        else:
            row[int(pos[j]) + 1] = v
            out["pos"].append(int(pos[j]) + 1)
            out["done"].append(1 if stop_at_eos and v == eos_id else 0)
            out["n_generated"].append(int(n_generated[j]) + 1)
        out["parent"].append(j); out["token"].append(v); out["ids"].append(row); out["score"].append(val)
    out["ids"] = torch.stack(out["ids"])
    return out


S_, EOS = 8, 2
IDS = torch.arange(2 * S_).view(2, S_) + 10


def ref(logits, score, done=(0, 0), pos=(3, 3), ngen=(1, 1), **kw):
    return beam_step_ref(logits, score, done, pos, IDS, ngen, eos_id=EOS, **kw)


def test_the_first_step_fills_every_slot_from_slot_zero():
    p = torch.tensor([0.1, 0.4, 0.2, 0.3], dtype=torch.float64)
    r = ref(torch.stack([p.log() + 7.0, torch.zeros(4, dtype=torch.float64)]), [0.0, NEG], ngen=(0, 0))
    assert r["parent"] == [0, 0] and r["token"] == [1, 3]
    assert r["score"] == pytest.approx([math.log(0.4), math.log(0.3)], abs=1e-12)
    assert r["ranked"][2][:1] + r["ranked"][2][1:] == (pytest.approx(math.log(0.2)), 0, 2)
    want = IDS[[0, 0]].clone()
    want[0, 4], want[1, 4] = 1, 3
    assert torch.equal(r["ids"], want) and r["pos"] == [4, 4] and r["done"] == [0, 0] and r["n_generated"] == [1, 1]


def test_a_finished_slot_is_carried_past_live_candidates():
    r = ref(torch.zeros(2, 4), [-2.0, -1.0], done=(0, 1), pos=(3, 5), ngen=(2, 4))
    assert r["parent"] == [1, 0] and r["token"] == [-1, 0]                   # (uniform row: the lowest token)
    assert r["score"] == pytest.approx([-1.0, -2.0 - math.log(4.0)], abs=1e-12)
    assert torch.equal(r["ids"][0], IDS[1]) and r["pos"] == [5, 4] and r["done"] == [1, 0] and r["n_generated"] == [4, 3]
    # a live candidate that is better than the finished slot goes in front of it; an EOS child is finished
    lg = torch.tensor([[0.0, 0.0, 30.0, 0.0], [0.0, 0.0, 0.0, 0.0]])
    r = ref(lg, [-0.5, -1.0], done=(0, 1))
    assert r["parent"] == [0, 1] and r["token"] == [EOS, -1] and r["done"] == [1, 1]
    assert ref(lg, [-0.5, -1.0], done=(0, 1), stop_at_eos=False)["done"] == [0, 1]


def test_an_exact_tie_inside_a_row_goes_to_the_lower_token():
    r = ref(torch.tensor([[1.0, 3.0, 3.0, 0.0], [9.0, 9.0, 9.0, 9.0]]), [0.0, NEG])
    assert r["parent"] == [0, 0] and r["token"] == [1, 2] and r["score"][0] == r["score"][1]


def test_an_exact_tie_across_identical_parents_goes_to_the_lower_parent():
    lg = torch.tensor([[5.0, 0.0, 0.0, 0.0]] * 2)
    r = ref(lg, [-1.0, -1.0])
    assert r["parent"] == [0, 1] and r["token"] == [0, 0] and r["score"][0] == r["score"][1]
    assert r["ranked"][2][1:] == (0, 1)                                      # then (parent 0, token 1) before (0, 2), (1, 1)


def test_a_slot_out_of_room_is_finished_first():
    lg = torch.tensor([[0.0, 9.0, 0.0, 0.0], [0.0, 0.0, 0.0, 9.0]])
    r = ref(lg, [-0.5, -0.7], pos=(S_ - 1, 3), ngen=(5, 1))
    assert r["parent"] == [0, 1] and r["token"] == [-1, 3]
    assert r["score"][0] == -0.5 and r["pos"] == [S_ - 1, 4] and r["done"] == [1, 0] and r["n_generated"] == [5, 2]
    assert torch.equal(r["ids"][0], IDS[0])


# ------------------------------------------------------------------------------------------------ ABI
def _step_args(dt, K=3, V=509, B=2):
    #      logits emb eos stop any ids_in ids_out pos score done ngen pos64 parent token x act counter B K  V  D    S   dtype stream
    return [A, A, 2, 1, 0, A, A2, A, A, A, A, A, A, A, A, A, A, B, K, V, 128, 16, dt, None]


def _move_args(dt, scratch=None, dst=A, src=A2):
    #      dst  src  scratch bytes      src_seq lo hi n_dst n_src group S   D    L  A   W  dtype stream
    return [dst, src, scratch, 1 << 40, A, A, A, 6, 2, 0, 16, 256, 3, 10, 4, dt, None]


@pytest.mark.parametrize("which,h16", BUILDS)
def test_the_entries_are_exported_and_check_their_operands_on_the_host(which, h16):
    """Every call here must be refused: one that passed validation would launch a kernel on fake addresses."""
    lib = _lib.load(which)
    assert lib.fvqa_version() == _lib.ABI_VERSION == 18          # an added entry changes no signature
    step, move = lib.fvqa_beam_step, lib.fvqa_kv_beam_move
    assert len(_step_args(h16)) == len(_lib.SIGNATURES["fvqa_beam_step"][1])
    assert len(_move_args(h16)) == len(_lib.SIGNATURES["fvqa_kv_beam_move"][1])
    for dt in (h16, _lib.F32):
        base = _step_args(dt)
        for at in (0, 1) + tuple(range(5, 17)):                   # every pointer is required
            a = list(base)
            a[at] = None
            assert step(*a) == -1, at
        a = list(base)
        a[6] = a[5]                                               # ids_out is ids_in
        assert step(*a) == -1
        for K in (0, 9, -1):
            assert step(*_step_args(dt, K=K)) == -2, K
        assert step(*_step_args(dt, K=5, V=4)) == -2              # K > V
        assert step(*_step_args(dt, K=8, V=1 << 28)) == -2        # K * V does not fit an int
        for at in (17, 19, 20, 21):                               # B, V, D, S <= 0
            a = list(base)
            a[at] = 0
            assert step(*a) == -2, at
        a = list(base)
        a[0] = C.c_void_p(258)                                    # fp32 logits off their 4-byte boundary
        assert step(*a) == -3
        base = _move_args(dt)
        for at in (0, 1, 4, 5, 6):
            a = list(base)
            a[at] = None
            assert move(*a) == -1, at
        assert move(*_move_args(dt, dst=A, src=A)) == -1          # inside one cache: only through the window
        for at in (7, 8, 10, 11, 12):                             # n_dst, n_src, S, D, L <= 0
            a = list(base)
            a[at] = 0
            assert move(*a) == -2, at
        a = list(base)
        a[11] = 130 if dt != _lib.F32 else 129                    # rows that are not whole 16-byte words
        assert move(*a) == -2
        a = _move_args(dt, scratch=A, dst=A, src=A)
        assert move(*a) == -2                                     # the window serves one geometry: n_dst == n_src
        a[8] = 6
        a[14] = 0
        assert move(*a) == -2                                     # ... and has at least one row
        a[14] = 4
        a[3] = lib.fvqa_kv_beam_move_scratch(6, 4, 256, 3, dt) - 1
        assert move(*a) == -3                                     # a short window
        a = list(base)
        a[0] = C.c_void_p(264)
        assert move(*a) == -3
    assert lib.fvqa_kv_beam_move_scratch(6, 4, 256, 3, _lib.F32) == 3 * 6 * 4 * 2 * 256 * 4
    other = _lib.F16 if h16 == _lib.BF16 else _lib.BF16
    assert step(*_step_args(other)) == -1 and move(*_move_args(other)) == -1      # the other build's 16-bit code
    assert step(*_step_args(7)) == -1 and move(*_move_args(7)) == -1


# ------------------------------------------------------------------------------------------------ host
def test_generate_refuses_what_beam_search_does_not_do():
    eng = types.SimpleNamespace(model=None, pack=None, device="cpu")
    for bad in (0, 9, -1, 2.5):
        with pytest.raises(ValueError, match="num_beams"):
            generate.generate(eng, {}, num_beams=bad)
    with pytest.raises(ValueError, match="temperature"):
        generate.generate(eng, {}, num_beams=2, temperature=0.7)


def test_one_beam_is_the_code_that_was_there(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("num_beams == 1 went to the beam search")
    monkeypatch.setattr(generate, "beam_search", boom)
    eng = types.SimpleNamespace(model=None, pack=None, device="cpu")
    for kw in ({}, {"num_beams": 1}, {"num_beams": 1, "length_penalty": 1.0}, {"num_beams": 1, "temperature": 0.7}):
        with pytest.raises(ValueError, match="prefix_index"):    # the first thing the existing path asks for
            generate.generate(eng, {}, **kw)
    with pytest.raises(AssertionError, match="went to the beam search"):
        generate.generate(eng, {}, num_beams=2)


def test_the_parsers_accept_the_flags():
    import train
    a = train.get_args_parser().parse_args([])
    assert a.num_beams == 1
    assert train.get_args_parser().parse_args(["--num_beams", "4", "--is_generation_task"]).num_beams == 4
    sys.path.insert(0, os.path.join(ROOT, "flipped-vqa_amd"))
    import answer
    a = answer.get_args_parser().parse_args(["--random_init", "--synthetic", "--question", "why"])
    assert a.num_beams == 1 and a.length_penalty == 0.0
    a = answer.get_args_parser().parse_args(["--random_init", "--synthetic", "--question", "why", "--num_beams", "3",
                                             "--length_penalty", "0.7"])
    assert a.num_beams == 3 and a.length_penalty == 0.7
