"""In-flight batching on the GPU: the token step (fvqa_decode_next_stream, csrc/sample.hip) bit for bit against the entries it
extends in its neutral form and on hand-made slots everywhere else, the seating launch (fvqa_slot_seat, csrc/stream.hip) and the
admission into the cache bit for bit against torch indexing, then `generate_stream` end to end on the reference-made fixtures:
every request's tokens are those of the plain `generate` call on its batch, whatever its slot, neighbours and time of arrival, in
the number of token steps and prefills `fvqa.stream.simulate` says."""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import engine
from fvqa import generate, ops, stream
from fvqa.constrain import options_of
from tests.test_beam_gpu import A_MV, S_MV, dense_logits, eos_batch, poison, tiny  # noqa: F401  (tiny: the fixture, its tolerance)
from tests.test_constrained_gpu import fan_trie, step_trie
from tests.test_eval import GOLDS, golden_batch
from tests.test_generate_gpu import CASES, DEV, DTYPES, GEN_EOS, model_of
from tests.test_sampling_gpu import assert_same_bits, make_emb, step_ex

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EOS = 2
EOS_K = [1, 3, 6, 12]                   # the greedy answer lengths of the fixtures' four samples (G["eos_k"], asserted below)
FAR = 2 ** 30                           # a budget beyond reach


# ------------------------------------------------------------------------------------------------ the token step alone
def step_stream(logits, req, budget, width, *, node=None, trie=None, emb=None, u=None, ids=None, pos=None, done=None,
                gen_start=None, S=16, D=128, dtype=torch.float32, want_logprob=True, **kw):
    """tests/test_sampling_gpu.py::step_ex through the stream entry: one launch on host arrays -> dict of host arrays; the
    requests' result arrays start as sentinels (-9 / 7.0 / -9) and come back whole."""
    lg_host = np.asarray(logits, dtype=np.float32)
    lg = torch.as_tensor(lg_host, device=DEV).clone()
    B, V = lg.shape
    N = len(budget)
    if emb is None:
        emb = make_emb(V, D, dtype)
    t = lambda a, dt: torch.as_tensor(np.asarray(a), dtype=dt, device=DEV).contiguous()   # noqa: E731
    ids = t(np.zeros((B, S)) if ids is None else ids, torch.int64)
    pos = t(np.full(B, 3) if pos is None else pos, torch.int32)
    done = t(np.zeros(B) if done is None else done, torch.int32)
    gs = t(np.zeros(B) if gen_start is None else gen_start, torch.int32)
    nd = None if node is None else t(node, torch.int32)
    x = torch.full((B, emb.shape[1]), float("nan"), dtype=emb.dtype, device=DEV)
    i32 = lambda *n: torch.full(n, -7, dtype=torch.int32, device=DEV)                    # noqa: E731
    tok, kept, act = i32(B), i32(B), i32(1)
    lp = torch.full((B,), float("nan"), dtype=torch.float32, device=DEV)
    pos64 = torch.full((B,), -7, dtype=torch.int64, device=DEV)
    counter = torch.zeros(1, dtype=torch.int32, device=DEV)
    out_tok, out_n = torch.full((N, width), -9, dtype=torch.int32, device=DEV), torch.full((N,), -9, dtype=torch.int32, device=DEV)
    out_lp = torch.full((N, width), 7.0, dtype=torch.float32, device=DEV) if want_logprob else None
    ops.decode_next_stream(lg, emb, ids, pos, done, gs, x, tok, kept, lp, act, counter, t(req, torch.int32), t(budget, torch.int32),
                           out_tok, out_n, out_logprob=out_lp, node=nd, trie=None if trie is None else trie.to(DEV),
                           u=None if u is None else t(u, torch.float32), pos64=pos64, **kw)
    torch.cuda.synchronize()
    r = {"token": tok.cpu().numpy(), "n_kept": kept.cpu().numpy(), "n_active": int(act), "ids": ids.cpu().numpy(),
         "pos": pos.cpu().numpy(), "done": done.cpu().numpy(), "x": x.cpu(), "emb": emb.cpu(), "pos64": pos64.cpu().numpy(),
         "logprob": lp.cpu().numpy(), "counter": int(counter), "logits_after": lg.cpu().numpy(),
         "out_tokens": out_tok.cpu().numpy(), "out_n_generated": out_n.cpu().numpy(),
         "out_logprob": None if out_lp is None else out_lp.cpu().numpy()}
    if nd is not None:
        r["node"] = nd.cpu().numpy()
    return r


MODES = [dict(temperature=0.0), dict(temperature=0.7, top_k=40, top_p=0.9, repetition_penalty=1.3)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("V", [509, 32000])
def test_the_neutral_form_is_decode_next_ex_bit_for_bit(V, dtype):
    """req = 0 .. B - 1 and budgets beyond reach. width 1: u laid out (1, B), every slot at its token 0 (gen_start = pos + 1).
    width 8: every slot at its token 3, so that the penalty has a span of three ids — each row's three best — to apply to; the
    eight rows of u are the same B draws."""
    B = 16
    rng = np.random.default_rng(V)
    lg = (6.0 * rng.standard_normal((B, V))).astype(np.float32)
    u = rng.random(B).astype(np.float32)
    ids = rng.integers(0, V, (B, 16))
    ids[:, 1:4] = np.argsort(-lg, axis=1)[:, :3]
    for D in (128, 36):                               # (36 elements: 16-bit rows that are no multiple of 16 bytes)
        emb = make_emb(V, D, dtype)
        for width, gs, i in ((1, 4, 0), (8, 1, 3)):
            for mode in MODES:
                kw = dict(emb=emb, ids=ids, gen_start=np.full(B, gs), eos_id=EOS, **mode)
                sampled = mode["temperature"] > 0
                old = step_ex(lg, u=u if sampled else None, **kw)
                new = step_stream(lg, np.arange(B), np.full(B, FAR), width, u=np.tile(u, (width, 1)) if sampled else None, **kw)
                assert_same_bits(old, new)            # token, n_kept, ids, pos, pos64, done, logprob, x_next, n_active
                assert new["counter"] == 0 and new["x"].dtype == dtype
                assert np.array_equal(new["logits_after"].view(np.uint32), lg.view(np.uint32))
                want_tok = np.full((B, width), -9)
                want_tok[:, i] = old["token"]
                want_lp = np.full((B, width), 7.0, dtype=np.float32)
                want_lp[:, i] = old["logprob"]
                assert np.array_equal(new["out_tokens"], want_tok) and np.array_equal(new["out_n_generated"], np.full(B, i + 1))
                assert np.array_equal(new["out_logprob"].view(np.uint32), want_lp.view(np.uint32))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("V", [509, 32000])
def test_the_neutral_form_under_a_trie_is_decode_next_trie_bit_for_bit(V, dtype):
    B = 16
    rng = np.random.default_rng(V + 1)
    lg = (6.0 * rng.standard_normal((B, V))).astype(np.float32)
    u = rng.random(B).astype(np.float32)
    ids = rng.integers(0, V, (B, 16))
    trie, roots = fan_trie(V, (1, 2, 7), 1)
    node = np.array([roots[b % 3] if b % 4 else -1 for b in range(B)])       # constrained rows beside free ones
    ids[:, 1:4] = np.argsort(-lg, axis=1)[:, :3]
    emb = make_emb(V, 36, dtype)
    for mode in MODES:
        kw = dict(emb=emb, ids=ids, gen_start=np.full(B, 1), eos_id=EOS, **mode)
        sampled = mode["temperature"] > 0
        old = step_trie(lg, node, trie, u=u if sampled else None, **kw)
        new = step_stream(lg, np.arange(B), np.full(B, FAR), 8, node=node, trie=trie, u=np.tile(u, (8, 1)) if sampled else None,
                          **kw)
        assert_same_bits(old, new)
        assert np.array_equal(old["node"], new["node"]) and new["counter"] == 0
        assert np.array_equal(new["out_tokens"][:, 3], old["token"]) and (np.delete(new["out_tokens"], 3, 1) == -9).all()


def test_bookkeeping_per_request():
    """Nine slots at different token indices of seven requests, width 5, one launch."""
    V, S, W = 509, 16, 5
    #            slot: 0       1 empty  2 req 9   3 no room  4 EOS    5 budget  6 past it  7 first   8 before its start
    req = [2, -1, 9, 0, 4, 1, 5, 3, 6]
    pos = [5, 0, 4, S - 1, 7, 6, 6, 3, 2]
    gs = [4, 0, 3, S - 2, 7, 5, 5, 4, 5]                   # token index pos + 1 - gen_start: 2, 1, 2, 2, 1, 2, 2, 0, -2
    done = [0, 1, 0, 0, 0, 0, 0, 0, 0]
    budget = [5, 3, 5, 5, 5, 2, 5]                         # request 1 ends with its third token, request 5 had two
    pick = [40, 50, 60, 70, EOS, 90, 100, 110, 120]
    lg = np.full((9, V), -1.0, dtype=np.float32)
    lg[np.arange(9), pick] = 3.0
    ids0 = np.arange(9 * S).reshape(9, S) % 400 + 3
    ids0[1] = 0
    for want_lp in (True, False):
        r = step_stream(lg, req, budget, W, ids=ids0, pos=pos, done=done, gen_start=gs, S=S, eos_id=EOS, want_logprob=want_lp)
        live = [0, 4, 5, 7]
        want_ids = ids0.copy()
        for b in live:
            want_ids[b, pos[b] + 1] = pick[b]
        assert np.array_equal(r["ids"], want_ids)
        assert r["token"].tolist() == [40, -1, -1, -1, EOS, 90, -1, 110, -1] and r["n_kept"].tolist() == [1, 0, 0, 0, 1, 1, 0, 1, 0]
        assert r["pos"].tolist() == [6, 0, 4, S - 1, 8, 7, 6, 4, 2] == r["pos64"].tolist()
        assert r["done"].tolist() == [0, 1, 1, 1, 1, 1, 1, 0, 1] and r["n_active"] == 2 and r["counter"] == 0
        want_tok, want_n = np.full((7, W), -9), np.full(7, -9)
        want_tok[2, 2], want_tok[4, 1], want_tok[1, 2], want_tok[3, 0] = 40, EOS, 90, 110
        want_n[[2, 4, 1, 3]] = [3, 2, 3, 1]
        assert np.array_equal(r["out_tokens"], want_tok) and np.array_equal(r["out_n_generated"], want_n)
        if want_lp:
            lp = np.full((7, W), 7.0, dtype=np.float32)
            lp[2, 2], lp[4, 1], lp[1, 2], lp[3, 0] = r["logprob"][[0, 4, 5, 7]]
            assert np.array_equal(r["out_logprob"].view(np.uint32), lp.view(np.uint32))
            assert (r["logprob"][live] < 0).all() and (np.delete(r["logprob"], live) == 0).all()
        emb = r["emb"]
        for b in range(9):                                  # the next input row: the token's, else the slot's current token's
            src = pick[b] if b in live else int(ids0[b, pos[b]])
            assert torch.equal(r["x"][b], emb[src]), b
    # the same slots without the EOS stop: slot 4 runs on
    r = step_stream(lg, req, budget, W, ids=ids0, pos=pos, done=done, gen_start=gs, S=S, eos_id=EOS, stop_at_eos=False)
    assert r["done"].tolist() == [0, 1, 1, 1, 0, 1, 1, 0, 1] and r["n_active"] == 3


def test_the_draw_is_read_at_token_index_and_request():
    """Two equally likely tokens per row, temperature 1: u < 0.5 walks to the lower one, u >= 0.5 to the higher. The slots stand at
    (request, token index) pairs whose entry u[i, r] says one thing while every other entry of the matrix — the slot's own index,
    [r, i], the flat index in a matrix of another pitch — says the other."""
    V, W, N, B = 509, 4, 6, 5
    req, idx = [2, 5, 1, 0, 3], [2, 2, 3, 1, 3]
    right = [i * N + r for r, i in zip(req, idx)]
    for b, (r, i) in enumerate(zip(req, idx)):
        assert not {b, r, i, r * W + i, i * W + r, b * N + r, i * N + b, i * B + r, r * N + i} - {right[b]} & set(right)
    lo, hi = 17, 300
    lg = np.full((B, V), -30.0, dtype=np.float32)
    lg[:, lo] = lg[:, hi] = 2.0
    pos, gs = np.full(B, 6), np.array([7 - i for i in idx])
    for here, elsewhere, want in ((0.75, 0.25, hi), (0.25, 0.75, lo)):
        u = np.full(W * N, elsewhere, dtype=np.float32)
        u[right] = here
        r = step_stream(lg, req, np.full(N, W), W, u=u.reshape(W, N), pos=pos, gen_start=gs, temperature=1.0, top_k=2)
        assert r["token"].tolist() == [want] * B and r["n_kept"].tolist() == [2] * B
        for b in range(B):
            assert r["out_tokens"][req[b], idx[b]] == want
        assert int((r["out_tokens"] != -9).sum()) == B


# ------------------------------------------------------------------------------------------------ seating
def seat_case(V, prefix, seed=0):
    """Five slots (0, 3, 4 free; 1 finished with request 3 still named; 2 running request 2) and a prefill of three rows."""
    S, n, M = 16, 5, 3
    g = torch.Generator().manual_seed(seed)
    d = lambda t: t.to(DEV).contiguous()                                            # noqa: E731
    ri = lambda lo, hi, *s, dt=torch.int32: torch.randint(lo, hi, s, generator=g).to(dt)    # noqa: E731
    st = {"ids": ri(3, V, n, S, dt=torch.int64), "pos": ri(0, S, n), "pos64": ri(0, S, n, dt=torch.int64),
          "done": torch.tensor([1, 1, 0, 1, 1], dtype=torch.int32), "gen_start": ri(0, S, n), "vstart": ri(0, 9, n),
          "req": torch.tensor([-1, 3, 2, -1, 0], dtype=torch.int32), "node": ri(0, 50, n), "lg": torch.randn(n, V, generator=g)}
    src = {"prompt_ids": ri(3, V, M, S, dt=torch.int64), "prefix": torch.tensor(prefix, dtype=torch.int64),
           "vstart_src": ri(10, 20, M), "logits_src": torch.randn(M, S, V, generator=g), "root": ri(100, 200, M)}
    return {k: d(v) for k, v in st.items()}, {k: d(v) for k, v in src.items()}


def seat(st, src, slot, rows, request, trie=True):
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    ops.slot_seat(slot, rows, request, src["prompt_ids"], src["prefix"], src["vstart_src"], src["logits_src"], st["ids"], st["pos"],
                  st["pos64"], st["done"], st["gen_start"], st["vstart"], st["req"], st["lg"], err,
                  root=src["root"] if trie else None, node=st["node"] if trie else None)
    torch.cuda.synchronize()
    return int(err)


def seated_state(before, src, slot, rows, request, trie=True):
    """What the launch must leave: torch indexing on copies."""
    want = {k: v.clone() for k, v in before.items()}
    for s, m, r in zip(slot, rows, request):
        p = int(src["prefix"][m])
        room = 1 <= p <= want["ids"].shape[1]
        want["ids"][s] = src["prompt_ids"][m]
        want["pos"][s] = want["pos64"][s] = p - 1 if room else 0
        want["gen_start"][s] = p if room else 0
        want["done"][s] = 0 if room else 1
        want["vstart"][s], want["req"][s] = src["vstart_src"][m], r
        if trie:
            want["node"][s] = src["root"][m]
        if room:
            want["lg"][s] = src["logits_src"][m, p - 1]
    return want


def assert_state(got, want):
    for k in want:
        assert torch.equal(got[k].view(torch.uint8), want[k].view(torch.uint8)), k


@pytest.mark.parametrize("V", [509, 32000])            # 2036-byte logits rows: the scalar path | rows of whole 16-byte words
def test_seating_two_of_five_slots(V):
    for trie in (True, False):
        st, src = seat_case(V, [5, 16, 9])
        before = {k: v.clone() for k, v in st.items()}
        assert seat(st, src, [3, 1], [2, 0], [7, 4], trie) == 0       # swapped order; slot 1's tenant had finished
        assert_state(st, seated_state(before, src, [3, 1], [2, 0], [7, 4], trie))
        assert st["done"].tolist() == [1, 0, 0, 0, 1] and st["pos"].tolist()[3] == 8 and st["req"].tolist() == [-1, 4, 2, 7, 0]
    # a logits matrix off the 16-byte boundary goes the scalar way
    st, src = seat_case(V, [5, 16, 9], seed=1)
    pad = torch.zeros(src["logits_src"].numel() + 1, device=DEV)
    pad[1:] = src["logits_src"].reshape(-1)
    src["logits_src"] = pad[1:].view(3, 16, V)
    before = {k: v.clone() for k, v in st.items()}
    assert seat(st, src, [0, 4], [1, 2], [8, 9]) == 0
    assert_state(st, seated_state(before, src, [0, 4], [1, 2], [8, 9]))


def test_an_occupied_slot_and_a_slot_outside_the_batch_are_refused():
    st, src = seat_case(509, [5, 16, 9])
    before = {k: v.clone() for k, v in st.items()}
    assert seat(st, src, [2, 9], [0, 1], [7, 4]) == 1                 # slot 2 runs request 2; there is no slot 9
    assert_state(st, before)
    assert seat(st, src, [0, -1], [5, 1], [7, 4]) == 1                # no source row 5, no slot -1
    assert_state(st, before)
    assert seat(st, src, [2, 4], [0, 1], [7, 4]) == 1                 # the entry beside a refused one is seated
    assert_state(st, seated_state(before, src, [4], [1], [4]))
    with pytest.raises(ValueError, match="twice"):
        seat(st, src, [0, 0], [0, 1], [7, 4])


def test_a_prefix_without_room_ends_the_request_at_once():
    st, src = seat_case(509, [0, 16, 17])
    before = {k: v.clone() for k, v in st.items()}
    assert seat(st, src, [0, 3, 4], [0, 1, 2], [5, 6, 7]) == 0
    assert_state(st, seated_state(before, src, [0, 3, 4], [0, 1, 2], [5, 6, 7]))
    assert st["done"].tolist() == [1, 1, 0, 0, 1] and st["pos"].tolist()[3] == 15       # prefix == S is seated: the step finds no room
    assert torch.equal(st["lg"][0], before["lg"][0]) and torch.equal(st["lg"][4], before["lg"][4])
    # ... and the token step ends all three with zero tokens
    r = step_stream(st["lg"].cpu().numpy(), st["req"].cpu().numpy(), np.full(8, 5), 5, ids=st["ids"].cpu().numpy(),
                    pos=st["pos"].cpu().numpy(), done=st["done"].cpu().numpy(), gen_start=st["gen_start"].cpu().numpy(), S=16)
    assert r["done"].tolist()[0] == r["done"].tolist()[3] == r["done"].tolist()[4] == 1
    assert (r["out_tokens"][5:8] == -9).all() and (r["out_n_generated"][5:8] == -9).all()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_admission_into_the_cache(dtype):
    """The kv_beam_move call of the loop: slots 3 and 1 of five take rows [0, prefix) of prefill rows 0 and 1, every other slot has
    lo = hi = 0. The adapter rows travel with every direct move (they are the same in every prefill): they are made equal here, so
    that every row outside the two prefixes must come back as it was."""
    L, D, n, M = 2, 128, 5, 2
    assert S_MV == 16
    src, cache = poison(L, M, D, dtype, 1), poison(L, n, D, dtype, 2)
    src[:, M * S_MV:] = cache[:, n * S_MV:]
    before = cache.clone()
    prefix = {3: (0, 11), 1: (1, 16)}                                  # slot: (prefill row, prefix)
    src_seq, hi = [0] * n, [0] * n
    for s, (m, p) in prefix.items():
        src_seq[s], hi[s] = m, p
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)     # noqa: E731
    ops.kv_beam_move(cache, src, i32(src_seq), i32([0] * n), i32(hi), S=S_MV, A=A_MV)
    torch.cuda.synchronize()
    want = before.clone()
    for s, (m, p) in prefix.items():
        want[:, s * S_MV:s * S_MV + p, D:] = src[:, m * S_MV:m * S_MV + p, D:]
    assert torch.equal(cache.view(torch.uint8), want.view(torch.uint8))
    for s, (m, p) in prefix.items():                                   # (the comparison above, said again per claim)
        assert torch.equal(cache[:, s * S_MV:s * S_MV + p, D:].view(torch.uint8), src[:, m * S_MV:m * S_MV + p, D:].view(torch.uint8))
        assert torch.equal(cache[:, s * S_MV + p:(s + 1) * S_MV].view(torch.uint8),
                           before[:, s * S_MV + p:(s + 1) * S_MV].view(torch.uint8))
    for s in (0, 2, 4):
        assert torch.equal(cache[:, s * S_MV:(s + 1) * S_MV].view(torch.uint8), before[:, s * S_MV:(s + 1) * S_MV].view(torch.uint8))


# ------------------------------------------------------------------------------------------------ end to end
_PLAIN = {}


def take(b, rows):
    """The rows `rows` of a fixture batch (tests/test_beam_gpu.py::eos_batch on any batch)."""
    idx = torch.tensor(rows)
    return {"video": b["video"][idx], "text_id": {"vqa": b["text_id"]["vqa"][idx]}, "label": {"vqa": b["label"]["vqa"][idx]},
            "video_start": {"vqa": [b["video_start"]["vqa"][i] for i in rows]},
            "prefix_index": {"vqa": [b["prefix_index"]["vqa"][i] for i in rows]}, "vid": [b["vid"][i] for i in rows]}


def plain(pname, dtype, rows=None, **kw):
    """The plain generate() call on the fixture's batch (greedy, EOS stop), once per set of keywords for the whole module."""
    key = (pname, dtype, None if rows is None else tuple(rows), tuple(sorted(kw.items())))
    if key not in _PLAIN:
        eng = model_of(pname, dtype).ensure_engine()
        _PLAIN[key] = generate.generate(eng, eos_batch(pname, rows), temperature=0.0, stop_at_eos=True, **kw)
    return _PLAIN[key]


def assert_request_is_the_plain_rows(out, r, ref, b, budget=31):
    n = int(ref["n_generated"][b])
    assert int(out["n_generated"][r]) == n <= budget, (r, b)
    assert out["tokens"][r, :n].tolist() == ref["tokens"][b, :n].tolist(), (r, b)
    assert bool((out["tokens"][r, n:] == -1).all()), (r, b)
    assert torch.equal(out["ids"][r], ref["ids"][b]), (r, b)


@pytest.mark.parametrize("pname,dtype", CASES)
def test_greedy_stream_is_the_plain_call_per_request(pname, dtype):
    eng = model_of(pname, dtype).ensure_engine()
    G = GEN_EOS[pname[:pname.rindex("_peaked")]]
    assert G["eos_k"].tolist() == EOS_K
    batch = eos_batch(pname)
    ref = plain(pname, dtype)
    out = stream.generate_stream(eng, [batch] * 3, slots=4, admit=2)
    assert tuple(out["tokens"].shape) == (12, 31) and out["tokens"].dtype == torch.int32 and out["n_generated"].dtype == torch.int64
    ids = out["ids"].cpu().numpy()
    for r in range(12):
        b = r % 4
        assert_request_is_the_plain_rows(out, r, ref, b)
        end = G["prefix_vqa"][b] + G["eos_k"][b]
        assert int(out["n_generated"][r]) == G["eos_k"][b] and ids[r, end - 1] == EOS
        assert np.array_equal(ids[r, :end], G["ids_after"][b, :end]) and np.array_equal(ids[r, end:], G["text_id_vqa"][b, 0, end:])
    steps, n_prefills, seated = stream.simulate(EOS_K * 3, 4, 2)
    assert (out["steps"], out["n_prefills"], out["seated"]) == (steps, n_prefills, seated) and (steps, n_prefills) == (29, 6)
    assert out["steps"] < 3 * ref["steps"] and out["occupancy"] == 66 / (4 * 29)
    print(f"{pname} {dtype}: 12 requests in {out['steps']} token steps and {out['n_prefills']} prefills of 2, occupancy "
          f"{out['occupancy']:.3f}; three plain batches: {3 * ref['steps']} steps, 3 prefills of 4")


@pytest.mark.parametrize("pname,dtype", CASES)
def test_reversed_order_three_slots_one_at_a_time(pname, dtype):
    eng = model_of(pname, dtype).ensure_engine()
    ref = plain(pname, dtype)
    out = stream.generate_stream(eng, [eos_batch(pname, [3, 2, 1, 0])] * 3, slots=3, admit=1)
    for r in range(12):
        assert_request_is_the_plain_rows(out, r, ref, 3 - r % 4)
    assert (out["steps"], out["n_prefills"]) == (30, 12) == stream.simulate(EOS_K[::-1] * 3, 3, 1)[:2]
    assert out["seated"] == stream.simulate(EOS_K[::-1] * 3, 3, 1)[2]


@pytest.mark.parametrize("pname,dtype", [CASES[0], CASES[3]])
def test_budgets(pname, dtype):
    eng = model_of(pname, dtype).ensure_engine()
    batch = eos_batch(pname)
    out = stream.generate_stream(eng, [batch] * 3, slots=4, admit=2, max_new_tokens=4)
    ref = plain(pname, dtype, max_new_tokens=4)
    assert tuple(out["tokens"].shape) == (12, 4)
    for r in range(12):
        assert_request_is_the_plain_rows(out, r, ref, r % 4, 4)
    assert out["n_generated"].tolist() == [1, 3, 4, 4] * 3
    assert (out["steps"], out["n_prefills"]) == (16, 6) == stream.simulate([1, 3, 4, 4] * 3, 4, 2)[:2]
    budgets = [2, 31, 3, 5, 31, 1, 31, 2, 4, 2, 6, 12]             # cut short, out of reach, and exactly an answer's length
    out = stream.generate_stream(eng, [batch] * 3, slots=4, admit=2, max_new_tokens=budgets)
    assert tuple(out["tokens"].shape) == (12, 31)
    for r, bud in enumerate(budgets):
        assert_request_is_the_plain_rows(out, r, plain(pname, dtype, max_new_tokens=bud), r % 4, bud)
    lengths = [min(bud, EOS_K[r % 4]) for r, bud in enumerate(budgets)]
    assert out["n_generated"].tolist() == lengths
    assert (out["steps"], out["n_prefills"], out["seated"]) == stream.simulate(lengths, 4, 2)


def test_sampled_requests_do_not_depend_on_order_slot_or_neighbours(tiny, monkeypatch):  # noqa: F811
    """tiny with its random LM head (near-flat logits: a draw decides every token), fp32: eight requests — the fixture's four
    samples twice, budgets of 2 to 8 tokens — in two orders through the same four slots, the uniforms and budgets permuted to
    follow. Tokens equal, log-probabilities bitwise equal, and within the tiny fixture's tolerance of a teacher-forced dense
    forward of each request's ids."""
    eng = model_of("tiny", torch.float32).ensure_engine()
    kw = dict(slots=4, admit=2, temperature=1.0, top_p=0.95, top_k=50, repetition_penalty=1.2, return_logprobs=True)
    rows_a, budgets_a = [0, 1, 2, 3, 0, 1, 2, 3], [8, 3, 5, 8, 2, 8, 6, 4]
    perm = [5, 2, 7, 0, 3, 6, 1, 4]
    rows_b, budgets_b = [rows_a[p] for p in perm], [budgets_a[p] for p in perm]
    batch_a, batch_b = take(golden_batch(GOLDS["tiny"]), rows_a), take(golden_batch(GOLDS["tiny"]), rows_b)
    # the draws are generate()'s: one torch.rand(W, N) from a generator seeded once
    seen = []
    real = ops.decode_next_stream
    monkeypatch.setattr(ops, "decode_next_stream", lambda *a, **k: (seen.append(k["u"]), real(*a, **k))[1])
    a = stream.generate_stream(eng, batch_a, seed=5, max_new_tokens=budgets_a, **kw)
    monkeypatch.setattr(ops, "decode_next_stream", real)
    gen = torch.Generator(device=DEV)
    gen.manual_seed(5)
    u_a = torch.rand(8, 8, dtype=torch.float32, device=DEV, generator=gen)
    assert len(seen) == a["steps"] and all(torch.equal(u, u_a) for u in seen)
    again = stream.generate_stream(eng, batch_a, seed=5, max_new_tokens=budgets_a, **kw)
    for k in ("tokens", "n_generated", "ids", "logprobs", "sum_logprob"):
        assert torch.equal(a[k], again[k]), k                     # two runs with one seed: the same bits
    assert a["seated"] == again["seated"] and a["steps"] == again["steps"]
    other = stream.generate_stream(eng, batch_a, seed=6, max_new_tokens=budgets_a, **kw)
    assert not torch.equal(a["tokens"], other["tokens"])
    u_b = u_a[:, perm].contiguous()
    monkeypatch.setattr(torch, "rand", lambda *s, **k: u_b)
    b = stream.generate_stream(eng, batch_b, seed=5, max_new_tokens=budgets_b, **kw)
    monkeypatch.undo()
    print("seated (step, slot, request), first order:", a["seated"], "second order:", b["seated"])
    for j, q in enumerate(perm):                                   # request j of the second order is request q of the first
        n = int(a["n_generated"][q])
        assert int(b["n_generated"][j]) == n and b["tokens"][j].tolist() == a["tokens"][q].tolist(), (j, q)
        assert torch.equal(b["logprobs"][j].view(torch.int32), a["logprobs"][q].view(torch.int32)), (j, q)
        assert torch.equal(b["ids"][j], a["ids"][q])
    lp = dense_logits(eng, batch_a, a["ids"]).double().log_softmax(-1)
    worst, total = 0.0, 0
    for q, p in enumerate(batch_a["prefix_index"]["vqa"]):
        n = int(a["n_generated"][q])
        assert 1 <= n <= budgets_a[q] and bool((a["tokens"][q, n:] == -1).all()) and bool((a["logprobs"][q, n:] == 0).all())
        for t in range(n):
            tok = int(a["tokens"][q, t])
            assert tok == int(a["ids"][q, p + t])
            worst = max(worst, abs(float(lp[q, p - 1 + t, tok]) - float(a["logprobs"][q, t])))
            total += 1
    print(f"{total} sampled tokens of 8 requests: largest difference of a log-probability to the dense forward {worst:.3e}, "
          f"tolerance {tiny.tol:.3e}; {a['steps']} token steps, {a['n_prefills']} prefills")
    assert worst <= tiny.tol
    assert torch.allclose(a["sum_logprob"], a["logprobs"].sum(1), rtol=0, atol=1e-6)


@pytest.mark.parametrize("pname,dtype", [CASES[0], CASES[3]])
def test_constrained_stream_is_the_plain_call_per_request(pname, dtype):
    m = model_of(pname, dtype)
    eng = m.ensure_engine()
    batch = eos_batch(pname)
    opts = options_of(batch, m.tokenizer)                          # each sample's own five options
    ref = generate.generate(eng, batch, temperature=0.0, constraints=opts)
    out = stream.generate_stream(eng, [batch] * 3, slots=4, admit=2, constraints=opts * 3)
    assert bool((ref["choice"] >= 0).all())
    for r in range(12):
        b = r % 4
        assert int(out["choice"][r]) == int(ref["choice"][b]), (r, b)
        assert_request_is_the_plain_rows(out, r, ref, b)
        n = int(out["n_generated"][r])
        assert out["tokens"][r, :n].tolist() == opts[b][int(out["choice"][r])] + [EOS]
    lengths = ref["n_generated"].tolist() * 3
    assert (out["steps"], out["n_prefills"], out["seated"]) == stream.simulate(lengths, 4, 2)


@pytest.mark.parametrize("pname,dtype", [CASES[0], CASES[3]])
def test_validation_through_one_stream(pname, dtype, tmp_path):
    """val_one_epoch with gen_stream = 4 over three copies of the fixture batch: the stats and the answers file of the
    --gen_stop_eos run."""
    m = model_of(pname, dtype)
    G = GEN_EOS[pname[:pname.rindex("_peaked")]]
    opt = types.SimpleNamespace(param_groups=[{"lr": 0.25}])
    stats, files = [], []
    m.args.gen_stop_eos = True
    try:
        for slots in (0, 4):
            d = tmp_path / f"stream{slots}"
            args = types.SimpleNamespace(is_generation_task=True, dataset="nextqa", debug=False, output_dir=str(d), gen_stream=slots)
            m.last_generation = None
            stats.append(engine.val_one_epoch(m, [golden_batch(G) for _ in range(3)], opt, epoch=1, args=args))
            files.append(json.load(open(d / "extracted_answers" / "extracted_answers_epoch1.json")))
            assert ("steps" in m.last_generation) == (slots > 0)
    finally:
        m.args.gen_stop_eos = False
    assert stats[0] == stats[1] and files[0] == files[1]
    assert (m.last_generation["steps"], m.last_generation["n_prefills"]) == (29, 6)


def test_the_public_surface():
    m = model_of("tiny_peakedperm", torch.float32)
    batch = eos_batch("tiny_peakedperm")
    want = m.generate(batch, stop_at_eos=True)
    ans = m.generate_stream([batch] * 3, slots=4, admit=2, return_logprobs=True)
    g = m.last_generation
    assert ans == want * 3 and (g["steps"], g["n_prefills"], g["occupancy"]) == (29, 6, 66 / 116)
    assert {"ids", "n_generated", "tokens", "seated", "logprobs", "sum_logprob"} <= set(g) and "choice" not in g
    assert m.generate_stream(batch, slots=1) == want and m.last_generation["n_prefills"] == 4          # admit defaults to 1
    # --gen_constrain options through the validation path: one trie over all requests, each batch's own options
    full = golden_batch(GEN_EOS["tiny"])
    m.args.gen_constrain = "options"
    try:
        want_best, want_ex = m(full, inference=True)
        want_choice = m.last_generation["choice"].clone()
        got = m.inference_stream([full, full], 3, 2)
    finally:
        del m.args.gen_constrain
    assert len(got) == 2 and m.last_generation["n_prefills"] == 4 and "occupancy" in m.last_generation
    for best, ex in got:
        assert torch.equal(best, want_best) and ex == want_ex
    assert torch.equal(m.last_generation["choice"], want_choice)
    with pytest.raises(ValueError, match="num_beams"):
        m.generate_stream(batch, slots=4, num_beams=2)
    with pytest.raises(ValueError, match="admit"):
        m.generate_stream(batch, slots=4, admit=5)


def test_answer_cli_over_a_file_of_questions(tmp_path):
    q = tmp_path / "questions.txt"
    q.write_text("what is the man doing\nwhy did the dog bark?\n\nwhere is the cat\nwho opens the door\nwhat happens next\n")
    r = subprocess.run([sys.executable, "answer.py", "--random_init", "--synthetic", "--questions", str(q), "--slots", "2",
                        "--max_new_tokens", "6", "--options", "a", "b", "c", "--constrain"],
                       cwd=os.path.join(ROOT, "flipped-vqa_amd"), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    head = next(i for i, ln in enumerate(lines) if ln.startswith("[5 questions, "))
    assert "prefills" in lines[head] and len(lines) == head + 6
    for ln in lines[head + 1:]:
        assert ln.split("\t")[-1] in ("[choice 0: a]", "[choice 1: b]", "[choice 2: c]"), ln
