"""Draft-and-verify greedy decoding, without a GPU: the rule of include/fvqa.h (fvqa_spec_step) restated in numpy — `lookup_draft`,
`given_draft` and `spec_step_ref`, the yardstick of tests/test_lookahead_gpu.py — and checked on hand-made id rows; the two C entries
exported by both builds at ABI 18 and refusing bad operands before any launch; `generate`'s keywords, what they refuse, and the
flags."""
import ctypes as C
import os
import sys
import types

import numpy as np
import pytest
import torch

from fvqa import _lib, generate, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A = C.c_void_p(256)
BUILDS = [("bf16", _lib.BF16), ("f16", _lib.F16)]
EOS = 2


# ------------------------------------------------------------------------------------------------ the rule
def lookup_draft(ids, P, G, room, V):
    """Prompt lookup over the committed ids[0 .. P]: for g = G down to 1 the largest e with g - 1 <= e < P and
    ids[e-g+1 .. e] == ids[P-g+1 .. P]; the first g with a match wins; the draft is ids[e+1 .. e+min(room, P-e)], ended in front
    of the first id outside [0, V). -> the draft, a list (empty: no match, no room)."""
    ids = [int(t) for t in ids]
    if room < 1:
        return []
    for g in range(G, 0, -1):
        if P - g + 1 < 0:
            continue
        tail = ids[P - g + 1:P + 1]
        hits = [e for e in range(g - 1, P) if ids[e - g + 1:e + 1] == tail]
        if hits:
            e = max(hits)
            out = []
            for t in ids[e + 1:e + 1 + min(room, P - e)]:
                if not 0 <= t < V:
                    break
                out.append(t)
            return out
    return []


def given_draft(drafts, n_generated, room, V):
    """The caller's drafts (max_new_tokens,) read at the row's n_generated: up to `room` entries, ended in front of the first one
    outside [0, V) (a -1 ends a draft) and by the end of the array."""
    out = []
    for t in [int(x) for x in drafts[n_generated:n_generated + max(room, 0)]]:
        if not 0 <= t < V:
            break
        out.append(t)
    return out


def first_argmax(row):
    """The first index of the largest value (np.argmax's rule, fvqa_decode_next's)."""
    return int(np.argmax(np.asarray(row)))


def spec_step_ref(logits, w, m, ids, pos, done, n_generated, *, T, eos_id=EOS, stop_at_eos=True, max_new_tokens, drafts=None, G=2):
    """One row of fvqa_spec_step in fp64. logits (T, V); w (T,) the pass's tokens (w[0] unused); ids (S,), copied.
    -> dict(ids, pos, done, n_generated, tokens, logprobs, n_committed, n_drafted, w_next (the next pass's tokens), start)."""
    lg = np.asarray(logits, dtype=np.float64)
    V, S = lg.shape[1], len(ids)
    ids = np.array(ids, dtype=np.int64)
    m = min(max(int(m), 1), T)
    live = done == 0 and pos >= -1 and pos + 1 < S and n_generated < max_new_tokens
    toks, lps = [], []
    if not live:
        at = min(max(pos, 0), S - 1)
        return dict(ids=ids, pos=pos, done=1, n_generated=n_generated, tokens=toks, logprobs=lps, n_committed=0, n_drafted=0,
                    w_next=[], w0=int(min(max(ids[at], 0), V - 1)), start=at, live=False)
    for i in range(m):
        g = first_argmax(lg[i])
        mx = lg[i].max()
        toks.append(g)
        lps.append(float(lg[i, g] - (mx + np.log(np.exp(lg[i] - mx).sum()))))
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
                n_drafted=m - 1, w_next=w_next, w0=toks[-1], start=pos, live=True)


def test_lookup_falls_back_from_G_to_one():
    #       0  1  2  3  4  5  6  7  8
    row = [5, 6, 7, 8, 9, 6, 7, 3, 7]                       # P = 8: "3 7" never occurred, "7" did (at 6 and at 2)
    assert lookup_draft(row, 8, 2, 3, 100) == [3, 7]        # g = 2 has no match; g = 1: e = 6 -> ids[7], ids[8]
    assert lookup_draft(row, 8, 1, 3, 100) == [3, 7]
    assert lookup_draft(row, 6, 2, 3, 100) == [8, 9, 6]     # P = 6: "6 7" occurred at e = 2
    assert lookup_draft(row, 6, 4, 3, 100) == [8, 9, 6]     # g = 4 and 3 have no match
    assert lookup_draft(row, 4, 4, 3, 100) == []            # "9" never occurred before: a plain step
    assert lookup_draft(row, 0, 4, 3, 100) == []            # nothing in front of position 0
    assert lookup_draft([4, 4], 1, 4, 3, 100) == [4]        # g = 2 needs P >= 2: g = 1 matches at e = 0


def test_the_most_recent_match_wins_and_the_longer_ngram_first():
    row = [1, 2, 30, 1, 2, 40, 9, 2, 50, 1, 2]              # P = 10: "1 2" at e = 1 and e = 4; "2" alone also at e = 7
    assert lookup_draft(row, 10, 2, 2, 100) == [40, 9]      # the later "1 2", not the first one
    assert lookup_draft(row, 10, 1, 2, 100) == [50, 1]      # G = 1: the most recent "2"
    assert lookup_draft(row, 10, 3, 2, 100) == [40, 9]      # "50 1 2" never occurred: falls to g = 2, not to the nearer g = 1


def test_the_draft_is_cut_at_P_minus_e_at_the_room_and_at_an_id_outside_the_vocabulary():
    row = [7, 8, 7]                                          # P = 2, e = 0: only ids[1], ids[2] lie behind the match
    assert lookup_draft(row, 2, 1, 5, 100) == [8, 7]        # min(room, P - e) = 2
    assert lookup_draft(row, 2, 1, 1, 100) == [8]           # the room
    assert lookup_draft(row, 2, 1, 0, 100) == []
    row = [7, 8, 200, 9, 7]
    assert lookup_draft(row, 4, 1, 4, 100) == [8]           # 200 >= V ends the draft
    assert lookup_draft(row, 4, 1, 4, 201) == [8, 200, 9, 7]
    row = [7, -3, 9, 7]
    assert lookup_draft(row, 3, 1, 4, 100) == []            # a negative id right behind the match
    assert given_draft([5, 6, -1, 8], 0, 3, 100) == [5, 6] and given_draft([5, 6, 100, 8], 1, 3, 100) == [6]
    assert given_draft([5, 6, 7, 8], 2, 5, 100) == [7, 8] and given_draft([5, 6, 7, 8], 4, 5, 100) == []


def test_a_row_of_the_rule_by_hand():
    V, S, T = 12, 10, 4
    lg = np.full((T, V), -1.0)
    for i, t in enumerate([5, 6, 7, 8]):
        lg[i, t] = 2.0
    ids = [3, 4, 5, 9, 0, 0, 0, 0, 0, 0]
    base = dict(T=T, max_new_tokens=20, drafts=np.array([5, 6, 7, 8, 9] + [-1] * 15))
    r = spec_step_ref(lg, [-1, 5, 6, 1], 4, ids, 3, 0, 1, **base)                  # drafts 5, 6 accepted, 1 is not row 2's 7
    assert r["tokens"] == [5, 6, 7] and r["pos"] == 6 and r["n_generated"] == 4 and r["n_drafted"] == 3
    assert r["ids"].tolist() == [3, 4, 5, 9, 5, 6, 7, 0, 0, 0] and r["w_next"] == [7, 9] and r["done"] == 0   # drafts[4:]: 9, -1
    r = spec_step_ref(lg, [-1, 9, 6, 7], 4, ids, 3, 0, 1, **base)                  # the first draft is wrong: a plain step
    assert r["tokens"] == [5] and r["w_next"] == [5, 7, 8, 9] and r["n_drafted"] == 3          # drafts[2:5]
    r = spec_step_ref(lg, [-1, 5, 6, 7], 4, ids, 3, 0, 1, **{**base, "max_new_tokens": 3})     # the budget cuts the commit
    assert r["tokens"] == [5, 6] and r["done"] == 1 and r["w_next"] == []
    r = spec_step_ref(lg, [-1, 5, 6, 7], 4, ids, 3, 0, 1, eos_id=6, **base)        # an EOS among the accepted drafts
    assert r["tokens"] == [5, 6] and r["done"] == 1
    r = spec_step_ref(lg, [-1, 5, 6, 7], 4, ids, S - 3, 0, 1, **base)              # the row fills: done at its NEXT step
    assert r["tokens"] == [5, 6] and r["pos"] == S - 1 and r["done"] == 0 and r["w_next"] == []
    r = spec_step_ref(lg, [-1, 5], 2, r["ids"], r["pos"], 0, 3, **base)
    assert not r["live"] and r["done"] == 1 and r["tokens"] == [] and r["w0"] == 6 and r["start"] == S - 1
    tie = lg.copy()
    tie[0, 2] = 2.0                                                                 # an exact tie: the lower index
    assert spec_step_ref(tie, [-1, 5, 6, 7], 4, ids, 3, 0, 1, **base)["tokens"] == [2]
    r = spec_step_ref(lg, [-1, 5, 6, 7], 4, ids, 3, 0, 1, T=T, max_new_tokens=20, G=2)   # prompt lookup: "9 5"? no; "5" at e = 2
    assert r["tokens"] == [5, 6, 7, 8] and r["w_next"] == [8]                      # 8 never occurred before


# ------------------------------------------------------------------------------------------------ the C entries
def _step_args(dt, n_seq=3, T=4, G=2, drafts=True, max_new=8):
    #       logits emb drafts           G  eos stop max_new ids pos done ngen w len start x tok lp nc nd act cnt pos64
    return [A, A, A if drafts else None, G, 2, 1, max_new, A, A, A, A, A, A, A, A, A, A, A, A, A, A, A,
            n_seq, T, 509, 128, 16, dt, None]                        # B T V D S dtype stream


def _append_args(dt, T=4, S=32, Dh=128):
    #       suf cache o g1 g2 vstart start len cos sin  n_seq T  S  H  Dh  A   F  rot dtype stream
    return [A, A, A, A, A, A, A, A, A, A, 3, T, S, 2, Dh, 10, 10, 1, dt, None]


@pytest.mark.parametrize("which,h16", BUILDS)
def test_the_entries_are_exported_and_check_their_operands_on_the_host(which, h16):
    """Every call here must be refused: one that passed validation would launch a kernel on fake addresses."""
    lib = _lib.load(which)
    assert lib.fvqa_version() == _lib.ABI_VERSION == 18          # added entries change no signature
    fn = lib.fvqa_spec_step
    assert len(_step_args(h16)) == len(_lib.SIGNATURES["fvqa_spec_step"][1])
    assert len(_append_args(h16)) == len(_lib.SIGNATURES["fvqa_attn_suffix_append"][1])
    assert callable(ops.spec_step) and callable(ops.attn_suffix_append)
    for dt in (h16, _lib.F32):
        base = _step_args(dt)
        for at in (0, 1, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20):       # every required pointer
            a = list(base)
            a[at] = None
            assert fn(*a) == -1, at
        for G in (0, 5, -1):
            assert fn(*_step_args(dt, G=G, drafts=False)) == -1, G                   # the lookup's n-gram; ignored under drafts
        for n_seq, T, want in ((0, 4, -2), (3, 0, -2), (3, 17, -2), (65536, 1, -2), (16384, 4, -2), (4096, 16, -2)):
            assert fn(*_step_args(dt, n_seq=n_seq, T=T)) == want, (n_seq, T)
        assert fn(*_step_args(dt, max_new=0)) == -2
        for at in (24, 25, 26):                                      # V, D, S <= 0
            a = list(base)
            a[at] = 0
            assert fn(*a) == -2, at
        for at in (0, 2, 8, 11, 16, 20):                             # logits, drafts, pos, w, logprob, counter off 4 bytes
            a = list(base)
            a[at] = C.c_void_p(258)
            assert fn(*a) == -3, at
        for at in (7, 21):                                           # ids, pos64 off 8 bytes
            a = list(base)
            a[at] = C.c_void_p(260)
            assert fn(*a) == -3, at
        ap = lib.fvqa_attn_suffix_append
        for at in range(10):
            a = list(_append_args(dt))
            a[at] = None
            assert ap(*a) == -1, at
        assert ap(*_append_args(dt, T=17)) == -2 and ap(*_append_args(dt, T=0)) == -2
        assert ap(*_append_args(dt, S=4097)) == -2 and ap(*_append_args(dt, Dh=64)) == -2
        a = list(_append_args(dt))
        a[1] = C.c_void_p(264)                                       # the cache off its 16-byte boundary
        assert ap(*a) == -3
    other = _lib.F16 if h16 == _lib.BF16 else _lib.BF16
    assert fn(*_step_args(other)) == -1 and fn(*_step_args(7)) == -1             # the other build's 16-bit code; no code at all
    assert lib.fvqa_attn_suffix_append(*_append_args(other)) == -1


# ------------------------------------------------------------------------------------------------ generate
def _data(B=2, S=16):
    return {"text_id": {"vqa": torch.zeros(B, 1, S, dtype=torch.int64)}, "prefix_index": {"vqa": [min(10, S - 1)] * B},
            "video": torch.ones(B, 10, 768)}


def test_generate_refuses_what_lookahead_cannot_serve():
    """All refused before the engine is touched (there is none here)."""
    eng = types.SimpleNamespace(model=None, pack=None, device="cpu", V=509)
    for kw in (dict(lookahead=4, temperature=0.7), dict(lookahead=4, num_beams=2), dict(lookahead=2, top_k=5),
               dict(lookahead=4, repetition_penalty=1.2), dict(lookahead=4, temperature=0.7, num_return_sequences=2),
               dict(lookahead=4, num_return_sequences=2), dict(lookahead=4, constraints=[[5, 6]]), dict(lookahead=4, contrast="blind"),
               dict(lookahead=17), dict(lookahead=-1), dict(lookahead=2.5), dict(lookahead=4, lookup_ngram=0),
               dict(lookahead=4, lookup_ngram=5), dict(lookahead=4, lookup_ngram=1.5),
               dict(lookahead=0, draft_tokens=torch.zeros(2, 31, dtype=torch.int32)),
               dict(lookahead=1, draft_tokens=torch.zeros(2, 31, dtype=torch.int32))):
        with pytest.raises(ValueError):
            generate.generate(eng, _data(), **kw)
    for bad in (torch.zeros(2, 30, dtype=torch.int32), torch.zeros(3, 31, dtype=torch.int32), torch.zeros(31, dtype=torch.int32),
                torch.zeros(2, 31)):
        with pytest.raises(ValueError, match="draft_tokens"):
            generate.generate(eng, _data(), lookahead=4, draft_tokens=bad)
    with pytest.raises(ValueError, match="draft_tokens"):
        generate.generate(eng, _data(), lookahead=4, max_new_tokens=5, draft_tokens=torch.zeros(2, 31, dtype=torch.int32))
    with pytest.raises(ValueError, match="65535"):
        generate.generate(eng, _data(B=4096, S=4), lookahead=16)
    with pytest.raises(ValueError, match="prefix_index"):
        generate.generate(eng, {}, lookahead=4)
    # what can be served passes these checks and goes on to the prefill's first read of the batch
    for kw in (dict(lookahead=2), dict(lookahead=16, lookup_ngram=4), dict(lookahead=4, return_logprobs=True, stop_at_eos=False),
               dict(lookahead=4, draft_tokens=torch.zeros(2, 31, dtype=torch.int64), lookup_ngram=99),
               dict(lookahead=4, max_new_tokens=3, draft_tokens=[[1, 2, 3], [4, 5, -1]])):
        with pytest.raises(KeyError, match="label"):
            generate.generate(eng, _data(), **kw)


def test_without_the_keyword_nothing_changes(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("a call without lookahead went to the draft-and-verify path")
    monkeypatch.setattr(generate, "_generate_lookahead", boom)
    monkeypatch.setattr(ops, "spec_step", boom)
    monkeypatch.setattr(ops, "attn_suffix_append", boom)
    eng = types.SimpleNamespace(model=None, pack=None, device="cpu")
    for kw in ({}, {"lookahead": 0}, {"lookahead": 1}, {"lookahead": 1, "lookup_ngram": 77}, {"temperature": 0.7, "lookahead": 0}):
        with pytest.raises(ValueError, match="prefix_index"):        # the first thing the existing path asks for
            generate.generate(eng, {}, **kw)
    seen = {}
    monkeypatch.setattr(generate, "beam_search", lambda *a, **k: seen.update(k))
    generate.generate(eng, {}, num_beams=2)
    assert seen and not any(k.startswith("look") or k.startswith("draft") for k in seen)      # beam search is called as it was


# ------------------------------------------------------------------------------------------------ the flags
def test_the_parsers_accept_the_flags_and_refuse_what_is_not_built():
    import train
    a = train.get_args_parser().parse_args([])
    assert a.lookahead == 0 and a.lookup_ngram == 2
    a = train.get_args_parser().parse_args(["--lookahead", "4", "--lookup_ngram", "3", "--is_generation_task"])
    assert a.lookahead == 4 and a.lookup_ngram == 3
    assert train.get_args_parser().parse_args(["--lookahead", "1", "--num_beams", "3"]).num_beams == 3      # 1: off
    for bad in (["--lookahead", "4", "--num_beams", "2"], ["--lookahead", "17"], ["--lookahead", "-2"],
                ["--lookahead", "4", "--lookup_ngram", "5"], ["--lookahead", "4", "--lookup_ngram", "0"],
                ["--lookahead", "4", "--contrast", "blind"], ["--lookahead", "4", "--gen_constrain", "options"]):
        with pytest.raises(SystemExit):
            train.get_args_parser().parse_args(bad)
    sys.path.insert(0, os.path.join(ROOT, "flipped-vqa_amd"))
    import answer
    base = ["--random_init", "--synthetic", "--question", "why"]
    assert answer.get_args_parser().parse_args(base).lookahead == 0
    a = answer.get_args_parser().parse_args(base + ["--lookahead", "8", "--lookup_ngram", "1"])
    assert a.lookahead == 8 and a.lookup_ngram == 1
    with pytest.raises(SystemExit):
        answer.get_args_parser().parse_args(base + ["--lookahead", "4", "--num_beams", "4"])


def test_the_model_passes_the_keywords_through(monkeypatch):
    from llama.model import Transformer
    seen = {}
    ids = torch.tensor([[7, 8, 9, EOS, 0, 0]])

    def fake(eng, data, **kw):
        seen.clear()
        seen.update(kw)
        out = {"ids": ids, "n_generated": torch.tensor([3]), "steps": 2, "tokens": ids[:, 1:4].int()}
        if kw.get("lookahead", 0) > 1:
            out.update(n_committed=torch.tensor([[1, 2]]), n_drafted=torch.tensor([[0, 3]]))
        return out
    monkeypatch.setattr(generate, "generate", fake)
    tok = types.SimpleNamespace(eos_id=EOS, sp_model=None)
    me = types.SimpleNamespace(ensure_engine=lambda: None, tokenizer=tok)
    data = {"prefix_index": {"vqa": [1]}}
    drafts = torch.tensor([[8, 9, EOS]])
    assert Transformer.generate.__wrapped__(me, data, max_new_tokens=3, lookahead=4, lookup_ngram=3, draft_tokens=drafts) == [[8, 9]]
    assert seen == {"max_new_tokens": 3, "lookahead": 4, "lookup_ngram": 3, "draft_tokens": drafts}
    assert set(me.last_generation) == {"ids", "n_generated", "steps", "n_committed", "n_drafted"}
    Transformer.generate.__wrapped__(me, data, max_new_tokens=3)
    assert seen == {"max_new_tokens": 3} and set(me.last_generation) == {"ids", "n_generated", "steps"}      # as it was
    # the validation path: --lookahead T [--lookup_ngram G]
    monkeypatch.setattr(generate, "match_answers", lambda model, d, i: ("best", "sims", "extracted"))
    me.args = types.SimpleNamespace(lookahead=4, lookup_ngram=3)
    assert Transformer.inference.__wrapped__(me, data) == ("best", "extracted")
    assert seen["lookahead"] == 4 and seen["lookup_ngram"] == 3 and seen["stop_at_eos"] is True and seen["temperature"] == 0.0
    assert set(me.last_generation) == {"ids", "similarities", "n_committed", "n_drafted"}
    me.args = types.SimpleNamespace(lookahead=4, contrast="blind")
    with pytest.raises(ValueError, match="lookahead"):
        Transformer.inference.__wrapped__(me, data)
    me.args = types.SimpleNamespace(lookahead=1, gen_stop_eos=True)                  # 1: off — the call --gen_stop_eos made before
    Transformer.inference.__wrapped__(me, data)
    assert "lookahead" not in seen and set(me.last_generation) == {"ids", "similarities"}
