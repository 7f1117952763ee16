"""min-p, n-gram blocking and a minimum length, without a GPU: the new C entry (fvqa_decode_next_rules) is exported by both builds
at ABI 18 and refuses bad operands before any launch, `generate` and the two parsers refuse the combinations that are not built
before anything touches the engine, and rules 0 and 3' of include/fvqa.h are restated here in fp64 numpy — `ban_set`,
`greedy_rules` and `kept_set_rules`, on top of tests/test_sampling_cpu.py::kept_set_ex; the yardsticks of
tests/test_pickrules_gpu.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from fvqa import _lib, generate, ops
from tests.test_sampling_cpu import kept_set_ex, penalised

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A = C.c_void_p(256)
BUILDS = [("bf16", _lib.BF16), ("f16", _lib.F16)]


# ------------------------------------------------------------------------------------------------ the rule in fp64
def ban_set(row_ids, gen_start, pos, V, n, m, eos):
    """Rule 0: the banned tokens of a row whose generated tokens are row_ids[max(gen_start, 0) .. pos] -> a set."""
    g0, X = max(int(gen_start), 0), set()
    if pos + 1 - int(gen_start) < m and 0 <= eos < V:
        X.add(int(eos))
    gen = [int(t) for t in row_ids[g0:pos + 1]] if pos + 1 > g0 else []
    if n >= 1 and len(gen) >= n - 1:
        s = gen[len(gen) - (n - 1):]                              # the last n - 1 generated tokens ([] for n = 1)
        for j in range(len(gen) - n + 1):                         # windows that lie inside the generated tokens
            if gen[j:j + n - 1] == s and 0 <= gen[j + n - 1] < V:
                X.add(gen[j + n - 1])
    return X


def greedy_rules(logits, R, r, X):
    """The greedy pick: the largest penalised logit among the tokens not banned, lowest index on ties; -1 when all are banned."""
    l1 = penalised(logits, R, r)
    idx = np.array([i for i in range(l1.size) if i not in X], dtype=np.int64)
    return int(idx[np.argmax(l1[idx])]) if idx.size else -1


def kept_set_rules(logits, R, r, T, top_k, top_p, X=(), min_p=0.0):
    """Rules 0 to 3' in fp64: the banned tokens leave the row (the maximum, Z and the number top-k is cut against are those of
    the others), kept_set_ex on what is left, and of that the tokens with p_i >= min_p * max p. -> (sorted kept token ids, p over
    the vocabulary with 0 at the banned tokens)."""
    l1 = penalised(logits, R, r)
    idx = np.array([i for i in range(l1.size) if i not in set(X)], dtype=np.int64)
    p = np.zeros(l1.size)
    if idx.size == 0:
        return idx, p
    kept, ps = kept_set_ex(l1[idx], [], 1.0, T, top_k, top_p)
    kept = kept[ps[kept] >= min_p * ps.max()]
    p[idx] = ps
    return idx[kept], p


def test_ban_set_on_hand_computed_rows():
    V, EOS = 50, 2
    row = [7, 8, 9, 7, 8, 9, 7, 8, 40, 41]                        # positions 0 .. 9
    # n = 1: every generated token, once; the prompt (in front of gen_start) is not scanned
    assert ban_set(row, 3, 7, V, 1, 0, EOS) == {7, 8, 9}
    assert ban_set(row, 6, 7, V, 1, 0, EOS) == {7, 8}
    # n = 2: what followed the last token (8 at position 7) inside the generated tokens: 9 at position 5 — not position 2
    assert ban_set(row, 3, 7, V, 2, 0, EOS) == {9}
    assert ban_set(row, 0, 7, V, 2, 0, EOS) == {9}
    # n = 3: what followed (7, 8): position 5 when the window 3..4 is generated; a window that straddles gen_start bans nothing
    assert ban_set(row, 3, 7, V, 3, 0, EOS) == {9}
    assert ban_set(row, 4, 7, V, 3, 0, EOS) == set()              # (7, 8) at 3..4 starts in the prompt
    assert ban_set(row, 0, 7, V, 3, 0, EOS) == {9}                # positions 0..1 and 3..4: the same token, once
    # fewer than n - 1 generated tokens: nothing (one generated token, n = 3); exactly n - 1: still no earlier window
    assert ban_set(row, 7, 7, V, 3, 0, EOS) == set()
    assert ban_set(row, 6, 7, V, 3, 0, EOS) == set()
    # nothing generated yet (pos = gen_start - 1), and gen_start below 0 reads from position 0
    assert ban_set(row, 8, 7, V, 1, 0, EOS) == set() == ban_set(row, 8, 7, V, 2, 0, EOS)
    assert ban_set(row, -3, 7, V, 2, 0, EOS) == {9}
    # a repeated n-gram with different continuations bans each of them
    assert ban_set([5, 6, 5, 7, 5, 6, 5], 0, 6, V, 2, 0, EOS) == {6, 7}
    # ids outside [0, V) are ignored as banned tokens, and compare as themselves inside a window
    assert ban_set([5, V + 3, 5, -4, 5], 0, 4, V, 2, 0, EOS) == set()
    assert ban_set([V + 3, 11, 9, V + 3], 0, 3, V, 2, 0, EOS) == {11}
    # the minimum length: the EOS while the token index p + 1 - gen_start is below m, free at i == m
    assert ban_set(row, 3, 4, V, 0, 3, EOS) == {EOS}              # i = 2
    assert ban_set(row, 3, 5, V, 0, 3, EOS) == set()              # i = 3
    assert ban_set(row, 3, 2, V, 0, 1, EOS) == {EOS}              # i = 0: the first pick
    assert ban_set(row, 3, 7, V, 2, 6, EOS) == {EOS, 9}           # both rules at once (i = 5 < 6)
    assert ban_set(row, 3, 4, V, 0, 3, V + 1) == set()            # an EOS outside the vocabulary bans nothing


def test_kept_set_rules_on_hand_computed_rows():
    lg = [2.0, 1.0, 0.0, -1.0]
    # neutral: kept_set_ex
    for top_k, top_p in ((0, 1.0), (2, 1.0), (0, 0.72), (2, 0.72)):
        assert np.array_equal(kept_set_rules(lg, [], 1.0, 1.0, top_k, top_p)[0], kept_set_ex(lg, [], 1.0, 1.0, top_k, top_p)[0])
    # a banned arg-max: the runner-up is the maximum, Z is the mass of the other three, top-k counts the tokens not banned
    kept, p = kept_set_rules(lg, [], 1.0, 1.0, 0, 1.0, X={0})
    assert kept.tolist() == [1, 2, 3] and p[0] == 0 and abs(p.sum() - 1) < 1e-12 and abs(p[1] - 1 / (1 + np.exp(-1) + np.exp(-2))) < 1e-12
    assert kept_set_rules(lg, [], 1.0, 1.0, 2, 1.0, X={0})[0].tolist() == [1, 2]
    assert kept_set_rules(lg, [], 1.0, 1.0, 3, 1.0, X={0})[0].tolist() == [1, 2, 3]      # k = the number not banned: the cut is off
    assert greedy_rules(lg, [], 1.0, {0}) == 1 and greedy_rules(lg, [], 1.0, {0, 1, 3}) == 2
    # the nucleus bound is taken of the mass without the banned token: 1 in front of rank 1 is 0.665 of 1.503
    assert kept_set_rules(lg, [], 1.0, 1.0, 0, 0.67, X={0})[0].tolist() == [1, 2]
    assert kept_set_rules(lg, [], 1.0, 1.0, 0, 0.66, X={0})[0].tolist() == [1]
    # the penalty's set R is unaffected by X: token 1 is penalised (1 / 4 = 0.25) although 0 is banned, and 1 stays in front of 2
    assert greedy_rules(lg, [1], 4.0, {0}) == 1 and greedy_rules(lg, [1], 4.0, set()) == 0
    assert greedy_rules([2.0, 1.0, 0.5, -1.0], [1], 4.0, {0}) == 2
    # every token banned: nothing is kept, nothing is picked
    assert kept_set_rules(lg, [], 1.0, 1.0, 0, 1.0, X={0, 1, 2, 3})[0].size == 0 and greedy_rules(lg, [], 1.0, {0, 1, 2, 3}) == -1
    # min-p: e = (1, 0.368, 0.135, 0.050)
    assert kept_set_rules(lg, [], 1.0, 1.0, 0, 1.0, min_p=0.04)[0].tolist() == [0, 1, 2, 3]
    assert kept_set_rules(lg, [], 1.0, 1.0, 0, 1.0, min_p=0.06)[0].tolist() == [0, 1, 2]
    assert kept_set_rules(lg, [], 1.0, 1.0, 0, 1.0, min_p=0.2)[0].tolist() == [0, 1]
    assert kept_set_rules(lg, [], 1.0, 1.0, 0, 1.0, min_p=0.999999)[0].tolist() == [0]
    # ... against the maximum that is NOT banned: with 0 banned e = (-, 1, 0.368, 0.135)
    assert kept_set_rules(lg, [], 1.0, 1.0, 0, 1.0, X={0}, min_p=0.2)[0].tolist() == [1, 2]
    # min_p -> 1 keeps the maximum and its exact ties, a whole tie group in or out
    tied = [1.0, 3.0, 3.0, 0.5, 3.0]
    assert kept_set_rules(tied, [], 1.0, 0.7, 0, 1.0, min_p=0.999999)[0].tolist() == [1, 2, 4]
    assert kept_set_rules([0.0, 3.0, 2.0, 2.0, 2.0], [], 1.0, 1.0, 0, 1.0, min_p=0.36)[0].tolist() == [1, 2, 3, 4]   # e = 0.368
    assert kept_set_rules([0.0, 3.0, 2.0, 2.0, 2.0], [], 1.0, 1.0, 0, 1.0, min_p=0.37)[0].tolist() == [1]
    # the shortest of the three prefixes: top-k 3, top-p 0.72 (two tokens), min-p — each the shortest once
    assert kept_set_rules(lg, [], 1.0, 1.0, 3, 1.0, min_p=0.04)[0].tolist() == [0, 1, 2]             # top-k
    assert kept_set_rules(lg, [], 1.0, 1.0, 3, 0.7, min_p=0.04)[0].tolist() == [0, 1]                # top-p: 1 <= 0.7 * 1.503
    assert kept_set_rules(lg, [], 1.0, 1.0, 3, 0.7, min_p=0.5)[0].tolist() == [0]                    # min-p
    # temperature enters e: at T = 2 e = (1, 0.607, 0.368, 0.223)
    assert kept_set_rules(lg, [], 1.0, 2.0, 0, 1.0, min_p=0.3)[0].tolist() == [0, 1, 2]


def test_min_p_is_the_sequential_warpers():
    """Hugging Face applies top-k, then top-p, then min-p, each on the renormalised survivors. The ratio of a probability to the
    largest does not change under renormalisation and every cut keeps the largest, so the result is the intersection."""
    rng = np.random.default_rng(3)
    for _ in range(50):
        V = int(rng.integers(5, 60))
        lg = 3.0 * rng.standard_normal(V)
        T, top_k, top_p, min_p = float(rng.uniform(0.5, 2)), int(rng.integers(0, V)), float(rng.uniform(0.3, 1)), float(rng.uniform(0, 0.6))
        x = lg / T
        alive = np.ones(V, dtype=bool)
        order = np.lexsort((np.arange(V), -x))
        if 1 <= top_k < V:
            alive[order[top_k:]] = False
        p = np.where(alive, np.exp(x - x.max()), 0.0)
        p /= p.sum()
        front = np.cumsum(p[order]) - p[order]
        alive[order[front > top_p]] = False
        p = np.where(alive, p, 0.0)
        p /= p.sum()
        alive &= p >= min_p * p.max()
        assert np.array_equal(np.flatnonzero(alive), kept_set_rules(lg, [], 1.0, T, top_k, top_p, min_p=min_p)[0])


# ------------------------------------------------------------------------------------------------ the C entry
def _args(dt, temperature=0.0, top_p=1.0, top_k=0, rep=1.0, u=A, stop=1, min_p=0.0, n=0, m=0):
    #      logits u emb T         top_p  top_k  r  eos stop ids pos done gen x tok kept lp act cnt pos64 B  V    D    S   dtype
    return [A, u, A, temperature, top_p, top_k, rep, 2, stop, A, A, A, A, A, A, A, A, A, A, A, 3, 509, 128, 16, dt, None, min_p, n, m]


@pytest.mark.parametrize("which,h16", BUILDS)
def test_decode_next_rules_is_exported_and_checks_its_operands_on_the_host(which, h16):
    """Every call here must be refused: one that passed validation would launch a kernel on fake addresses."""
    lib = _lib.load(which)
    assert lib.fvqa_version() == _lib.ABI_VERSION == 18          # an added entry changes no signature
    fn = lib.fvqa_decode_next_rules
    sig, sig_ex = _lib.SIGNATURES["fvqa_decode_next_rules"][1], _lib.SIGNATURES["fvqa_decode_next_ex"][1]
    assert len(_args(h16)) == len(sig) and sig[:len(sig_ex)] == sig_ex and sig[len(sig_ex):] == [C.c_float, C.c_int, C.c_int]
    assert callable(ops.decode_next_rules)                        # declared = bound = exported
    header = open(os.path.join(ROOT, "include", "fvqa.h")).read()
    assert "int fvqa_decode_next_rules(" in header and "int fvqa_sample_vote(" in header
    for dt in (h16, _lib.F32):
        base = _args(dt, temperature=0.7, top_p=0.9, top_k=8, rep=1.2, min_p=0.1, n=2, m=3)
        for at in (0, 1, 2, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18):   # every required pointer; u is required when sampling
            a = list(base)
            a[at] = None
            assert fn(*a) == -1, at
        for at in (20, 21, 22, 23):                               # B, V, D, S <= 0
            for bad in (0, -4):
                a = list(base)
                a[at] = bad
                assert fn(*a) == -2, (at, bad)
        a = list(base)
        a[20] = 65536                                             # the counter holds arrivals in 16 bits
        assert fn(*a) == -2
        for t in (-0.5, float("nan")):
            assert fn(*_args(dt, temperature=t, top_p=0.9, n=2)) == -1, t
        for p in (0.0, -0.1, 1.0001, float("nan")):
            assert fn(*_args(dt, temperature=0.7, top_p=p, n=2)) == -1, p
        for r in (0.999, 0.0, -2.0, float("nan")):
            assert fn(*_args(dt, temperature=0.7, top_p=0.9, rep=r, n=2)) == -1, r
        assert fn(*_args(dt, temperature=0.7, top_p=0.9, top_k=-1, n=2)) == -1
        for mp in (-0.01, 1.0, 1.5, float("nan"), float("inf")):  # min_p outside [0, 1)
            assert fn(*_args(dt, temperature=0.7, top_p=0.9, min_p=mp)) == -1, mp
            assert fn(*_args(dt, min_p=mp)) == -1, mp             # in greedy mode too
        for bad in (-1, -40):
            assert fn(*_args(dt, n=bad)) == -1 and fn(*_args(dt, m=bad)) == -1, bad
        assert fn(*_args(dt, m=1, stop=0)) == -1                  # a minimum length without the EOS stop
        # a bad parameter is reported in front of a bad shape, a bad shape in front of a bad alignment
        a = _args(dt, n=-1)
        a[21] = 0
        assert fn(*a) == -1
        a = list(base)
        a[21], a[0] = 0, C.c_void_p(258)
        assert fn(*a) == -2
        for at in (0, 12, 16, 18):                                # fp32 logits, gen_start, logprob, counter off their boundary
            a = list(base)
            a[at] = C.c_void_p(258)
            assert fn(*a) == -3, at
        for rep, v_bad in ((1.0, 1216513), (1.2, 626689)):        # no room in LDS for one bitmap / for the two
            a = _args(dt, rep=rep, n=2)
            a[21] = v_bad
            assert fn(*a) == -2, v_bad
    other = _lib.F16 if h16 == _lib.BF16 else _lib.BF16
    assert fn(*_args(other, n=2)) == -1                           # the other build's 16-bit code
    assert fn(*_args(7, n=2)) == -1


# ------------------------------------------------------------------------------------------------ generate and the parsers
def test_generate_refuses_what_it_cannot_serve():
    """All of these are refused before the engine is touched (there is none here)."""
    for kw in (dict(min_p=-0.1, temperature=0.8), dict(min_p=1.0, temperature=0.8), dict(min_p=float("nan"), temperature=0.8),
               dict(no_repeat_ngram_size=-1), dict(no_repeat_ngram_size=1.5), dict(min_new_tokens=-1), dict(min_new_tokens=2.5),
               dict(min_new_tokens=3, stop_at_eos=False), dict(min_new_tokens=9, max_new_tokens=8),
               dict(no_repeat_ngram_size=2, num_beams=2), dict(min_new_tokens=2, num_beams=2),
               dict(min_p=0.1, temperature=0.8, constraints=[[5, 6]]), dict(no_repeat_ngram_size=2, constraints=[[5, 6]]),
               dict(no_repeat_ngram_size=2, contrast="blind"), dict(min_new_tokens=2, contrast="blind"),
               dict(no_repeat_ngram_size=2, lookahead=4), dict(min_p=0.1, temperature=0.8, seed=0, lookahead=4),
               dict(no_repeat_ngram_size=2, lookahead=4, draft_tokens=np.zeros((1, 31), dtype=np.int32)),
               dict(min_new_tokens=2, lookahead=4, draft_answers=[[5, 6]]),
               dict(no_repeat_ngram_size=2, constraints=[[5, 6]], jump_forward=4),
               dict(vote=True), dict(vote=True, num_return_sequences=1, temperature=0.8),
               dict(vote=True, num_return_sequences=ops.VOTE_SAMPLES_MAX + 1, temperature=0.8),
               dict(vote=True, num_return_sequences=3, temperature=0.0),
               dict(vote=True, num_return_sequences=3, temperature=0.8, num_beams=2),
               dict(vote=True, num_return_sequences=3, temperature=0.8, seed=0, lookahead=4)):
        with pytest.raises(ValueError):
            generate.generate(None, {}, **kw)
    assert ops.VOTE_SAMPLES_MAX == 64


def test_the_stream_refuses_the_new_keywords():
    from fvqa import stream
    for kw in (dict(min_p=0.1), dict(no_repeat_ngram_size=2), dict(min_new_tokens=2), dict(vote=True)):
        with pytest.raises((TypeError, ValueError)):
            stream.generate_stream(None, [], slots=2, **kw)


def _refused(parser, argv):
    with pytest.raises(SystemExit):
        parser.parse_args(argv)


def test_the_parsers_accept_and_refuse_as_generate_does(capsys):
    sys.path.insert(0, os.path.join(ROOT, "flipped-vqa_amd"))
    import answer
    import train
    base = ["--random_init", "--synthetic", "--question", "why"]
    ap = answer.get_args_parser()
    a = ap.parse_args(base)
    assert a.min_p == 0.0 and a.no_repeat_ngram == 0 and a.min_new_tokens == 0 and a.vote is False
    a = ap.parse_args(base + ["--temperature", "1.5", "--min_p", "0.1", "--no_repeat_ngram", "3", "--min_new_tokens", "4",
                              "--num_samples", "5", "--vote", "--top_k", "8", "--repetition_penalty", "1.2", "--frame_attention"])
    assert a.min_p == 0.1 and a.no_repeat_ngram == 3 and a.min_new_tokens == 4 and a.vote is True and a.num_samples == 5
    a = ap.parse_args(base + ["--no_repeat_ngram", "2"])          # greedy with a ban set
    assert a.no_repeat_ngram == 2
    ap.parse_args(base + ["--temperature", "0.8", "--num_samples", "3", "--vote", "--options", "a", "b", "--constrain"])
    ap.parse_args(base + ["--temperature", "0.8", "--num_samples", "3", "--vote", "--contrast", "blind"])
    for bad in (["--min_p", "1.0", "--temperature", "0.8"], ["--min_p", "-0.1", "--temperature", "0.8"], ["--min_p", "0.1"],
                ["--no_repeat_ngram", "-1"], ["--min_new_tokens", "-2"], ["--min_new_tokens", "40", "--max_new_tokens", "8"],
                ["--no_repeat_ngram", "2", "--num_beams", "2"], ["--no_repeat_ngram", "2", "--options", "a", "b", "--constrain"],
                ["--min_new_tokens", "2", "--contrast", "blind"], ["--no_repeat_ngram", "2", "--lookahead", "4"],
                ["--no_repeat_ngram", "2", "--lookahead", "4", "--draft", "options", "--options", "a", "b"],
                ["--vote"], ["--vote", "--num_samples", "3"], ["--vote", "--num_samples", "1", "--temperature", "0.8"],
                ["--vote", "--num_samples", "65", "--temperature", "0.8"],
                ["--vote", "--num_samples", "3", "--temperature", "0.8", "--seed", "0", "--lookahead", "4"]):
        _refused(ap, base + bad)
    _refused(ap, ["--random_init", "--synthetic", "--questions", "q.txt", "--slots", "2", "--no_repeat_ngram", "2"])
    tp = train.get_args_parser()
    t = tp.parse_args([])
    assert t.gen_vote == 0 and t.gen_vote_temperature == 1.0 and t.gen_vote_top_p == 1.0
    assert t.gen_no_repeat_ngram == 0 and t.gen_min_new_tokens == 0
    assert not any(hasattr(t, k) for k in ("top_k", "repetition_penalty", "num_samples", "logprobs"))
    gen = ["--is_generation_task"]
    t = tp.parse_args(gen + ["--gen_vote", "5", "--gen_vote_temperature", "0.7", "--gen_vote_top_p", "0.9", "--gen_no_repeat_ngram",
                             "2", "--gen_min_new_tokens", "1"])
    assert t.gen_vote == 5 and t.gen_vote_temperature == 0.7 and t.gen_vote_top_p == 0.9 and t.gen_no_repeat_ngram == 2
    tp.parse_args(gen + ["--gen_vote", "3", "--gen_constrain", "options"])
    tp.parse_args(gen + ["--gen_vote", "3", "--contrast", "blind"])
    tp.parse_args(gen + ["--gen_stop_eos", "--gen_no_repeat_ngram", "2", "--gen_min_new_tokens", "2"])
    for bad in (["--gen_vote", "1"], ["--gen_vote", "65"], ["--gen_vote", "-3"], ["--gen_vote", "3", "--num_beams", "2"],
                ["--gen_vote", "3", "--lookahead", "4"], ["--gen_vote", "3", "--gen_constrain", "options", "--gen_jump_forward", "4"],
                ["--gen_vote", "3", "--gen_stream", "4"], ["--gen_vote", "3", "--val_vocab", "--answer_vocab", "v.txt"],
                ["--gen_vote", "3", "--gen_vote_temperature", "0"], ["--gen_vote", "3", "--gen_vote_top_p", "1.5"],
                ["--gen_no_repeat_ngram", "2"], ["--gen_stop_eos", "--gen_no_repeat_ngram", "-1"],
                ["--gen_stop_eos", "--gen_min_new_tokens", "2", "--gen_constrain", "options"],
                ["--gen_stop_eos", "--gen_no_repeat_ngram", "2", "--contrast", "blind"],
                ["--gen_stop_eos", "--gen_no_repeat_ngram", "2", "--gen_stream", "4"]):
        _refused(tp, gen + bad)
    _refused(tp, ["--gen_vote", "3"])                             # validation by vote is generation-task validation
    capsys.readouterr()
