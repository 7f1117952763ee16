"""The vote over the samples of a prompt, without a GPU: the rule of include/fvqa.h fvqa_sample_vote restated in numpy (`vote_rule`,
the yardstick of tests/test_vote_gpu.py) on hand-computed cases, and the C entry — exported by both builds at ABI 18, refusing
bad operands before any launch."""
import ctypes as C

import numpy as np
import pytest

from fvqa import _lib, ops

A = C.c_void_p(256)


def vote_rule(tokens, score):
    """tokens (B, n, steps) int, score (B, n) float -> group, votes (B, n), winner, n_groups (B,) int32 and share (B,) fp32."""
    tokens, score = np.asarray(tokens), np.asarray(score, dtype=np.float32)
    B, n, _ = tokens.shape
    group, votes = np.zeros((B, n), dtype=np.int32), np.zeros((B, n), dtype=np.int32)
    winner, n_groups, share = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.float32)
    for b in range(B):
        for a in range(n):
            group[b, a] = next(j for j in range(a + 1) if np.array_equal(tokens[b, j], tokens[b, a]))
        for a in range(n):
            votes[b, a] = int((group[b] == a).sum()) if group[b, a] == a else 0
        reps = [a for a in range(n) if votes[b, a] > 0]
        s = np.where(np.isnan(score[b]), -np.inf, score[b])
        winner[b] = min(reps, key=lambda a: (-int(votes[b, a]), -float(s[a]), a))
        n_groups[b] = len(reps)
        share[b] = np.float32(votes[b, winner[b]]) / np.float32(n)
    return {"group": group, "votes": votes, "winner": winner, "n_groups": n_groups, "share": share}


def one(tokens, score):
    return {k: v[0].tolist() for k, v in vote_rule([tokens], [score]).items()}


def test_vote_rule_on_hand_computed_cases():
    a, b, c = [5, 6, -1], [5, 7, -1], [5, 6, 2]
    r = one([a, b, a, c, a], [-1.0, -0.5, -3.0, -0.1, -2.0])
    assert r["group"] == [0, 1, 0, 3, 0] and r["votes"] == [3, 1, 0, 1, 0] and r["winner"] == 0 and r["n_groups"] == 3
    assert r["share"] == pytest.approx(0.6)
    # all equal; all distinct (every group has one vote: the largest score wins); one sample
    assert one([a, a, a], [0.0, 0.0, 0.0]) == {"group": [0, 0, 0], "votes": [3, 0, 0], "winner": 0, "n_groups": 1, "share": 1.0}
    r = one([a, b, c], [-2.0, -1.0, -3.0])
    assert r["group"] == [0, 1, 2] and r["votes"] == [1, 1, 1] and r["winner"] == 1 and r["n_groups"] == 3
    assert one([a], [-1.0]) == {"group": [0], "votes": [1], "winner": 0, "n_groups": 1, "share": 1.0}
    # rows that differ only in their padding are two groups
    r = one([[5, 6, -1], [5, 6, 6], [5, 6, -1]], [0.0, 0.0, 0.0])
    assert r["group"] == [0, 1, 0] and r["votes"] == [2, 1, 0] and r["winner"] == 0
    # two groups tied on votes: the larger score of the REPRESENTATIVE decides (sample 3's -0.1 is not one)
    r = one([a, b, b, a], [-2.0, -1.0, -9.0, -0.1])
    assert r["votes"] == [2, 2, 0, 0] and r["winner"] == 1
    r = one([a, b, b, a], [-1.0, -2.0, -0.1, -9.0])
    assert r["winner"] == 0
    # tied on score too: the lower index
    assert one([a, b, b, a], [-1.0, -1.0, 0.0, 0.0])["winner"] == 0
    assert one([b, a, a, b], [-1.0, -1.0, 0.0, 0.0])["winner"] == 0
    # a NaN score counts as -inf: it loses a tie against any number, and ties with -inf go to the lower index
    assert one([a, b, b, a], [float("nan"), -50.0, 0.0, 0.0])["winner"] == 1
    assert one([a, b, b, a], [-50.0, float("nan"), 0.0, 0.0])["winner"] == 0
    assert one([a, b], [float("nan"), float("-inf")])["winner"] == 0
    assert one([a, b], [float("nan"), float("nan")])["winner"] == 0
    # more votes beat any score
    assert one([a, b, b], [0.0, float("nan"), 0.0])["winner"] == 1


def _args(B=3, n=5, steps=7):
    return [A] * 7 + [B, n, steps, None]


@pytest.mark.parametrize("which", ["bf16", "f16"])
def test_sample_vote_is_exported_and_checks_its_operands_on_the_host(which):
    """Every call here must be refused: one that passed validation would launch a kernel on fake addresses."""
    lib = _lib.load(which)
    assert lib.fvqa_version() == _lib.ABI_VERSION == 18
    fn = lib.fvqa_sample_vote
    assert len(_args()) == len(_lib.SIGNATURES["fvqa_sample_vote"][1]) and callable(ops.sample_vote)
    assert ops.VOTE_SAMPLES_MAX == 64
    for at in range(7):                                           # every pointer is required
        a = _args()
        a[at] = None
        assert fn(*a) == -1, at
    for kw in (dict(B=0), dict(B=-1), dict(B=65536), dict(n=0), dict(n=65), dict(n=-2), dict(steps=0), dict(steps=-3),
               dict(B=65535, n=64, steps=1024)):                  # (the last: more than 2^31 - 1 tokens)
        assert fn(*_args(**kw)) == -2, kw
    a = _args(n=0)
    a[0] = None
    assert fn(*a) == -1                                           # a null pointer is reported in front of a bad shape
    for at in range(7):                                           # every operand is 32-bit words
        a = _args()
        a[at] = C.c_void_p(258)
        assert fn(*a) == -3, at
    a = _args(steps=0)
    a[1] = C.c_void_p(258)
    assert fn(*a) == -2                                           # a bad shape in front of a bad alignment

