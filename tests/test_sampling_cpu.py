"""Top-k, repetition penalty, log-probabilities and several samples per prompt, without a GPU: the new C entry
(fvqa_decode_next_ex) is exported by both builds at ABI 18 and refuses bad operands before any launch, `generate` refuses the
argument combinations it cannot serve before it touches the engine, and the rule of include/fvqa.h is restated here in fp64
numpy — `kept_set_ex`, which extends tests/test_generate_cpu.py::kept_set and is the yardstick of tests/test_sampling_gpu.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from fvqa import _lib, generate, ops
from tests.test_generate_cpu import kept_set

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
A = C.c_void_p(256)
BUILDS = [("bf16", _lib.BF16), ("f16", _lib.F16)]


# ------------------------------------------------------------------------------------------------ the rule in fp64
def penalised(logits, R, r):
    """Step 1: the ids of R inside [0, V), each once: l / r if l > 0 else l * r. -> fp64 copy."""
    l1 = np.asarray(logits, dtype=np.float64).copy()
    for i in {int(i) for i in R if 0 <= int(i) < l1.size}:
        l1[i] = l1[i] / r if l1[i] > 0 else l1[i] * r
    return l1


def ranked(logits, R, r, T):
    """-> (p = softmax(l1 / T), the order (p descending, index ascending), the mass in front of each rank), as kept_set."""
    x = penalised(logits, R, r) / T
    p = np.exp(x - x.max())
    p /= p.sum()
    order = np.lexsort((np.arange(p.size), -p))
    return p, order, np.cumsum(p[order]) - p[order]


def kept_set_ex(logits, R, r, T, top_k, top_p):
    """Steps 1-3 in fp64: the token at rank j is kept iff j < k and the mass in front of it is <= top_p * Z_k, Z_k the mass of
    the first k ranks (1 for k = V), k = top_k if 1 <= top_k < V else V. -> (sorted kept indices, p)."""
    p, order, front = ranked(logits, R, r, T)
    V = p.size
    k = top_k if 1 <= top_k < V else V
    z_k = 1.0 if k == V else float(p[order[:k]].sum())
    keep = (np.arange(V) < k) & (front <= top_p * z_k)
    return np.sort(order[keep]), p


def test_restatement_with_neutral_parameters_is_kept_set():
    rng = np.random.default_rng(11)
    for V, scale in ((64, 2.0), (509, 3.0), (4000, 6.0)):
        for T, top_p in ((0.8, 0.95), (1.0, 0.5), (0.3, 0.9), (1.5, 0.99), (1.0, 1.0)):
            lg = (scale * rng.standard_normal(V)).astype(np.float32)
            for top_k in (0, V, V + 7):
                got, p = kept_set_ex(lg, [3, 5, 5], 1.0, T, top_k, top_p)
                want, p0 = kept_set(lg, T, top_p)
                assert np.array_equal(got, want) and np.array_equal(p, p0), (V, T, top_p, top_k)


def test_restatement_on_hand_computed_rows():
    lg = [2.0, 1.0, 0.0, -1.0]
    assert kept_set_ex(lg, [], 1.0, 1.0, 2, 1.0)[0].tolist() == [0, 1]
    assert kept_set_ex(lg, [], 1.0, 1.0, 1, 1.0)[0].tolist() == [0]
    # e = (1, 1/e, ...): Z_2 = 1.3679; the mass in front of rank 1 is 1 = 0.731 * Z_2
    assert kept_set_ex(lg, [], 1.0, 1.0, 2, 0.74)[0].tolist() == [0, 1]
    assert kept_set_ex(lg, [], 1.0, 1.0, 2, 0.72)[0].tolist() == [0]
    # without the k the same bound is taken of the whole mass 1.5530: 1 = 0.644 of it
    assert kept_set_ex(lg, [], 1.0, 1.0, 0, 0.72)[0].tolist() == [0, 1]
    # ties across rank k: the lower indices
    assert kept_set_ex([1.0, 3.0, 1.0, 1.0, 0.5], [], 1.0, 0.7, 2, 1.0)[0].tolist() == [0, 1]
    assert kept_set_ex([1.0, 3.0, 1.0, 1.0, 0.5], [], 1.0, 0.7, 3, 1.0)[0].tolist() == [0, 1, 2]
    # the penalty: once per id however often it occurs, ids outside [0, V) ignored, negative logits multiplied
    assert penalised([4.0, 2.5, -1.0], [0, 0, 0, 7, -3], 1.5).tolist() == [4.0 / 1.5, 2.5, -1.0]
    assert penalised([-1.0, -1.4, 0.0], [0, 2, 0], 1.3).tolist() == [-1.3, -1.4, 0.0]
    assert kept_set_ex([4.0, 2.5, -1.0], [0, 0, 0], 1.5, 1.0, 1, 1.0)[0].tolist() == [0]       # 2.67 > 2.5
    assert kept_set_ex([4.0, 2.5, -1.0], [0, 0, 0], 1.7, 1.0, 1, 1.0)[0].tolist() == [1]       # 2.35 < 2.5
    assert kept_set_ex([-1.0, -1.4, -9.0], [0], 1.5, 1.0, 1, 1.0)[0].tolist() == [1]           # -1.5 < -1.4


# ------------------------------------------------------------------------------------------------ the C entry
def _args(dt, temperature=0.0, top_p=1.0, top_k=0, rep=1.0, u=A):
    #      logits u emb T         top_p  top_k  r  eos stop ids pos done gen x tok kept lp act cnt pos64 B  V    D    S   dtype
    return [A, u, A, temperature, top_p, top_k, rep, 2, 1, A, A, A, A, A, A, A, A, A, A, A, 3, 509, 128, 16, dt, None]


@pytest.mark.parametrize("which,h16", BUILDS)
def test_decode_next_ex_is_exported_and_checks_its_operands_on_the_host(which, h16):
    """Every call here must be refused: one that passed validation would launch a kernel on fake addresses."""
    lib = _lib.load(which)
    assert lib.fvqa_version() == _lib.ABI_VERSION == 18          # an added entry changes no signature
    fn = lib.fvqa_decode_next_ex
    assert len(_args(h16)) == len(_lib.SIGNATURES["fvqa_decode_next_ex"][1])
    assert callable(ops.decode_next_ex)                           # declared = bound = exported
    for dt in (h16, _lib.F32):
        base = _args(dt, temperature=0.7, top_p=0.9, top_k=8, rep=1.2)
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
            assert fn(*_args(dt, temperature=t, top_p=0.9)) == -1, t
        for p in (0.0, -0.1, 1.0001, float("nan")):
            assert fn(*_args(dt, temperature=0.7, top_p=p)) == -1, p
        for r in (0.999, 0.0, -2.0, float("nan")):
            assert fn(*_args(dt, temperature=0.7, top_p=0.9, rep=r)) == -1, r
            assert fn(*_args(dt, rep=r)) == -1, r                 # in greedy mode too
        for k in (-1, -40):
            assert fn(*_args(dt, temperature=0.7, top_p=0.9, top_k=k)) == -1, k
        for at in (0, 12, 16, 18):                                # fp32 logits, gen_start, logprob, counter off their boundary
            a = list(base)
            a[at] = C.c_void_p(258)
            assert fn(*a) == -3, at
        a = list(base)
        a[21] = 1216513                                           # no room in LDS for the bitmap of the penalised ids
        assert fn(*a) == -2
    other = _lib.F16 if h16 == _lib.BF16 else _lib.BF16
    assert fn(*_args(other)) == -1                                # the other build's 16-bit code
    assert fn(*_args(7)) == -1


# ------------------------------------------------------------------------------------------------ generate, answer.py
def test_generate_refuses_what_it_cannot_serve():
    """All of these are refused before the engine is touched (there is none here)."""
    for kw in (dict(num_return_sequences=3, temperature=0.0),
               dict(num_return_sequences=3, temperature=0.8, num_beams=2),
               dict(num_return_sequences=3, temperature=0.0, num_beams=2),
               dict(num_return_sequences=0, temperature=0.8),
               dict(top_k=-1, temperature=0.8),
               dict(top_k=1.5, temperature=0.8),
               dict(repetition_penalty=0.9),
               dict(repetition_penalty=float("nan")),
               dict(num_beams=2, return_logprobs=True),
               dict(num_beams=2, top_k=4)):
        with pytest.raises(ValueError):
            generate.generate(None, {}, **kw)


def test_answer_cli_has_the_sampling_flags():
    sys.path.insert(0, os.path.join(ROOT, "flipped-vqa_amd"))
    import answer
    import train
    a = answer.get_args_parser().parse_args(["--random_init", "--synthetic", "--question", "why"])
    assert a.top_k == 0 and a.repetition_penalty == 1.0 and a.num_samples == 1 and a.logprobs is False
    a = answer.get_args_parser().parse_args(["--random_init", "--synthetic", "--question", "why", "--temperature", "0.8", "--top_k",
                                             "8", "--repetition_penalty", "1.3", "--num_samples", "5", "--logprobs"])
    assert a.top_k == 8 and a.repetition_penalty == 1.3 and a.num_samples == 5 and a.logprobs is True
    t = train.get_args_parser().parse_args([])                   # validation stays greedy or beam: no new flag there
    assert not any(hasattr(t, k) for k in ("top_k", "repetition_penalty", "num_samples", "logprobs"))
