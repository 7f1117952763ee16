"""min-p, n-gram blocking and a minimum length on the GPU: fvqa_decode_next_rules alone — its neutral parameters against
fvqa_decode_next_ex bit for bit, rules 0 and 3' against their fp64 restatement (tests/test_pickrules_cpu.py) on five vocabularies,
among them the last whose row lives in LDS beside both bitmaps (36864) and the first whose row is recomputed (36865) — and
`generate` with the new keywords end to end."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from fvqa import generate, ops
from tests.test_beam_gpu import GAP, eos_batch, tiny  # noqa: F401  (tiny: the fixture and its tolerance)
from tests.test_generate_gpu import DEV, DTYPES, EPS, model_of, spread_u
from tests.test_pickrules_cpu import ban_set, greedy_rules, kept_set_rules
from tests.test_sampling_cpu import penalised
from tests.test_sampling_gpu import EOS, SAME, VOCABS, assert_same_bits, make_emb, step_ex

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# EPS (tests/test_generate_gpu.py:22) holds here unchanged: the ban set only takes elements out of the sums (they enter as 0.0f,
# as the elements outside top-k do) and min-p adds a pass that counts. The bound is EPS of the mass of what takes part.
VOCABS5 = VOCABS + [(36864, 6.0), (36865, 6.0)]      # ... | row + both bitmaps = 156672 bytes of LDS | the first row recomputed


def step_rules(logits, *, emb=None, u=None, ids=None, pos=None, done=None, gen_start=None, S=16, D=128, dtype=torch.float32,
               counter=None, **kw):
    """One launch of fvqa_decode_next_rules on host arrays -> dict of host arrays, as tests/test_sampling_gpu.py::step_ex."""
    lg_host = np.asarray(logits, dtype=np.float32)
    lg = torch.as_tensor(lg_host, device=DEV).clone()
    B, V = lg.shape
    if emb is None:
        emb = make_emb(V, D, dtype)
    t = lambda a, dt: torch.as_tensor(np.asarray(a), dtype=dt, device=DEV).contiguous()   # noqa: E731
    ids = t(np.zeros((B, S)) if ids is None else ids, torch.int64)
    pos = t(np.full(B, 3) if pos is None else pos, torch.int32)
    done = t(np.zeros(B) if done is None else done, torch.int32)
    gs = t(np.zeros(B) if gen_start is None else gen_start, torch.int32)
    x = torch.full((B, emb.shape[1]), float("nan"), dtype=emb.dtype, device=DEV)
    i32 = lambda n: torch.full((n,), -7, dtype=torch.int32, device=DEV)                  # noqa: E731
    tok, kept, act = i32(B), i32(B), i32(1)
    lp = torch.full((B,), float("nan"), dtype=torch.float32, device=DEV)
    pos64 = torch.full((B,), -7, dtype=torch.int64, device=DEV)
    if counter is None:
        counter = torch.zeros(1, dtype=torch.int32, device=DEV)
    ops.decode_next_rules(lg, emb, ids, pos, done, gs, x, tok, kept, lp, act, counter,
                          u=None if u is None else t(u, torch.float32), pos64=pos64, **kw)
    torch.cuda.synchronize()
    return {"token": tok.cpu().numpy(), "n_kept": kept.cpu().numpy(), "n_active": int(act), "ids": ids.cpu().numpy(),
            "pos": pos.cpu().numpy(), "done": done.cpu().numpy(), "x": x.cpu(), "emb": emb.cpu(), "pos64": pos64.cpu().numpy(),
            "logprob": lp.cpu().numpy(), "counter": int(counter), "logits_after": lg.cpu().numpy(), "logits": lg_host}


def check_rules_rows(r, lg, u, T, top_k, top_p, min_p=0.0, spans=None, rep=1.0, bans=None, max_left_out=0):
    """n_kept and the token of every row against rules 0 to 3' in fp64. The nucleus bound moves by EPS of the mass of the k; the
    min-p prefix is exact under its premise, asserted first: every token's |x_i - x_max - ln(min_p)| > GAP. A row whose gap at
    rank k is within GAP (fp32 could not tell which token has rank k) is left out, at most max_left_out of them."""
    B, V = lg.shape
    left_out = 0
    for b in range(B):
        R = [] if spans is None else spans[b]
        X = set() if bans is None else set(bans[b])
        idx = np.array([i for i in range(V) if i not in X], dtype=np.int64)          # what takes part
        x = penalised(lg[b], R, rep)[idx] / T
        p = np.exp(x - x.max())
        p /= p.sum()
        order = np.lexsort((np.arange(idx.size), -p))
        front = np.cumsum(p[order]) - p[order]
        k = top_k if 1 <= top_k < idx.size else idx.size
        n_mp = idx.size
        if min_p > 0:
            assert np.abs(x - x.max() - np.log(min_p)).min() > GAP, (b, np.abs(x - x.max() - np.log(min_p)).min())
            n_mp = int((x - x.max() >= np.log(min_p)).sum())
        if k < idx.size and np.sort(x)[::-1][k - 1] - np.sort(x)[::-1][k] <= GAP:
            left_out += 1
            continue
        z_k = float(p[order[:k]].sum())
        in_k = np.arange(idx.size) < k
        n = int(r["n_kept"][b])
        n_lo = min(n_mp, int((in_k & (front <= (top_p - EPS) * z_k)).sum()))
        n_hi = min(n_mp, int((in_k & (front <= (top_p + EPS) * z_k)).sum()))
        exact = kept_set_rules(lg[b], R, rep, T, top_k, top_p, X, min_p)[0].size
        print(f"V={V} T={T} top_p={top_p} k={top_k} min_p={min_p} r={rep} |X|={len(X)} row {b}: n_kept {n} in [{n_lo}, {n_hi}] "
              f"(fp64 {exact}, min-p prefix {n_mp})")
        assert n_lo <= exact <= n_hi and n_lo <= n <= n_hi, (b, n, n_lo, n_hi)
        if min_p > 0 and top_p == 1.0 and k == idx.size:
            assert n == n_mp, (b, n, n_mp)
        kept = np.sort(order[:n])                      # the n_kept highest elements, walked in index order
        tok = int(r["token"][b])
        assert tok not in X and 0 <= tok < V, (b, tok)
        j = int(np.searchsorted(idx, tok))
        assert j in kept, (b, tok)
        cdf = np.cumsum(p[kept])
        M = cdf[-1]
        at = int(np.searchsorted(kept, j))
        lo, hi = (cdf[at - 1] if at else 0.0) - EPS * M, cdf[at] + EPS * M
        assert lo <= float(u[b]) * M <= hi, (b, tok, lo, float(u[b]) * M, hi)
    assert left_out <= max_left_out, left_out


def decidable(lg, T, top_k, min_p, rep=1.0, spans=None, bans=None):
    """The premises of check_rules_rows on every row, in fp64: the gap at rank k and every token's distance to the min-p
    threshold exceed GAP. Tests that make their own rows take the first seed of seed, seed + 1000, .. whose rows are decidable."""
    for b in range(lg.shape[0]):
        X = set() if bans is None else set(bans[b])
        idx = np.array([i for i in range(lg.shape[1]) if i not in X], dtype=np.int64)
        x = np.sort(penalised(lg[b], [] if spans is None else spans[b], rep)[idx] / T)[::-1]
        if 1 <= top_k < idx.size and x[top_k - 1] - x[top_k] <= GAP:
            return False
        if min_p > 0 and np.abs(x - x[0] - np.log(min_p)).min() <= GAP:
            return False
    return True


def first_decidable(build, seed, *a):
    """build(seed) -> (lg, spans, bans, ...): the case of the first seed among seed, seed + 1000, .. that is decidable(lg, *a, ...)."""
    for j in range(10):
        case = build(seed + 1000 * j)
        if decidable(case[0], *a, spans=case[1], bans=case[2]):
            return case
    raise AssertionError("no decidable rows in ten seeds")


# ---- 1
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("V,scale", VOCABS5)
def test_neutral_parameters_are_decode_next_ex_bit_for_bit(V, scale, dtype):
    rng = np.random.default_rng(V)
    lg = (scale * rng.standard_normal((16, V))).astype(np.float32)
    u = rng.random(16).astype(np.float32)
    ids = rng.integers(0, V, (16, 16))
    for D in (128, 36):                               # (36 elements: 16-bit rows that are no multiple of 16 bytes)
        emb = make_emb(V, D, dtype)
        for T, top_p, top_k, rep in ((0.0, 1.0, 0, 1.0), (0.0, 1.0, 0, 1.3), (0.8, 0.95, 0, 1.0), (1.0, 0.5, 40, 1.0),
                                     (0.3, 0.9, 8, 1.3), (1.5, 0.99, 0, 1.2)):
            kw = dict(emb=emb, ids=ids, u=u if T > 0 else None, temperature=T, top_p=top_p, top_k=top_k, repetition_penalty=rep,
                      gen_start=np.full(16, 1), eos_id=EOS)
            old = step_ex(lg, **kw)
            new = step_rules(lg, min_p=0.0, no_repeat_ngram=0, min_new_tokens=0, **kw)
            assert_same_bits(old, new)                # token, n_kept, ids, pos, pos64, done, logprob; x_next and n_active
            assert new["counter"] == 0 and new["x"].dtype == dtype
            assert np.array_equal(new["logits_after"].view(np.uint32), lg.view(np.uint32))


# ---- 2
def minp_rows(V, scale, min_p, T):
    """The rows of the issue: default_rng(V + int(100 * min_p)); (509, T = 1.0, 0.02) needs the offset 3000 for its premise."""
    rng = np.random.default_rng((3000 if (V, T, min_p) == (509, 1.0, 0.02) else 0) + V + int(100 * min_p))
    return (scale * rng.standard_normal((16, V))).astype(np.float32), rng


@pytest.mark.parametrize("T", [0.7, 1.0])
@pytest.mark.parametrize("min_p", [0.02, 0.1, 0.5])
@pytest.mark.parametrize("V,scale", VOCABS5)
def test_min_p_follows_the_rule_in_fp64(V, scale, min_p, T):
    lg, rng = minp_rows(V, scale, min_p, T)
    u = rng.random(16).astype(np.float32)
    r = step_rules(lg, u=u, temperature=T, top_p=1.0, min_p=min_p)
    check_rules_rows(r, lg, u, T, 0, 1.0, min_p)       # (n_kept is exact here: the premise is asserted inside)
    assert np.array_equal(r["logits_after"].view(np.uint32), lg.view(np.uint32))
    r = step_rules(lg, u=u, temperature=T, top_p=0.9, top_k=8, min_p=min_p)
    check_rules_rows(r, lg, u, T, 8, 0.9, min_p, max_left_out=1)
    again = step_rules(lg, u=u, temperature=T, top_p=0.9, top_k=8, min_p=min_p)
    assert_same_bits(r, again)


@pytest.mark.parametrize("min_p,T", [(0.1, 0.7), (0.5, 1.0)])
@pytest.mark.parametrize("V,scale", VOCABS5)
def test_planted_tie_groups_are_wholly_in_or_out(V, scale, min_p, T):
    """Two groups of four exactly equal logits, 0.05 in l / T above and below the threshold ln(min_p) under the maximum: the upper
    group is kept whole, the lower one not at all; everything else lies 30 below."""
    rng = np.random.default_rng(V)
    row = (scale * rng.standard_normal(V)).astype(np.float32)
    v = np.float32(row.max() + 30.0)
    top, upper, lower = V // 3, [V - 1, 5, V // 2, 200], [V - 2, 7, V // 2 + 1, 300]
    row[top] = v
    row[upper] = np.float32(v + T * (np.log(min_p) + 0.05))
    row[lower] = np.float32(v + T * (np.log(min_p) - 0.05))
    r = step_rules(np.tile(row, (64, 1)), u=spread_u(64), temperature=T, top_p=1.0, min_p=min_p)
    assert np.array_equal(r["n_kept"], np.full(64, 5)), r["n_kept"]
    assert set(r["token"].tolist()) == set(upper) | {top}
    r = step_rules(np.tile(row, (64, 1)), u=spread_u(64), temperature=T, top_p=1.0, top_k=3, min_p=min_p)
    assert np.array_equal(r["n_kept"], np.full(64, 3)) and set(r["token"].tolist()) == {top, 5, 200}   # (the lower indices)
    r = step_rules(np.tile(row, (64, 1)), u=spread_u(64), temperature=T, top_p=1.0, min_p=0.999999)
    assert np.array_equal(r["n_kept"], np.ones(64)) and set(r["token"].tolist()) == {top}
    row[upper] = v                                    # min_p -> 1: the maximum and its exact ties
    r = step_rules(np.tile(row, (64, 1)), u=spread_u(64), temperature=T, top_p=1.0, min_p=0.999999)
    assert np.array_equal(r["n_kept"], np.full(64, 5)) and set(r["token"].tolist()) == set(upper) | {top}


# ---- 3
V_S, S_S = 509, 16
WINDOW_CASES = [                                      # (ids of a row from position 0, gen_start, pos)
    ([7, 8, 9, 7, 8, 9, 7, 8], 3, 7),                 # the hand-computed rows of tests/test_pickrules_cpu.py
    ([7, 8, 9, 7, 8, 9, 7, 8], 0, 7),
    ([7, 8, 9, 7, 8, 9, 7, 8], 4, 7),                 # n = 3: the window (7, 8) at 3 .. 4 straddles gen_start
    ([7, 8, 9, 7, 8, 9, 7, 8], 6, 7),                 # n - 1 = 2 generated tokens: no earlier window
    ([7, 8, 9, 7, 8, 9, 7, 8], 7, 7),                 # fewer than n - 1
    ([7, 8, 9, 7, 8, 9, 7, 8], 8, 7),                 # nothing generated
    ([7, 8, 9, 7, 8, 9, 7, 8], -3, 7),                # gen_start below 0
    ([5, 6, 5, 7, 5, 6, 5], 0, 6),                    # repeated occurrences with two continuations
    ([5, V_S + 3, 5, -4, 5], 0, 4),                   # continuations outside [0, V)
    ([V_S + 3, 11, 9, V_S + 3], 0, 3),                # an id outside [0, V) inside the window
    ([12, 12, 12, 12, 12, 12], 2, 5),                 # one token over and over
    ([20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31, 32, 33, 34], 1, 14),   # the longest row: pos = S - 2
]


@pytest.mark.parametrize("n", [1, 2, 3])
def test_ban_set_windows_and_occurrences(n):
    """Each row's logits put the tokens of its own id row in front, the later positions first, and in front of those what the
    restatement bans (tests/test_pickrules_cpu.py: hand-computed there): the greedy pick is the best token the ban set leaves,
    and a sampled row at top_p = 1 keeps exactly the tokens that are not banned."""
    B = len(WINDOW_CASES)
    ids = np.full((B, S_S), 400)
    lg = np.full((B, V_S), -5.0, dtype=np.float32)
    lg[:, 100] = 1.0                                  # what is left when every token of the row is banned
    gs, pos, bans = np.zeros(B), np.zeros(B), []
    for b, (row, g, p) in enumerate(WINDOW_CASES):
        ids[b, :len(row)] = row
        gs[b], pos[b] = g, p
        for j, t in enumerate(row):
            if 0 <= t < V_S:
                lg[b, t] = 10.0 + 0.25 * j
        bans.append(ban_set(ids[b], g, p, V_S, n, 0, EOS))
        lg[b, list(bans[b])] += 10.0
    print(f"n = {n}: ban sets {bans}")
    assert any(bans) and not all(bans)
    r = step_rules(lg, ids=ids, pos=pos, gen_start=gs, S=S_S, no_repeat_ngram=n)
    want = [greedy_rules(lg[b], [], 1.0, bans[b]) for b in range(B)]
    assert r["token"].tolist() == want and np.array_equal(r["n_kept"], np.ones(B))
    plain = step_ex(lg, ids=ids, pos=pos, gen_start=gs, S=S_S)
    assert [a != b for a, b in zip(plain["token"].tolist(), want)] == [bool(X) for X in bans]    # (the ban decides every such row)
    ref = torch.log_softmax(torch.from_numpy(lg).double(), -1).numpy()
    assert np.abs(r["logprob"] - ref[np.arange(B), r["token"]]).max() <= 1e-5        # the raw, whole row's
    u = spread_u(B)
    r = step_rules(lg, u=u, ids=ids, pos=pos, gen_start=gs, S=S_S, temperature=1.0, top_p=1.0, no_repeat_ngram=n)
    assert r["n_kept"].tolist() == [V_S - len(X) for X in bans]
    check_rules_rows(r, lg, u, 1.0, 0, 1.0, bans=bans)


def test_a_banned_arg_max_is_never_returned():
    V = 32000
    rng = np.random.default_rng(5)
    row = (6.0 * rng.standard_normal(V)).astype(np.float32)
    best, second = np.argsort(-row)[:2]
    ids = np.full((64, 16), int(best))
    r = step_rules(np.tile(row, (64, 1)), ids=ids, pos=np.full(64, 5), gen_start=np.full(64, 4), no_repeat_ngram=1)
    assert set(r["token"].tolist()) == {int(second)}
    u = spread_u(64)
    r = step_rules(np.tile(row, (64, 1)), u=u, ids=ids, pos=np.full(64, 5), gen_start=np.full(64, 4), temperature=1.0, top_p=0.95,
                   no_repeat_ngram=1)
    assert int(best) not in r["token"].tolist() and len(set(r["token"].tolist())) > 1
    check_rules_rows(r, np.tile(row, (64, 1)), u, 1.0, 0, 0.95, bans=[{int(best)}] * 64)


@pytest.mark.parametrize("V,scale", VOCABS5)
def test_a_dominant_banned_token_leaves_no_trace(V, scale):
    """The banned token holds 0.99 of the mass: n_kept and the draws are those of the row without it, so neither the maximum nor
    Z saw it (with it in Z the nucleus of 0.9 is that one token: asserted on the entry without the ban)."""
    def build(seed):
        rng = np.random.default_rng(seed)
        lg = (scale * rng.standard_normal((16, V))).astype(np.float32)
        heavy = rng.integers(0, V, 16)
        rest = np.log(np.exp(lg.astype(np.float64) - lg.max(1, keepdims=True)).sum(1)) + lg.max(1)
        lg[np.arange(16), heavy] = (rest + np.log(99.0)).astype(np.float32)
        return lg, None, [{int(t)} for t in heavy], heavy, rng.random(16).astype(np.float32)
    lg, _, bans, heavy, u = first_decidable(build, V + 1, 1.0, 40, 0.3)
    ids = np.tile(heavy[:, None], (1, 16))
    kw = dict(u=u, ids=ids, pos=np.full(16, 6), gen_start=np.full(16, 5), temperature=1.0, top_p=0.9)
    assert np.array_equal(step_ex(lg, **kw)["n_kept"], np.ones(16))                  # without the ban: the heavy token alone
    r = step_rules(lg, no_repeat_ngram=2, **kw)       # the bigram (heavy, heavy) occurred
    check_rules_rows(r, lg, u, 1.0, 0, 0.9, bans=bans)
    r = step_rules(lg, no_repeat_ngram=2, min_p=0.3, top_k=40, **kw)
    check_rules_rows(r, lg, u, 1.0, 40, 0.9, 0.3, bans=bans)


def test_top_k_is_cut_against_the_number_not_banned():
    lg = np.tile(np.array([[3.0, 2.5, 2.0, 1.5, 1.0, 0.5, 0.0, -0.5]], dtype=np.float32), (16, 1))
    ids = np.tile(np.array([[0, 2, 4, 6, 7] + [0] * 11]), (16, 1))                   # banned: 0, 2, 4, 6, 7 — left: 1, 3, 5
    kw = dict(u=spread_u(16), ids=ids, pos=np.full(16, 4), gen_start=np.zeros(16), temperature=1.0, top_p=1.0, no_repeat_ngram=1)
    for top_k, want in ((0, 3), (1, 1), (2, 2), (3, 3), (5, 3), (8, 3)):
        r = step_rules(lg, top_k=top_k, **kw)
        assert np.array_equal(r["n_kept"], np.full(16, want)), (top_k, r["n_kept"])
        assert set(r["token"].tolist()) == set([1, 3, 5][:want]), (top_k, r["token"])


def test_a_row_with_every_token_banned_ends():
    lg = np.tile(np.array([[2.0, 1.0, 0.0, -1.0]], dtype=np.float32), (3, 1))
    ids = np.tile(np.array([[3, 1, 0, 2, 1, 1, 1, 1]]), (3, 1))
    ids[1, 3] = 1                                     # row 1 has not generated token 2: it goes on
    pos, gs = np.array([3, 3, 3]), np.array([0, 0, 0])
    for kw in (dict(), dict(temperature=0.8, top_p=0.9, top_k=2, min_p=0.1, u=[0.3, 0.6, 0.9])):
        r = step_rules(lg, ids=ids, pos=pos, gen_start=gs, S=8, no_repeat_ngram=1, repetition_penalty=1.2, eos_id=0, **kw)
        assert r["token"].tolist() == [-1, 2, -1] and r["done"].tolist() == [1, 0, 1] and r["n_kept"].tolist() == [0, 1, 0]
        assert r["n_active"] == 1 and r["counter"] == 0
        want = ids.copy()
        want[1, 4] = 2
        assert np.array_equal(r["ids"], want) and r["pos"].tolist() == [3, 4, 3] == r["pos64"].tolist()
        assert r["logprob"][0] == 0.0 and r["logprob"][2] == 0.0 and r["logprob"][1] < 0
        emb = r["emb"]
        assert torch.equal(r["x"][0], emb[2]) and torch.equal(r["x"][1], emb[2]) and torch.equal(r["x"][2], emb[2])


# ---- 4
@pytest.mark.parametrize("V,scale", VOCABS5)
def test_minimum_length_bans_the_eos_until_the_mth_token(V, scale):
    """The EOS is the arg-max with 0.99 of the mass. Token index i = pos + 1 - gen_start: rows 0 .. 31 have i = m - 1, rows
    32 .. 63 have i = m."""
    m, g = 4, 6
    rng = np.random.default_rng(V + 2)
    row = (scale * rng.standard_normal(V)).astype(np.float32)
    row[EOS] = -50.0
    row[EOS] = np.float32(np.log(np.exp(row.astype(np.float64) - row.max()).sum()) + row.max() + np.log(99.0))
    lg = np.tile(row, (64, 1))
    pos = np.concatenate([np.full(32, g + m - 2), np.full(32, g + m - 1)])
    ids = rng.integers(3, V, (64, 16))
    kw = dict(ids=ids, pos=pos, gen_start=np.full(64, g), eos_id=EOS, min_new_tokens=m)
    r = step_rules(lg, **kw)
    runner_up = int(np.argsort(-row)[1])
    assert r["token"].tolist() == [runner_up] * 32 + [EOS] * 32 and r["done"].tolist() == [0] * 32 + [1] * 32
    assert r["n_active"] == 32
    u = np.concatenate([spread_u(32), spread_u(32)])
    r = step_rules(lg, u=u, temperature=1.0, top_p=0.9, **kw)
    assert EOS not in r["token"][:32].tolist() and not r["done"][:32].any() and (r["n_kept"][:32] > 1).all()
    assert r["token"][32:].tolist() == [EOS] * 32 and r["done"][32:].all() and np.array_equal(r["n_kept"][32:], np.ones(32))
    check_rules_rows({k: v[:32] for k, v in r.items() if k in ("token", "n_kept")}, lg[:32], u[:32], 1.0, 0, 0.9, bans=[{EOS}] * 32)
    ref = torch.log_softmax(torch.from_numpy(row).double(), -1).numpy()
    assert np.abs(r["logprob"][32:] - ref[EOS]).max() <= 1e-5 and np.abs(r["logprob"][:32] - ref[r["token"][:32]]).max() <= 1e-4
    with pytest.raises(ValueError):
        step_rules(lg, stop_at_eos=False, **kw)


# ---- 5
@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("V,scale", VOCABS5)
def test_everything_at_once(V, scale, n):
    """Penalty + ban + min-p + top-k: spans of 9 ids with repeats, among them each row's five most likely tokens (the penalty
    reorders the head, the ban takes some of it out), an id past the vocabulary and a negative one; the EOS banned as well."""
    S, T, top_p, rep, top_k, min_p, m = 16, 0.8, 0.9, 1.3, 40, 0.05, 12

    def build(seed):
        rng = np.random.default_rng(seed)
        lg = (scale * rng.standard_normal((16, V))).astype(np.float32)
        u = rng.random(16).astype(np.float32)
        ids = rng.integers(0, V, (16, S))
        head = np.argsort(-lg, axis=1)[:, :5]
        ids[:, 5:10] = head
        ids[:, 10] = head[:, 0]
        ids[:, 11] = V + 3
        ids[:, 12] = -1
        ids[:, 13] = head[:, 0]                       # n = 2: what followed head[0] before — head[1] and V + 3 — is banned
        ids[:, 4] = head[:, 1]                        # (in front of gen_start: no part of R or X)
        lg[:, EOS] = lg.max(1) + 1.0                  # the EOS in front, and banned: i = 9 < m
        spans = [ids[b, 5:14].tolist() for b in range(16)]
        bans = [ban_set(ids[b], 5, 13, V, n, m, EOS) for b in range(16)]
        return lg, spans, bans, u, ids
    lg, spans, bans, u, ids = first_decidable(build, 9000 + V + n, T, top_k, min_p, rep)
    gs, pos = np.full(16, 5), np.full(16, 13)
    assert all(EOS in X and len(X) >= 2 for X in bans) and any(set(spans[b]) - bans[b] for b in range(16))
    kw = dict(u=u, ids=ids, pos=pos, gen_start=gs, S=S, temperature=T, top_p=top_p, top_k=top_k, repetition_penalty=rep, min_p=min_p,
              no_repeat_ngram=n, min_new_tokens=m, eos_id=EOS)
    r = step_rules(lg, **kw)
    check_rules_rows(r, lg, u, T, top_k, top_p, min_p, spans=spans, rep=rep, bans=bans)
    assert np.array_equal(r["logits_after"].view(np.uint32), lg.view(np.uint32))
    assert_same_bits(r, step_rules(lg, **kw))         # two launches, the same bits
    # the penalty's bitmap is unaffected by X: with nothing banned the entry is fvqa_decode_next_ex under the same penalty
    free = dict(kw, no_repeat_ngram=0, min_new_tokens=0, min_p=0.0)
    assert_same_bits(step_rules(lg, **free), step_ex(lg, **{k: v for k, v in free.items()
                                                             if k not in ("no_repeat_ngram", "min_new_tokens", "min_p")}))
    g = step_rules(lg, **dict(kw, temperature=0.0, u=None))
    assert g["token"].tolist() == [greedy_rules(lg[b], spans[b], rep, bans[b]) for b in range(16)]


@pytest.mark.parametrize("B", [5, 20])
def test_counter_and_determinism(B):
    V, S = 32000, 16
    rng = np.random.default_rng(B)
    lg = (6.0 * rng.standard_normal((B, V))).astype(np.float32)
    lg[:, EOS] = -50.0
    lg[1, EOS] = 99.0                                 # row 1 takes the EOS (i = 5 >= m), row 2 has no room, row 3 is done
    u = rng.random(B).astype(np.float32)
    ids = rng.integers(3, V, (B, S))
    pos, done = np.full(B, 6), np.zeros(B)
    pos[2], done[3] = S - 1, 1
    kw = dict(u=u, ids=ids, pos=pos, done=done, gen_start=np.full(B, 2), S=S, temperature=0.9, top_p=0.9, top_k=40,
              repetition_penalty=1.2, eos_id=EOS, min_p=0.05, no_repeat_ngram=1, min_new_tokens=3)
    counter = torch.zeros(1, dtype=torch.int32, device=DEV)
    a = step_rules(lg, counter=counter, **kw)
    assert a["n_active"] == B - 3 == int((a["done"] == 0).sum()) and a["counter"] == 0 and a["token"][1] == EOS
    b = step_rules(lg, counter=counter, **kw)         # back to back on the same word, fresh copies of the inputs
    assert b["n_active"] == B - 3 and b["counter"] == 0
    assert_same_bits(a, b)
    for row in range(B):
        if row not in (2, 3):
            assert a["token"][row] not in ids[row, 2:7].tolist()                     # n = 1: no generated token again


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("D", [128, 36])
def test_sixteen_bit_rows_are_gathered(dtype, D):
    V = 509
    rng = np.random.default_rng(D)
    lg = (3.0 * rng.standard_normal((16, V))).astype(np.float32)
    ids = rng.integers(0, V, (16, 16))
    r = step_rules(lg, u=spread_u(16), ids=ids, pos=np.full(16, 7), gen_start=np.full(16, 2), temperature=0.9, top_p=0.9, min_p=0.05,
                   no_repeat_ngram=1, D=D, dtype=dtype)
    assert r["x"].dtype == dtype
    assert torch.equal(r["x"].view(torch.uint8), r["emb"][torch.from_numpy(r["token"]).long()].view(torch.uint8))
    for b in range(16):
        assert r["token"][b] not in ids[b, 2:8].tolist()


# ------------------------------------------------------------------------------------------------ end to end
def spied_rules(eng, batch, **kw):
    """generate(**kw) with every launch of ops.decode_next_rules recorded: (logits, ids, pos, gen_start) as the launch found them."""
    seen = []
    real = ops.decode_next_rules

    def spy(lg, emb, ids, pos, done, gen_start, *a, **k):
        seen.append((lg.cpu().numpy().copy(), ids.cpu().numpy().copy(), pos.cpu().numpy().copy(), gen_start.cpu().numpy().copy()))
        return real(lg, emb, ids, pos, done, gen_start, *a, **k)

    ops.decode_next_rules = spy
    try:
        out = generate.generate(eng, batch, **kw)
    finally:
        ops.decode_next_rules = real
    return out, seen


def follows_the_rule(out, seen, prefix, V, n, m, eos):
    """Every token of a greedy run is the first arg-max of its row's logits without the ban set, restated on the very logits and
    id rows each launch was given — where the two best are apart. -> the number of undecided steps."""
    tokens = out["tokens"].cpu().numpy()
    undecided = 0
    for t, (lg, ids, pos, gs) in enumerate(seen[:out["steps"]]):
        for b, p in enumerate(prefix):
            tok = int(tokens[b, t])
            if tok < 0:
                continue                              # the row had stopped
            assert gs[b] == p and pos[b] == p - 1 + t
            X = ban_set(ids[b], gs[b], pos[b], V, n, m, eos)
            assert tok not in X, (t, b, tok)
            l1 = lg[b].astype(np.float64)
            l1[list(X)] = -np.inf
            best = np.sort(l1)[::-1]
            if best[0] - best[1] > GAP:
                assert tok == int(l1.argmax()), (t, b)
            else:
                undecided += 1
    return undecided


def test_no_repeat_ngram_end_to_end_follows_the_rule():
    """On tiny_peaked, whose greedy answer is one token over and over (the answers of tiny_peakedperm, the fixture of the other end
    to end tests, are chains of distinct tokens: they hold no bigram twice and would show nothing here)."""
    eng = model_of("tiny_peaked", torch.float32).ensure_engine()
    batch = eos_batch("tiny_peakedperm")
    prefix = batch["prefix_index"]["vqa"]
    kw = dict(temperature=0.0, stop_at_eos=False, max_new_tokens=12)
    plain = generate.generate(eng, batch, **kw)["tokens"].cpu().numpy()
    for row in plain:                                 # the premise: every plain answer repeats a bigram
        grams = list(zip(row[:-1].tolist(), row[1:].tolist()))
        assert len(set(grams)) < len(grams), row
    out, seen = spied_rules(eng, batch, no_repeat_ngram_size=2, **kw)
    tokens = out["tokens"].cpu().numpy()
    assert len(seen) == out["steps"] == 12 and tuple(tokens.shape) == (4, 12)
    for row in tokens:
        grams = list(zip(row[:-1].tolist(), row[1:].tolist()))
        assert len(set(grams)) == len(grams), row
    assert not np.array_equal(tokens, plain) and np.array_equal(tokens[:, :2], plain[:, :2])     # (the first bigram is free)
    undecided = follows_the_rule(out, seen, prefix, eng.V, 2, 0, eng.model.tokenizer.eos_id)
    print(f"{4 * 12} token steps, {undecided} with the two best allowed logits within {GAP}")
    assert 4 * undecided <= 4 * 12
    for b, p in enumerate(prefix):
        assert out["ids"][b, p:p + 12].tolist() == tokens[b].tolist()


def test_min_new_tokens_end_to_end_follows_the_rule(tiny):  # noqa: F811
    eng, batch, m = tiny.eng, tiny.batch, 5
    eos = eng.model.tokenizer.eos_id
    plain = generate.generate(eng, batch, temperature=0.0, stop_at_eos=True, max_new_tokens=12)
    assert int(plain["n_generated"].min()) < m        # the premise: a plain answer ends before m (sample 0: at its first token)
    out, seen = spied_rules(eng, batch, temperature=0.0, stop_at_eos=True, max_new_tokens=12, min_new_tokens=m)
    assert int(out["n_generated"].min()) >= m
    tokens = out["tokens"].cpu().numpy()
    assert not (tokens[:, :m] == eos).any()
    for b in range(len(tiny.prefix)):
        if int(plain["n_generated"][b]) > m:          # a row that was long enough anyway is untouched
            assert torch.equal(out["ids"][b], plain["ids"][b])
    undecided = follows_the_rule(out, seen, tiny.prefix, eng.V, 0, m, eos)
    assert 4 * undecided <= tokens.size
    with pytest.raises(ValueError):
        generate.generate(eng, batch, temperature=0.0, stop_at_eos=True, max_new_tokens=4, min_new_tokens=5)


def test_sampled_rules_end_to_end(tiny):  # noqa: F811
    """min_p, the ban set and several samples per prompt together: seeded runs repeat, no sample repeats a token (n = 1), and
    every picked token's probability is at least min_p times the largest of its row (checked on the launches' own logits)."""
    eng, batch = tiny.eng, tiny.batch
    kw = dict(temperature=3.0, min_p=0.05, no_repeat_ngram_size=1, num_return_sequences=3, max_new_tokens=8, seed=11,
              stop_at_eos=False, return_logprobs=True)
    out, seen = spied_rules(eng, batch, **kw)
    again = generate.generate(eng, batch, **kw)
    for k in ("ids", "tokens", "logprobs"):
        assert torch.equal(out[k], again[k]), k
    tokens = out["tokens"].cpu().numpy().reshape(-1, out["steps"])
    for row in tokens:
        assert len(set(row.tolist())) == row.size, row
    for t, (lg, ids, pos, gs) in enumerate(seen):
        for b in range(tokens.shape[0]):
            X = ban_set(ids[b], gs[b], pos[b], eng.V, 1, 0, 2)
            x = lg[b].astype(np.float64) / 3.0
            x[list(X)] = -np.inf
            assert x[tokens[b, t]] - x.max() >= np.log(0.05) - GAP, (t, b)


# ---- 9
def test_the_defaults_launch_what_they_launched(tiny):  # noqa: F811
    """The four keywords at their defaults: the same sequence of ops calls, operand for operand, and the same result bits as the
    call without them (tools/generate_trace.py's recorder)."""
    spec = importlib.util.spec_from_file_location("generate_trace", os.path.join(ROOT, "tools", "generate_trace.py"))
    gt = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gt)
    eng, batch = tiny.eng, tiny.batch
    off = dict(min_p=0.0, no_repeat_ngram_size=0, min_new_tokens=0, vote=False)
    for kw in (dict(), dict(temperature=0.8, top_p=0.9, seed=0), dict(top_k=5, repetition_penalty=1.2, return_logprobs=True),
               dict(temperature=0.8, seed=0, num_return_sequences=3), dict(num_beams=3), dict(contrast="blind")):
        generate.generate(eng, batch, **kw)           # (a first call may build what later calls find: the fan-out cache)
        lines = []
        for extra in ({}, off):
            gt.forget_plans(eng)
            tr = gt.Trace()
            out = tr.run(lambda: generate.generate(eng, batch, **kw, **extra))
            lines.append((tr.calls, tr.sha.hexdigest(), gt.result_hash(out)))
        print(kw, lines[0])
        assert lines[0] == lines[1] and lines[0][0] > 0, kw
    seen = []
    real = ops.decode_next_rules
    ops.decode_next_rules = lambda *a, **k: seen.append(1) or real(*a, **k)
    try:
        generate.generate(eng, batch, top_k=5, temperature=0.8, seed=0, **off)
        assert not seen
        generate.generate(eng, batch, top_k=5, temperature=0.8, seed=0, min_p=0.1, max_new_tokens=3)
        assert len(seen) == 3                         # still one launch per token
    finally:
        ops.decode_next_rules = real
