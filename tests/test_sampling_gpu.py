"""Top-k, repetition penalty, log-probabilities and several samples per prompt on the GPU: the token-step kernel alone
(fvqa_decode_next_ex, csrc/sample.hip) against the old entry bit for bit at neutral parameters and against the fp64 restatement
of tests/test_sampling_cpu.py everywhere else, then `generate` end to end on the tiny fixture of tests/test_beam_gpu.py — against
beam search's score, against teacher-forced dense forwards of what it returns, and against the restatement on spied logits."""
import numpy as np
import pytest
import torch

from fvqa import generate, ops
from tests.test_beam_gpu import GAP, dense_logits, eos_batch, tiny  # noqa: F401  (tiny: the fixture and its tolerance)
from tests.test_generate_gpu import DEV, DTYPES, EPS, model_of, spread_u
from tests.test_generate_gpu import step as step_old
from tests.test_sampling_cpu import kept_set_ex, penalised, ranked

pytestmark = pytest.mark.gpu
# EPS (tests/test_generate_gpu.py:22) holds here unchanged: the passes the new entry adds either count (integers) or sum a
# thread's strided elements exactly as the nucleus bisection does — still at most 125 fp32 adds in sequence per thread at
# V = 32000 (157 at V = 40003: 9.4e-6 in place of 7.5e-6, five times that plus 1e-5 for __expf stays under 1e-4) —, and Z_k adds
# ONE product to such a sum. Under top-k every masked sum and the walk only ever add kept tokens (the others enter as 0.0f), so
# the bound is EPS of the mass of the k, which is what the checks below use.
VOCABS = [(509, 3.0), (32000, 6.0), (40003, 6.0)]    # ragged strided tails | the row in LDS | 4 * V > 144 KiB: recomputed
EOS = 2


# ------------------------------------------------------------------------------------------------ the kernel alone
def make_emb(V, D, dtype):
    return torch.randn(V, D, generator=torch.Generator().manual_seed(1)).to(dtype).to(DEV)


def step_ex(logits, *, emb=None, u=None, ids=None, pos=None, done=None, gen_start=None, S=16, D=128, dtype=torch.float32,
            counter=None, **kw):
    """One launch of the new entry on host arrays -> dict of host arrays (the in/out operands after the step included, the
    logits buffer as the launch left it, and the counter)."""
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
    ops.decode_next_ex(lg, emb, ids, pos, done, gs, x, tok, kept, lp, act, counter,
                       u=None if u is None else t(u, torch.float32), pos64=pos64, **kw)
    torch.cuda.synchronize()
    return {"token": tok.cpu().numpy(), "n_kept": kept.cpu().numpy(), "n_active": int(act), "ids": ids.cpu().numpy(),
            "pos": pos.cpu().numpy(), "done": done.cpu().numpy(), "x": x.cpu(), "emb": emb.cpu(), "pos64": pos64.cpu().numpy(),
            "logprob": lp.cpu().numpy(), "counter": int(counter), "logits_after": lg.cpu().numpy(), "logits": lg_host}


SAME = ("token", "n_kept", "ids", "pos", "pos64", "done")


def assert_same_bits(a, b, keys=SAME + ("logprob",)):
    for k in keys:
        assert np.array_equal(a[k].view(np.uint32) if a[k].dtype == np.float32 else a[k],
                              b[k].view(np.uint32) if b[k].dtype == np.float32 else b[k]), k
    assert torch.equal(a["x"].view(torch.uint8), b["x"].view(torch.uint8)) and a["n_active"] == b["n_active"]


BOOK = dict(V=509, S=16, tokens=[40, EOS, 77, 88, EOS], pos=[3, 4, 15, 6, -1], done=[0, 0, 0, 1, 0])


def book_case():
    """The case of tests/test_generate_gpu.py::test_row_bookkeeping: row 2 is full, row 3 is done, row 4 starts at -1."""
    lg = np.full((5, BOOK["V"]), -1.0, dtype=np.float32)
    for b, t in enumerate(BOOK["tokens"]):
        lg[b, t] = 3.0
    ids0 = np.arange(5 * BOOK["S"]).reshape(5, BOOK["S"]) % 400 + 3
    return lg, ids0


# ---- 1
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("V,scale", VOCABS)
def test_neutral_parameters_are_the_old_kernel_bit_for_bit(V, scale, dtype):
    rng = np.random.default_rng(V)
    lg = (scale * rng.standard_normal((16, V))).astype(np.float32)
    u = rng.random(16).astype(np.float32)
    ids = rng.integers(0, V, (16, 16))
    for D in (128, 36):                               # (36 elements: 16-bit rows that are no multiple of 16 bytes)
        emb = make_emb(V, D, dtype)
        for T, top_p in ((0.0, 1.0), (0.8, 0.95), (1.0, 0.5), (0.3, 0.9), (1.5, 0.99)):
            kw = dict(emb=emb, ids=ids, u=u if T > 0 else None, temperature=T, top_p=top_p, eos_id=EOS)
            old = step_old(lg, **kw)
            new = step_ex(lg, gen_start=np.full(16, 1), top_k=0, repetition_penalty=1.0, **kw)   # (a span of three ids, r = 1)
            assert_same_bits(old, new, SAME)
            assert new["counter"] == 0 and new["x"].dtype == dtype
            assert torch.equal(new["x"].view(torch.uint8), new["emb"][torch.from_numpy(new["token"]).long()].view(torch.uint8))
            assert np.array_equal(new["logits_after"].view(np.uint32), lg.view(np.uint32))


def test_row_bookkeeping_through_the_new_entry():
    lg, ids0 = book_case()
    S = BOOK["S"]
    kw = dict(ids=ids0, pos=BOOK["pos"], done=BOOK["done"], S=S, eos_id=EOS)
    for stop, done_want, act_want in ((True, [0, 1, 1, 1, 1], 1), (False, [0, 0, 1, 1, 0], 3)):
        r = step_ex(lg, gen_start=[2, 2, 2, 2, 0], stop_at_eos=stop, **kw)
        want = ids0.copy()
        want[0, 4], want[1, 5], want[4, 0] = 40, EOS, EOS
        assert np.array_equal(r["ids"], want)                                   # rows 2 (full) and 3 (done) untouched
        assert r["pos"].tolist() == [4, 5, S - 1, 6, 0] == r["pos64"].tolist()
        assert r["done"].tolist() == done_want and r["n_active"] == act_want and r["counter"] == 0
        assert r["token"].tolist() == [40, EOS, -1, -1, EOS] and r["n_kept"].tolist() == [1, 1, 0, 0, 1]
        assert r["logprob"][2] == 0.0 and r["logprob"][3] == 0.0 and (r["logprob"][[0, 1, 4]] < 0).all()
        emb = r["emb"]
        assert torch.equal(r["x"][0], emb[40]) and torch.equal(r["x"][1], emb[EOS])
        assert torch.equal(r["x"][2], emb[int(ids0[2, S - 1])]) and torch.equal(r["x"][3], emb[int(ids0[3, 6])])
        assert_same_bits(step_old(lg, stop_at_eos=stop, **kw), r, SAME)
    r = step_ex(lg[:2], ids=ids0[:2], pos=[S - 1, S - 1], done=[0, 1], S=S, temperature=0.7, top_k=4, u=[0.3, 0.6])
    assert r["n_active"] == 0 and np.array_equal(r["ids"], ids0[:2]) and r["logprob"].tolist() == [0.0, 0.0]


# ---- 2
def check_rows(r, lg, u, T, top_k, top_p, spans=None, rep=1.0):
    """n_kept and the token of every row against the rule in fp64, the nucleus bound moved by EPS of the mass of the k.
    Asserts the premise first: the gap of l1 / T at rank k exceeds GAP (else fp32 could not tell which token has rank k)."""
    B, V = lg.shape
    k = top_k if 1 <= top_k < V else V
    for b in range(B):
        R = [] if spans is None else spans[b]
        p, order, front = ranked(lg[b], R, rep, T)
        if k < V:
            x = np.sort(penalised(lg[b], R, rep) / T)[::-1]
            assert x[k - 1] - x[k] > GAP, (b, k, x[k - 1] - x[k])
        z_k = float(p[order[:k]].sum())
        in_k = np.arange(V) < k
        n = int(r["n_kept"][b])
        n_lo = int((in_k & (front <= (top_p - EPS) * z_k)).sum())
        n_hi = int((in_k & (front <= (top_p + EPS) * z_k)).sum())
        exact = kept_set_ex(lg[b], R, rep, T, top_k, top_p)[0].size
        print(f"V={V} T={T} top_p={top_p} k={top_k} r={rep} row {b}: n_kept {n} in [{n_lo}, {n_hi}] (fp64 {exact})")
        assert n_lo <= exact <= n_hi and n_lo <= n <= n_hi, (b, n, n_lo, n_hi)
        if top_p == 1.0 and k < V:
            assert n == k, (b, n)
        kept = np.sort(order[:n])                      # the n_kept highest tokens, walked in index order
        tok = int(r["token"][b])
        assert tok in kept, (b, tok)
        cdf = np.cumsum(p[kept])
        M = cdf[-1]
        j = int(np.searchsorted(kept, tok))
        lo, hi = (cdf[j - 1] if j else 0.0) - EPS * M, cdf[j] + EPS * M
        assert lo <= float(u[b]) * M <= hi, (b, tok, lo, float(u[b]) * M, hi)


def topk_rows(V, scale, k):
    """16 rows whose gap of l / T at rank k exceeds GAP for both temperatures below (asserted in check_rows): default_rng(V + k)
    gives such rows for every pair but two."""
    rng = np.random.default_rng((1000 if (V, k) in ((40003, 2), (40003, 40)) else 0) + V + k)
    return (scale * rng.standard_normal((16, V))).astype(np.float32), rng


@pytest.mark.parametrize("T,top_p", [(0.7, 1.0), (1.0, 0.9)])
@pytest.mark.parametrize("k", [1, 2, 8, 40])
@pytest.mark.parametrize("V,scale", VOCABS)
def test_top_k_follows_the_rule_in_fp64(V, scale, k, T, top_p):
    lg, rng = topk_rows(V, scale, k)
    u = rng.random(16).astype(np.float32)
    r = step_ex(lg, u=u, temperature=T, top_p=top_p, top_k=k)
    check_rows(r, lg, u, T, k, top_p)


@pytest.mark.parametrize("V,scale", VOCABS)
def test_top_k_edges(V, scale):
    lg, _ = topk_rows(V, scale, 1)
    u = spread_u(16)                                  # 0 and 1 - 2^-24 among them
    for T in (0.7, 1.0):
        r = step_ex(lg, u=u, temperature=T, top_p=0.9, top_k=1)
        assert np.array_equal(r["token"], lg.argmax(1)) and np.array_equal(r["n_kept"], np.ones(16))
    off = step_ex(lg, u=u, temperature=0.8, top_p=0.95, top_k=0)
    for k in (V, V + 5, 2 ** 31 - 1):
        assert_same_bits(off, step_ex(lg, u=u, temperature=0.8, top_p=0.95, top_k=k))
    g = step_ex(lg, temperature=0.0, top_k=3, top_p=0.2)                       # greedy ignores both cuts
    assert np.array_equal(g["token"], lg.argmax(1)) and np.array_equal(g["n_kept"], np.ones(16))


# ---- 3
@pytest.mark.parametrize("top_p", [1.0, 0.999])
@pytest.mark.parametrize("V,scale", VOCABS)
def test_planted_ties_at_the_cut(V, scale, top_p):
    """k = 6: four tokens above a group of four exactly equal logits that straddles rank k — ranks 4 .. 7. The two lower indices
    of the group are inside the k. (top_p = 0.999 goes through the nucleus bisection as well and must come out at the same cut:
    the mass in front of rank 5 is at most 0.92 of Z_k.)"""
    rng = np.random.default_rng(V)
    row = (scale * rng.standard_normal(V)).astype(np.float32)
    v = np.float32(row.max() + 2.0)
    above = [V - 1, 17, V // 2, 3]
    group = [V - 2, 5, V - 7, 200]                    # in index order: 5, 200, V - 7, V - 2
    for j, i in enumerate(above):
        row[i] = v + np.float32(0.1 * (j + 1))
    row[group] = v
    support = set(above) | {5, 200}
    r = step_ex(np.tile(row, (64, 1)), u=spread_u(64), temperature=0.7, top_p=top_p, top_k=6)
    assert np.array_equal(r["n_kept"], np.full(64, 6)), r["n_kept"]
    assert set(r["token"].tolist()) == support
    r = step_ex(np.tile(row, (64, 1)), u=spread_u(64), temperature=0.7, top_p=top_p, top_k=7)
    assert np.array_equal(r["n_kept"], np.full(64, 7)) and set(r["token"].tolist()) == support | {V - 7}


# ---- 4
def test_repetition_penalty_in_greedy_mode():
    V, S = 509, 16
    lg = np.full((8, V), -5.0, dtype=np.float32)
    ids = np.full((8, S), 300)
    gs, pos = np.full(8, 4), np.full(8, 8)
    # rows 0, 1: token 7 three times in the span, beside an id past the vocabulary and a negative one. Penalised once it stays in
    # front (4 / 1.5 = 2.67 > 2.5; -1 * 1.3 = -1.3 > -1.4), penalised twice it would not (1.78; -1.69)
    ids[0, 4:9] = ids[1, 4:9] = [7, V + 91, 7, -5, 7]
    lg[0, 7], lg[0, 9] = 4.0, 2.5
    lg[1, 7], lg[1, 9] = -1.0, -1.4
    r = step_ex(lg, ids=ids, pos=pos, gen_start=gs, S=S, repetition_penalty=1.5)
    assert r["token"][0] == 7
    r13 = step_ex(lg, ids=ids, pos=pos, gen_start=gs, S=S, repetition_penalty=1.3)
    assert r13["token"][1] == 7
    # rows 2, 3: a planted margin — the arg-max sits in R and falls to the runner-up when r crosses 2 (4 / r against 2; -1 * r
    # against -2): both sides of the ratio
    ids[2, 6] = ids[3, 6] = 11
    lg[2, 11], lg[2, 13] = 4.0, 2.0
    lg[3, 11], lg[3, 13] = -1.0, -2.0
    # row 4: an empty span (pos = gen_start - 1); row 5: the arg-max is the prompt token just in front of gen_start
    ids[4, :] = 21
    lg[4, 21], lg[4, 23] = 4.0, 3.9
    pos[4] = gs[4] - 1
    ids[5, :4] = 31
    lg[5, 31], lg[5, 33] = 4.0, 3.9
    # row 6: gen_start below 0 reads from position 0; row 7: a span of the whole row up to pos
    ids[6, 0] = 41
    gs[6] = -3
    lg[6, 41], lg[6, 43] = 4.0, 2.0
    ids[7, 0] = 51
    gs[7] = 0
    lg[7, 51], lg[7, 53] = 4.0, 2.0
    lo = step_ex(lg, ids=ids, pos=pos, gen_start=gs, S=S, repetition_penalty=1.9)
    hi = step_ex(lg, ids=ids, pos=pos, gen_start=gs, S=S, repetition_penalty=2.1)
    ref = torch.log_softmax(torch.from_numpy(lg).double(), -1)
    bound = max(4.0 * float((torch.log_softmax(torch.from_numpy(lg), -1).double() - ref).abs().max()), 1e-6)
    assert lo["token"][2:].tolist() == [11, 11, 21, 31, 41, 51]
    assert hi["token"][2:].tolist() == [13, 13, 21, 31, 43, 53]
    for r in (lo, hi):
        assert np.array_equal(r["logits_after"].view(np.uint32), lg.view(np.uint32))          # the logits are read only
        assert np.array_equal(r["n_kept"], np.ones(8))
        # the log-probability is the raw row's, whatever the penalty did to the pick
        assert np.abs(r["logprob"] - ref.numpy()[np.arange(8), r["token"]]).max() <= bound


@pytest.mark.parametrize("top_k", [0, 40])
@pytest.mark.parametrize("V,scale", VOCABS)
def test_repetition_penalty_in_sampling_mode(V, scale, top_k):
    """Spans of 9 ids with repeats, among them each row's five most likely tokens (so that the penalty reorders the head of the
    distribution), an id past the vocabulary and a negative one; r = 1.3, T = 0.8, top_p = 0.9."""
    S, T, top_p, rep = 16, 0.8, 0.9, 1.3
    rng = np.random.default_rng(7000 + V + top_k)
    lg = (scale * rng.standard_normal((16, V))).astype(np.float32)
    u = rng.random(16).astype(np.float32)
    ids = rng.integers(0, V, (16, S))
    head = np.argsort(-lg, axis=1)[:, :5]
    ids[:, 5:10] = head
    ids[:, 10] = head[:, 0]
    ids[:, 11] = V + 3
    ids[:, 12] = -1
    ids[:, 4] = head[:, 1]                            # (in front of gen_start: no part of R)
    gs, pos = np.full(16, 5), np.full(16, 13)
    spans = [ids[b, 5:14].tolist() for b in range(16)]
    r = step_ex(lg, u=u, ids=ids, pos=pos, gen_start=gs, S=S, temperature=T, top_p=top_p, top_k=top_k, repetition_penalty=rep)
    check_rows(r, lg, u, T, top_k, top_p, spans=spans, rep=rep)
    assert np.array_equal(r["logits_after"].view(np.uint32), lg.view(np.uint32))
    # an empty span is a no-op, bit for bit
    empty = step_ex(lg, u=u, ids=ids, pos=np.full(16, 4), gen_start=gs, S=S, temperature=T, top_p=top_p, top_k=top_k,
                    repetition_penalty=rep)
    plain = step_ex(lg, u=u, ids=ids, pos=np.full(16, 4), gen_start=gs, S=S, temperature=T, top_p=top_p, top_k=top_k)
    assert_same_bits(empty, plain)


# ---- 5
@pytest.mark.parametrize("V,scale", VOCABS)
def test_logprob_is_log_softmax_of_the_raw_logits(V, scale):
    rng = np.random.default_rng(V + 5)
    lg = (scale * rng.standard_normal((16, V))).astype(np.float32)
    u = rng.random(16).astype(np.float32)
    lg32 = torch.from_numpy(lg)
    ref = torch.log_softmax(lg32.double(), -1)
    # the bound: 4 x what torch's own fp32 log_softmax deviates from fp64 on these logits, floor 1e-6 (tests/test_beam_gpu.py)
    dev32 = float((torch.log_softmax(lg32, -1).double() - ref).abs().max())
    bound = max(4.0 * dev32, 1e-6)
    ids = rng.integers(0, V, (16, 16))
    worst = 0.0
    for kw in (dict(temperature=0.0), dict(temperature=0.8, top_p=0.95), dict(temperature=1.5, top_p=0.9, top_k=40),
               dict(temperature=0.7, top_p=1.0, top_k=8, repetition_penalty=1.3)):
        r = step_ex(lg, u=u, ids=ids, gen_start=np.zeros(16), **kw)
        want = ref.numpy()[np.arange(16), r["token"]]
        worst = max(worst, float(np.abs(r["logprob"] - want).max()))
        assert np.abs(r["logprob"] - want).max() <= bound, (kw, np.abs(r["logprob"] - want).max(), bound)
    print(f"V={V}: largest log-probability error {worst:.3e}, bound {bound:.3e} (torch fp32 log_softmax {dev32:.3e})")
    # one token in front by 30: every setting picks it, and its log-probability has the same bits under all of them
    lg[np.arange(16), np.arange(16) * 31 + 2] = np.float32(lg.max() + 30.0)
    ids[:, 0:4] = lg.argmax(1)[:, None] + 1           # R holds other tokens than the arg-max
    got = [step_ex(lg, u=u, ids=ids, gen_start=np.zeros(16), **kw)
           for kw in (dict(temperature=0.0), dict(temperature=0.7, top_p=1e-6), dict(temperature=1.5, top_p=1.0, top_k=1),
                      dict(temperature=1.0, top_p=0.5, top_k=40, repetition_penalty=1.7),
                      dict(temperature=0.0, repetition_penalty=1.2))]
    for g in got[1:]:
        assert np.array_equal(g["token"], lg.argmax(1))
        assert np.array_equal(g["logprob"].view(np.uint32), got[0]["logprob"].view(np.uint32))


# ---- 6
@pytest.mark.parametrize("B", [5, 20])
def test_counter_and_determinism(B):
    V, S = 32000, 16
    rng = np.random.default_rng(B)
    lg = (6.0 * rng.standard_normal((B, V))).astype(np.float32)
    lg[:, EOS] = -50.0
    lg[1, EOS] = 99.0                                 # row 1 takes the EOS (no other can), row 2 has no room, row 3 is done
    u = rng.random(B).astype(np.float32)
    ids = rng.integers(3, V, (B, S))
    pos, done = np.full(B, 6), np.zeros(B)
    pos[2], done[3] = S - 1, 1
    kw = dict(u=u, ids=ids, pos=pos, done=done, gen_start=np.full(B, 2), S=S, temperature=0.9, top_p=0.9, top_k=40,
              repetition_penalty=1.2, eos_id=EOS)
    counter = torch.zeros(1, dtype=torch.int32, device=DEV)
    a = step_ex(lg, counter=counter, **kw)
    assert a["n_active"] == B - 3 == int((a["done"] == 0).sum()) and a["counter"] == 0
    b = step_ex(lg, counter=counter, **kw)            # back to back on the same word, fresh copies of the inputs
    assert b["n_active"] == B - 3 and b["counter"] == 0
    assert_same_bits(a, b)
    emb = make_emb(V, 128, torch.float32)
    two = [torch.full((1,), -7, dtype=torch.int32, device=DEV) for _ in range(2)]
    st = [{k: torch.as_tensor(np.asarray(v), dtype=dt, device=DEV) for k, v, dt in
           (("ids", ids, torch.int64), ("pos", pos, torch.int32), ("done", done, torch.int32))} for _ in range(2)]
    i32 = lambda n: torch.zeros(n, dtype=torch.int32, device=DEV)               # noqa: E731
    lgd, ud, gsd = torch.from_numpy(lg).to(DEV), torch.from_numpy(u).to(DEV), torch.full((B,), 2, dtype=torch.int32, device=DEV)
    for k in range(2):                                # two launches queued with nothing between them
        ops.decode_next_ex(lgd, emb, st[k]["ids"], st[k]["pos"], st[k]["done"], gsd, torch.empty(B, 128, device=DEV), i32(B),
                           i32(B), torch.empty(B, device=DEV), two[k], counter, u=ud, temperature=0.9, top_p=0.9, top_k=40,
                           repetition_penalty=1.2, eos_id=EOS)
    torch.cuda.synchronize()
    assert int(two[0]) == int(two[1]) == B - 3 and int(counter) == 0


# ------------------------------------------------------------------------------------------------ end to end
def test_greedy_logprobs_are_beam_searchs_score(tiny):  # noqa: F811
    eng, batch = tiny.eng, tiny.batch
    print(f"per-token tolerance (greedy decode against one dense forward, times 4, floor 1e-5): {tiny.tol:.3e}")
    ref = generate.generate(eng, batch, temperature=0.0, stop_at_eos=True)
    out = generate.generate(eng, batch, temperature=0.0, stop_at_eos=True, return_logprobs=True)
    assert set(out) == set(ref) | {"logprobs", "sum_logprob"} and out["steps"] == ref["steps"]
    for k in ("ids", "n_generated", "tokens"):
        assert torch.equal(out[k], ref[k]), k
    assert out["logprobs"].dtype == torch.float32 and tuple(out["logprobs"].shape) == tuple(out["tokens"].shape)
    assert tuple(out["sum_logprob"].shape) == (len(tiny.prefix),)
    assert bool((out["logprobs"][out["tokens"] < 0] == 0).all()) and bool((out["logprobs"][out["tokens"] >= 0] < 0).all())
    one = generate.beam_search(eng, batch, stop_at_eos=True, num_beams=1)
    assert torch.equal(one["ids"], ref["ids"])
    for b in range(len(tiny.prefix)):
        n = int(out["n_generated"][b])
        got, want = float(out["sum_logprob"][b]), float(one["score"][b])
        print(f"sample {b}: {n} tokens, sum_logprob {got:.6f}, beam search (1 slot) {want:.6f}")
        assert abs(got - want) <= n * tiny.tol, (b, got, want)


def test_three_samples_per_prompt(tiny):  # noqa: F811
    eng, batch = tiny.eng, tiny.batch
    B, n, K, S = len(tiny.prefix), 3, 8, 128
    kw = dict(temperature=0.8, top_k=K, num_return_sequences=n, return_logprobs=True, stop_at_eos=True, max_new_tokens=12)
    out = generate.generate(eng, batch, seed=5, **kw)
    steps = out["steps"]
    assert tuple(out["ids"].shape) == (B, n, S) and tuple(out["n_generated"].shape) == (B, n)
    assert tuple(out["tokens"].shape) == (B, n, steps) == tuple(out["logprobs"].shape)
    assert tuple(out["sum_logprob"].shape) == (B, n) and out["tokens"].dtype == torch.int32
    again = generate.generate(eng, batch, seed=5, **kw)
    for k in ("ids", "tokens", "logprobs", "n_generated"):
        assert torch.equal(out[k], again[k]), k
    left_out = total = 0
    worst = 0.0
    for k in range(n):
        dense = dense_logits(eng, batch, out["ids"][:, k]).double()
        lp = dense.log_softmax(-1)
        for b, p in enumerate(tiny.prefix):
            assert torch.equal(out["ids"][b, k, :p].cpu(), batch["text_id"]["vqa"][b, 0, :p])  # the prompt of ITS sample
            m = int(out["n_generated"][b, k])
            assert 1 <= m <= 12
            for t in range(m):
                tok = int(out["ids"][b, k, p + t])
                assert tok == int(out["tokens"][b, k, t])
                d = abs(float(lp[b, p - 1 + t, tok]) - float(out["logprobs"][b, k, t]))
                worst = max(worst, d)
                assert d <= tiny.tol, (b, k, t, d, tiny.tol)            # (a wrong fan-out row would show here)
                top = dense[b, p - 1 + t].sort(descending=True)
                total += 1
                if float(top.values[K - 1] - top.values[K]) > GAP:
                    assert tok in top.indices[:K].tolist(), (b, k, t, tok)
                else:
                    left_out += 1
            assert bool((out["tokens"][b, k, m:] == -1).all()) and bool((out["logprobs"][b, k, m:] == 0).all())
    print(f"{total} sampled positions, {left_out} left out of the top-{K} check (gap at rank {K} <= {GAP}); largest difference "
          f"of a log-probability to the dense forward {worst:.3e}, tolerance {tiny.tol:.3e}")
    assert 4 * left_out <= total
    with pytest.raises(ValueError):
        generate.generate(eng, batch, temperature=0.0, num_return_sequences=2)


def test_top_k_of_one_samples_the_greedy_ids(tiny):  # noqa: F811
    eng, batch = tiny.eng, tiny.batch
    ref = generate.generate(eng, batch, temperature=0.0, stop_at_eos=True)
    one = generate.generate(eng, batch, temperature=1.0, top_k=1, seed=3, stop_at_eos=True)
    assert torch.equal(one["ids"], ref["ids"]) and torch.equal(one["tokens"], ref["tokens"])


def test_repetition_penalty_end_to_end_follows_the_rule():
    """The greedy answers of gen_eos_tiny_peakedperm hold no immediate repeat (the fixture's answers are a chain of distinct
    tokens), so this asserts what remains: at every token step the chosen token is the first arg-max of the penalised row, the
    rule restated in fp64 on the very logits and id rows the launch was given — where the restatement's two best are apart."""
    eng = model_of("tiny_peakedperm", torch.float32).ensure_engine()
    batch = eos_batch("tiny_peakedperm")
    rep = 1.3
    greedy = generate.generate(eng, batch, temperature=0.0, stop_at_eos=False, max_new_tokens=31)
    tok_g = greedy["tokens"].cpu().numpy()
    print("immediate repeats in the greedy run:", int((tok_g[:, 1:] == tok_g[:, :-1]).sum()))
    seen = []
    real = ops.decode_next_ex

    def spy(lg, emb, ids, pos, done, gen_start, *a, **k):
        seen.append((lg.cpu().numpy().copy(), ids.cpu().numpy().copy(), pos.cpu().numpy().copy(), gen_start.cpu().numpy().copy()))
        return real(lg, emb, ids, pos, done, gen_start, *a, **k)

    ops.decode_next_ex = spy
    try:
        out = generate.generate(eng, batch, temperature=0.0, stop_at_eos=False, max_new_tokens=31, repetition_penalty=rep)
    finally:
        ops.decode_next_ex = real
    tokens = out["tokens"].cpu().numpy()
    assert len(seen) == out["steps"] == 31 and tuple(tokens.shape) == (4, 31)
    undecided = 0
    for t, (lg, ids, pos, gs) in enumerate(seen):
        for b, p in enumerate(batch["prefix_index"]["vqa"]):
            assert gs[b] == p and pos[b] == p - 1 + t
            R = ids[b, gs[b]:pos[b] + 1].tolist()
            assert R == tokens[b, :t].tolist()                                  # the tokens generated so far, not the prompt
            l1 = penalised(lg[b], R, rep)
            best = np.sort(l1)[::-1]
            if best[0] - best[1] > GAP:
                assert int(tokens[b, t]) == int(l1.argmax()), (t, b)
            else:
                undecided += 1
    print(f"{4 * 31} token steps, {undecided} with the two best penalised logits within {GAP}")
    assert 4 * undecided <= 4 * 31


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_sixteen_bit_builds_sample_too(dtype):
    m = model_of("tiny_peakedperm", dtype)
    batch = eos_batch("tiny_peakedperm")
    kw = dict(temperature=0.8, top_k=8, top_p=0.95, repetition_penalty=1.2, num_return_sequences=2, return_logprobs=True,
              max_new_tokens=6, seed=1)
    out = generate.generate(m.ensure_engine(), batch, **kw)
    assert tuple(out["ids"].shape) == (4, 2, 128) and tuple(out["logprobs"].shape) == (4, 2, out["steps"])
    picked = out["tokens"] >= 0
    assert bool(torch.isfinite(out["logprobs"]).all()) and bool((out["logprobs"][picked] < 0).all())
    assert torch.allclose(out["sum_logprob"], out["logprobs"].sum(-1), rtol=0, atol=1e-5)
    assert torch.equal(out["tokens"], generate.generate(m.ensure_engine(), batch, **kw)["tokens"])
    ans = m.generate(batch, **kw)
    g = m.last_generation
    assert len(ans) == 4 and all(len(a) == 2 for a in ans) and {"logprobs", "sum_logprob"} <= set(g)
    for b, p in enumerate(batch["prefix_index"]["vqa"]):
        for k in range(2):
            row = g["ids"][b, k, p:p + int(g["n_generated"][b, k])].tolist()
            assert ans[b][k] == (row[:row.index(EOS)] if EOS in row else row)
