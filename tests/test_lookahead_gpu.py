"""Draft-and-verify greedy decoding on the GPU: the token step (fvqa_spec_step, csrc/spec.hip) against the numpy restatement of
tests/test_lookahead_cpu.py and, at T = 1, against fvqa_decode_next bit for bit; the suffix attention whose rows join the cache
(fvqa_attn_suffix_append, csrc/score.hip) against what fvqa_attn_decode stores and what fvqa_attn_suffix returns; then
`generate(lookahead=T)` end to end on the fixtures of tests/test_beam_gpu.py: the plain greedy call's ids, token for token."""
import numpy as np
import pytest
import torch

from fvqa import generate, ops, score
from tests.test_beam_gpu import GAP, ROWS, dense_logits, eos_batch, tiny  # noqa: F401  (tiny: the fixture and its tolerance)
from tests.test_eval import GOLDS, golden_batch
from tests.test_generate_gpu import model_of
from tests.test_lookahead_cpu import given_draft, lookup_draft, spec_step_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
EOS = 2
B_K, S_K, D_K = 5, 16, 128
MAX_NEW = 40
VOCABS = {509: 3.0, 32000: 6.0, 40003: 6.0}         # ragged strided tails | tests/test_sampling_gpu.py's row in LDS | beyond it
# make_rows' seed per (T, V): one for which the top two logits of every row of every pass are more than 10 * GAP apart wherever
# no tie is planted (asserted where the rows are compared: a seed that stops doing so fails the test)
SEEDS = {(1, 509): 0, (1, 32000): 0, (1, 40003): 0, (4, 509): 5, (4, 32000): 0, (4, 40003): 2, (16, 509): 29, (16, 32000): 20,
         (16, 40003): 3}
BITS = lambda t: t.contiguous().view(torch.uint8)   # noqa: E731


# ------------------------------------------------------------------------------------------------ the token step alone
def make_rows(T, V, seed):
    """Row cases for one (T, V): dicts of logits (T, V) fp32, w (T,), m, ids (S,), pos, done, ngen, drafts (MAX_NEW,), the set
    `ties` of logits rows with a planted tie, and a name. Pure numpy."""
    rng = np.random.default_rng(seed)
    scale = VOCABS[V]
    rows = []

    def new(name, *, m=T, pos=3, done=0, ngen=0):
        lg = (scale * rng.standard_normal((T, V))).astype(np.float32)
        r = dict(name=name, logits=lg, m=m, pos=pos, done=done, ngen=ngen, ties=set(),
                 ids=rng.integers(3, 9, S_K).astype(np.int64), w=np.full(T, -1, dtype=np.int32),
                 drafts=rng.integers(0, V, MAX_NEW).astype(np.int32))
        rows.append(r)
        return r

    def draft_from_argmax(r, upto, wrong=None):
        """w[1 .. upto] = what the model picks at rows 0 .. upto - 1; w[wrong] = another token."""
        am = r["logits"].argmax(1)
        for i in range(1, min(upto, T - 1) + 1):
            r["w"][i] = am[i - 1]
        if wrong is not None and wrong < T:
            r["w"][wrong] = (am[wrong - 1] + 1) % V

    for i in range(T):                                             # exactly i drafts accepted (0: none, T - 1: all)
        r = new(f"accept{i}", pos=min(3, S_K - 2 - i))
        draft_from_argmax(r, T - 1, wrong=i + 1)
    if T >= 2:
        r = new("short_pass", m=2)                                 # m < T: w[2] would match, but row 2 is not part of the pass
        draft_from_argmax(r, T - 1)
        r = new("eos_as_fresh_token", m=2)
        r["logits"][1, EOS] = r["logits"][1].max() + 5
        draft_from_argmax(r, 1)
        r = new("tie_rejects_the_higher_index")
        top = np.float32(r["logits"][0].max() + 1)
        r["logits"][0, 7] = r["logits"][0, 300] = top
        r["ties"].add(0)
        draft_from_argmax(r, T - 1)
        r["w"][1] = 300
        r = new("tie_accepts_the_lower_index")
        top = np.float32(r["logits"][0].max() + 1)
        r["logits"][0, 7] = r["logits"][0, 300] = top
        r["ties"].add(0)
        draft_from_argmax(r, T - 1)                                # (np.argmax: the first index, 7)
    if T >= 3:
        r = new("eos_among_the_accepted")
        r["logits"][1, EOS] = r["logits"][1].max() + 5
        draft_from_argmax(r, T - 1)
    r = new("eos_first")
    r["logits"][0, EOS] = r["logits"][0].max() + 5
    draft_from_argmax(r, T - 1)
    r = new("pos_S_minus_2", pos=S_K - 2)                          # one token fits, whatever the drafts say
    draft_from_argmax(r, T - 1)
    r = new("pos_S_minus_1", pos=S_K - 1)                          # no room: done, nothing written
    draft_from_argmax(r, T - 1)
    r = new("pos_minus_1", pos=-1)                                 # a row that starts at position 0
    draft_from_argmax(r, T - 1, wrong=3)
    r = new("budget", ngen=MAX_NEW - 2)                            # two tokens are left of max_new_tokens
    draft_from_argmax(r, T - 1)
    r = new("budget_spent", ngen=MAX_NEW)
    r = new("done_row", done=1)
    draft_from_argmax(r, T - 1)
    # given drafts that end: a -1, an id == V, a negative id, all behind one good entry; and one that starts with V + 5
    for k, bad in enumerate((-1, V, -7)):
        r = new(f"drafts_end_{k}", ngen=4)
        draft_from_argmax(r, 0)
        r["drafts"][5 + 1] = bad                                   # (after one commit n_generated = 5: drafts[5] is fed, [6] ends it)
    r = new("drafts_start_out_of_range", ngen=4)
    r["drafts"][5] = V + 5
    # prompt lookup: the two tokens this pass commits occur earlier in the row, the last one once more on its own
    r = new("lookup", m=min(T, 2), pos=8)
    draft_from_argmax(r, 1)
    am = r["logits"].argmax(1)
    t0, t1 = (int(am[0]), int(am[1])) if T >= 2 else (int(r["ids"][8]), int(am[0]))
    r["ids"][:8] = [t0, t1, 3, V + 9 if V + 9 < 2 ** 31 else 0, t0, t1, 4, t1]    # "t0 t1" ends at 1 and 5; "t1" at 7
    if T < 2:
        r["ids"][8] = t0
    r = new("lookup_out_of_range_id", m=1, pos=8)
    t1 = int(r["logits"][0].argmax())
    r["ids"][:9] = [t1, 5, V, 6, 7, 8, 3, 4, 5]                    # the match at e = 0 is followed by 5, then by an id == V
    return rows


def run_rows(rows, T, V, emb, src, G=2, counter=None, sync=True):
    """One launch on B = len(rows) row cases -> dict of host tensors (the in/out operands after the step included)."""
    B = len(rows)
    t = lambda a, dt: torch.as_tensor(np.asarray(a), dtype=dt, device=DEV).contiguous()   # noqa: E731
    i32 = lambda *s: torch.full(s, -7, dtype=torch.int32, device=DEV)                      # noqa: E731
    st = dict(logits=t(np.stack([r["logits"] for r in rows]).reshape(B * T, V), torch.float32),
              ids=t(np.stack([r["ids"] for r in rows]), torch.int64), pos=t([r["pos"] for r in rows], torch.int32),
              done=t([r["done"] for r in rows], torch.int32), ngen=t([r["ngen"] for r in rows], torch.int32),
              w=t(np.stack([r["w"] for r in rows]), torch.int32), len=t([r["m"] for r in rows], torch.int32),
              start=i32(B), x=torch.full((B * T, emb.shape[1]), float("nan"), dtype=emb.dtype, device=DEV),
              token=i32(B, T), logprob=torch.full((B, T), float("nan"), device=DEV), n_committed=i32(B), n_drafted=i32(B),
              n_active=i32(1), counter=torch.zeros(1, dtype=torch.int32, device=DEV) if counter is None else counter,
              pos64=torch.full((B,), -7, dtype=torch.int64, device=DEV))
    drafts = t(np.stack([r["drafts"] for r in rows]), torch.int32) if src == "given" else None
    ops.spec_step(st["logits"], emb, st["ids"], st["pos"], st["done"], st["ngen"], st["w"], st["len"], st["start"], st["x"],
                  st["token"], st["logprob"], st["n_committed"], st["n_drafted"], st["n_active"], st["counter"],
                  max_new_tokens=MAX_NEW, draft_tokens=drafts, lookup_ngram=G, pos64=st["pos64"], eos_id=EOS, stop_at_eos=True)
    if not sync:
        return st
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in st.items() if k != "logits"}


def check_rows(rows, got, T, V, emb, src, G=2):
    """Every row of a launch against the restatement; -> (rows still running, largest log-probability error, its bound)."""
    emb_h = emb.cpu()
    running, worst, bound_all = 0, 0.0, 0.0
    for b, r in enumerate(rows):
        want = spec_step_ref(r["logits"], r["w"], r["m"], r["ids"], r["pos"], r["done"], r["ngen"], T=T, eos_id=EOS,
                             max_new_tokens=MAX_NEW, drafts=r["drafts"] if src == "given" else None, G=G)
        what = (r["name"], src, G)
        nc = want["n_committed"]
        for i in range(nc):                                        # every argmax the comparison rests on is decided
            top = np.sort(r["logits"][i])[::-1]
            if i in r["ties"]:
                assert top[0] == top[1] and top[1] - top[2] > GAP, what
            else:
                assert top[0] - top[1] > GAP, (what, i, float(top[0] - top[1]))
        assert got["token"][b].tolist() == want["tokens"] + [-1] * (T - nc), what
        assert int(got["n_committed"][b]) == nc and int(got["n_drafted"][b]) == want["n_drafted"], what
        assert np.array_equal(got["ids"][b].numpy(), want["ids"]), what
        assert int(got["pos"][b]) == want["pos"] and int(got["ngen"][b]) == want["n_generated"], what
        assert int(got["done"][b]) == want["done"], what
        assert int(got["start"][b]) == want["start"] == int(got["pos64"][b]), what
        wn = want["w_next"]
        assert int(got["len"][b]) == len(wn), (what, int(got["len"][b]), wn)
        if want["live"]:
            assert got["w"][b].tolist() == wn + [-1] * (T - len(wn)), (what, got["w"][b].tolist(), wn)
        else:                                                      # a row that committed nothing keeps its state
            assert got["w"][b].tolist() == r["w"].tolist() and np.array_equal(got["ids"][b].numpy(), r["ids"]), what
            assert int(got["pos"][b]) == r["pos"] and int(got["ngen"][b]) == r["ngen"], what
        feed = wn if wn else [want["w0"]]                          # (a row that feeds nothing stays a valid row)
        x = got["x"][b * T:(b + 1) * T]
        for j in range(T):
            ref = emb_h[feed[j]] if j < len(feed) else torch.zeros_like(emb_h[0])
            assert torch.equal(BITS(x[j]), BITS(ref)), (what, j)
        lg32 = torch.from_numpy(r["logits"][:max(nc, 1)])
        dev32 = float((torch.log_softmax(lg32, -1).double() - torch.log_softmax(lg32.double(), -1)).abs().max())
        bound = max(4.0 * dev32, 1e-6)       # 4 x what torch's own fp32 log_softmax deviates from fp64 on these rows (floor 1e-6)
        for i in range(T):
            lp = float(got["logprob"][b, i])
            if i < nc:
                worst, bound_all = max(worst, abs(lp - want["logprobs"][i])), max(bound_all, bound)
                assert abs(lp - want["logprobs"][i]) <= bound, (what, i, lp, want["logprobs"][i], bound)
            else:
                assert lp == 0.0, (what, i)
        running += want["done"] == 0
    return running, worst, bound_all


def assert_cases_are_what_they_say(rows, T):
    """What the row cases are there for does happen, by the restatement (no device needed)."""
    by = {r["name"]: r for r in rows}
    ref = lambda r, **k: spec_step_ref(r["logits"], r["w"], r["m"], r["ids"], r["pos"], r["done"], r["ngen"], T=T,   # noqa: E731
                                       max_new_tokens=MAX_NEW, **k)
    for i in range(T):
        r = by[f"accept{i}"]
        assert ref(r, drafts=r["drafts"])["n_committed"] == i + 1 and r["m"] == T
    assert ref(by["pos_S_minus_2"])["n_committed"] == 1 and ref(by["pos_S_minus_2"])["w_next"] == []
    assert ref(by["budget"])["n_committed"] == min(T, 2) and ref(by["budget"])["done"] == (1 if T >= 2 else 0)
    assert ref(by["eos_first"])["tokens"] == [EOS] and not ref(by["done_row"])["live"] and not ref(by["budget_spent"])["live"]
    if T >= 2:
        assert ref(by["tie_rejects_the_higher_index"])["tokens"] == [7] and ref(by["tie_accepts_the_lower_index"])["tokens"][0] == 7
        assert ref(by["tie_accepts_the_lower_index"])["n_committed"] == min(T, S_K - 1 - 3)     # all of them, up to the row's end
        assert ref(by["short_pass"])["n_committed"] == 2 and ref(by["eos_as_fresh_token"])["tokens"][-1] == EOS
        for k in range(3):
            assert len(ref(by[f"drafts_end_{k}"], drafts=by[f"drafts_end_{k}"]["drafts"])["w_next"]) == 2
        assert len(ref(by["drafts_start_out_of_range"], drafts=by["drafts_start_out_of_range"]["drafts"])["w_next"]) == 1
        lk = by["lookup"]
        assert ref(lk, G=2)["w_next"][1:3] == [4, int(lk["ids"][7])][:T - 1]       # the 2-gram's later occurrence, at e = 5
        assert ref(by["lookup_out_of_range_id"], G=2)["w_next"][1:] == [5]         # ended in front of the id == V
    if T >= 3:
        assert ref(by["eos_among_the_accepted"])["tokens"][-1] == EOS and ref(by["eos_among_the_accepted"])["n_committed"] == 2


def chunks(rows):
    for k in range(0, len(rows), B_K):
        part = rows[k:k + B_K]
        yield part + rows[:B_K - len(part)]                        # (the last launch is filled up: B = 5 throughout)


def make_emb(V, dtype):
    return torch.randn(V, D_K, generator=torch.Generator().manual_seed(1)).to(dtype).to(DEV)


CASES_K = [(T, V, torch.float32) for T in (1, 4, 16) for V in VOCABS] + [(4, 509, torch.bfloat16), (4, 509, torch.float16)]


@pytest.mark.parametrize("T,V,dtype", CASES_K)
def test_spec_step_follows_the_rule(T, V, dtype):
    rows = make_rows(T, V, SEEDS[T, V])
    names = {r["name"] for r in rows}
    assert {f"accept{i}" for i in range(T)} <= names and {"pos_S_minus_2", "done_row", "budget", "lookup"} <= names
    emb = make_emb(V, dtype)
    worst = bound = 0.0
    for src, G in (("given", 2), ("lookup", 2)):
        for part in chunks(rows):
            got = run_rows(part, T, V, emb, src, G)
            running, w_, b_ = check_rows(part, got, T, V, emb, src, G)
            worst, bound = max(worst, w_), max(bound, b_)
            assert int(got["n_active"]) == running and int(got["counter"]) == 0, (src, [r["name"] for r in part])
    print(f"T={T} V={V} {dtype}: {len(rows)} row cases under both draft sources, largest log-probability error {worst:.3e} "
          f"(largest bound {bound:.3e})")
    assert_cases_are_what_they_say(rows, T)


@pytest.mark.parametrize("G", [1, 2, 4])
def test_prompt_lookup_on_the_device(G):
    """The lookup rows of the T = 4 cases under every n-gram length, plus id rows of a small alphabet at positions near the end of
    the sequence: many matches, n-grams that fall back, drafts cut by the room and by P - e."""
    T, V = 4, 509
    emb = make_emb(V, torch.float32)
    rows = [r for r in make_rows(T, V, SEEDS[T, V]) if r["name"].startswith("lookup")]
    rng = np.random.default_rng(11 + G)
    for k in range(B_K * 3 - len(rows)):
        lg = (3.0 * rng.standard_normal((T, V))).astype(np.float32)
        lg[0, 3 + k % 3] = lg[0].max() + 2                         # the committed token is of the alphabet
        rows.append(dict(name=f"alphabet{k}", logits=lg, m=1, pos=int(rng.integers(2, S_K - 1)), done=0, ngen=k % 5, ties=set(),
                         ids=rng.integers(3, 6, S_K).astype(np.int64), w=np.full(T, -1, dtype=np.int32),
                         drafts=np.zeros(MAX_NEW, dtype=np.int32)))
    n_draft = 0
    for part in chunks(rows):
        got = run_rows(part, T, V, emb, "lookup", G)
        running, _, _ = check_rows(part, got, T, V, emb, "lookup", G)
        assert int(got["n_active"]) == running and int(got["counter"]) == 0
        n_draft += int((got["len"] > 1).sum())
    print(f"G={G}: {n_draft} of {len(rows)} rows found a draft")
    assert n_draft >= len(rows) // 2


DONE0 = [0, 0, 0, 1, 0]
POS0 = [3, S_K - 2, S_K - 1, 6, -1]                 # row 1 fills the sequence, row 2 has no room, row 4 starts at position 0


@pytest.mark.parametrize("V,dtype", [(V, torch.float32) for V in VOCABS] + [(509, torch.bfloat16), (509, torch.float16)])
def test_one_row_per_pass_is_decode_next_bit_for_bit(V, dtype):
    rng = np.random.default_rng(V)
    lg = (VOCABS[V] * rng.standard_normal((B_K, V))).astype(np.float32)
    lg[1, EOS] = lg[1].max() + 3                                   # an EOS, written into the last position
    lg[4, 9] = lg[4, 200] = np.float32(lg[4].max() + 1)            # an exact tie
    ids0 = rng.integers(3, 400, (B_K, S_K)).astype(np.int64)
    ids0[3, 6] = V + 11                                            # a done row on an id outside the vocabulary: clamped alike
    emb = make_emb(V, dtype)
    t = lambda a, dt: torch.as_tensor(np.asarray(a), dtype=dt, device=DEV).contiguous()   # noqa: E731
    i32 = lambda *s: torch.full(s, -7, dtype=torch.int32, device=DEV)                      # noqa: E731
    for stop in (True, False):
        a = dict(ids=t(ids0, torch.int64), pos=t(POS0, torch.int32), done=t(DONE0, torch.int32),
                 x=torch.full((B_K, D_K), float("nan"), dtype=dtype, device=DEV), token=i32(B_K), n_active=i32(1),
                 pos64=torch.full((B_K,), -7, dtype=torch.int64, device=DEV))
        ops.decode_next(t(lg, torch.float32), emb, a["ids"], a["pos"], a["done"], a["x"], a["token"], i32(B_K), a["n_active"],
                        pos64=a["pos64"], temperature=0.0, eos_id=EOS, stop_at_eos=stop)
        b = dict(ids=t(ids0, torch.int64), pos=t(POS0, torch.int32), done=t(DONE0, torch.int32),
                 x=torch.full((B_K, D_K), float("nan"), dtype=dtype, device=DEV), token=i32(B_K, 1), n_active=i32(1),
                 pos64=torch.full((B_K,), -7, dtype=torch.int64, device=DEV))
        counter = torch.zeros(1, dtype=torch.int32, device=DEV)
        ops.spec_step(t(lg, torch.float32), emb, b["ids"], b["pos"], b["done"], torch.zeros(B_K, dtype=torch.int32, device=DEV),
                      i32(B_K, 1), torch.ones(B_K, dtype=torch.int32, device=DEV), i32(B_K), b["x"], b["token"],
                      torch.empty(B_K, 1, device=DEV), i32(B_K), i32(B_K), b["n_active"], counter, max_new_tokens=MAX_NEW,
                      lookup_ngram=2, pos64=b["pos64"], eos_id=EOS, stop_at_eos=stop)
        torch.cuda.synchronize()
        for k in a:
            assert torch.equal(BITS(a[k]), BITS(b[k].view_as(a[k]))), (k, stop, a[k], b[k])
        assert a["token"].tolist()[2:4] == [-1, -1] and int(a["token"][4]) == 9 and int(counter) == 0
        assert a["done"].tolist() == ([0, 1, 1, 1, 0] if stop else [0, 0, 1, 1, 0])


def test_two_launches_back_to_back_on_one_counter():
    T, V = 4, 32000
    rows = make_rows(T, V, SEEDS[T, V])[:B_K]
    emb = make_emb(V, torch.float32)
    counter = torch.zeros(1, dtype=torch.int32, device=DEV)
    a = run_rows(rows, T, V, emb, "given", counter=counter, sync=False)    # queued with nothing between them
    b = run_rows(rows, T, V, emb, "given", counter=counter, sync=False)
    torch.cuda.synchronize()
    assert int(counter) == 0 and int(a["n_active"]) == int(b["n_active"]) == int((a["done"] == 0).sum())
    for k in a:
        assert torch.equal(BITS(a[k]), BITS(b[k])), k
    check_rows(rows, {k: v.cpu() for k, v in a.items()}, T, V, emb, "given")


def test_the_wrapper_refuses_bad_operands():
    T, V = 4, 509
    rows = make_rows(T, V, SEEDS[T, V])[:B_K]
    emb = make_emb(V, torch.float32)
    with pytest.raises(ValueError):
        run_rows(rows, T, V, emb, "lookup", G=5)
    with pytest.raises(ValueError):
        run_rows(rows, T, V, make_emb(V + 1, torch.float32), "lookup")
    rows17 = [dict(r, logits=np.zeros((17, V), np.float32), w=np.full(17, -1, np.int32)) for r in rows]
    with pytest.raises(ValueError):
        run_rows(rows17, 17, V, emb, "lookup")


# ------------------------------------------------------------------------------------------------ the rows join the cache
N_A, S_A, H_A, DH_A, A_A, F_A, T_A = 3, 32, 2, 128, 10, 10, 4
APPEND_CASES = [([5, S_A - 4, S_A - 1], [4, 4, 1]),                # start + len reaches S for two sequences
                ([7, S_A - 1, S_A - 4], [0, 1, 4]),                # a sequence that feeds nothing
                ([S_A - 2, 0, 12], [4, 1, 0])]                     # len beyond the end of the sequence is cut; an empty cache


@pytest.mark.parametrize("dtype,rotated", [(torch.float32, True), (torch.bfloat16, True), (torch.bfloat16, False),
                                           (torch.float16, True), (torch.float16, False)])
@pytest.mark.parametrize("start,length", APPEND_CASES)
def test_append_stores_what_attn_decode_stores_and_returns_what_attn_suffix_returns(start, length, dtype, rotated):
    D = H_A * DH_A
    g = torch.Generator().manual_seed(len(str(dtype)) + 7 * start[0])
    rnd = lambda *s: (1.5 * torch.randn(*s, generator=g)).to(dtype).to(DEV)     # noqa: E731
    before = rnd(N_A * S_A + A_A, 3 * D)                           # sentinels everywhere: whatever is written that should not be, shows
    suf = rnd(N_A * T_A, 3 * D)
    g1, g2 = torch.randn(H_A, generator=g).to(DEV), torch.randn(H_A, generator=g).to(DEV)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)               # noqa: E731
    vstart, st, ln = i32([1, 3, 20]), i32(start), i32(length)
    ang = torch.arange(S_A).float()[:, None] * (10000.0 ** (-torch.arange(0, DH_A, 2).float() / DH_A))[None]
    rope = (ang.cos().contiguous().to(DEV), ang.sin().contiguous().to(DEV))
    cache = before.clone()
    o = torch.full((N_A * T_A, D), float("nan"), dtype=dtype, device=DEV)
    ops.attn_suffix_append(suf, cache, o, g1, g2, vstart, st, ln, rope, N_A, T_A, S_A, H_A, DH_A, A_A, F_A, cache_rotated=rotated)
    # the same raw rows one by one through attn_decode, each on a cache of its own; what it stores depends on the row and its position
    want = before.clone()
    for j in range(T_A):
        scratch = before.clone()
        pos = torch.tensor([min(s + j, S_A - 1) for s in start], dtype=torch.int64, device=DEV)
        ops.attn_decode(suf.view(N_A, T_A, 3 * D)[:, j].contiguous(), scratch, torch.empty(N_A, D, dtype=dtype, device=DEV), g1, g2,
                        vstart, pos, rope, N_A, S_A, H_A, DH_A, A_A, F_A, cache_rotated=rotated)
        for n in range(N_A):
            if j < min(length[n], S_A - start[n]):
                row = n * S_A + start[n] + j
                want[row, D:] = scratch[row, D:]
    o_ref = torch.full((N_A * T_A, D), float("nan"), dtype=dtype, device=DEV)
    ops.attn_suffix(suf, before.clone(), o_ref, g1, g2, vstart, st, ln, rope, N_A, 1, T_A, S_A, H_A, DH_A, A_A, F_A,
                    cache_rotated=rotated)
    torch.cuda.synchronize()
    assert torch.equal(BITS(cache), BITS(want))                    # k and v of the fed rows as attn_decode stores them; nothing else
    n_rows = sum(min(ln_, S_A - s) for s, ln_ in zip(start, length))
    assert int((BITS(cache) != BITS(before)).any(1).sum()) == n_rows
    assert torch.equal(BITS(cache[:, :D]), BITS(before[:, :D]))    # the q third
    assert torch.equal(BITS(o), BITS(o_ref))
    assert bool(torch.isfinite(o.float()).all())


# ------------------------------------------------------------------------------------------------ end to end
def trimmed(tokens):
    """A plain call's "tokens" (B, steps) without the all -1 columns its superfluous last step may have left."""
    keep = int((tokens >= 0).any(0).sum())
    assert bool((tokens[:, keep:] == -1).all())
    return tokens[:, :keep]


def drafts_of(plain, max_new):
    d = torch.full((plain["tokens"].shape[0], max_new), -1, dtype=torch.int32)
    tk = trimmed(plain["tokens"]).cpu()
    d[:, :tk.shape[1]] = tk
    return d


def predict_commits(true_tokens, prompt_row, p, *, T, max_new, S, V, stop=True, drafts=None, G=2):
    """What each token step commits for one row, by the restatement: the model's pick behind a correct prefix is the plain greedy
    run's next token, so only the drafts decide how far a pass gets. -> the list of n_committed up to the step that ends the row."""
    ids = [int(x) for x in prompt_row]
    pos, ngen, done, w, out = p - 1, 0, False, [], []
    while not done and pos + 1 < S and ngen < max_new:
        m, nc = max(1, len(w)), 0
        for i in range(m):
            g = int(true_tokens[ngen])
            pos, ngen, nc = pos + 1, ngen + 1, nc + 1
            ids[pos] = g
            if (stop and g == EOS) or ngen == max_new:
                done = True
                break
            if pos + 1 >= S or i + 1 >= m or w[i + 1] != g:
                break
        out.append(nc)
        room = 0 if done else min(T, max_new - ngen, S - 1 - pos)
        w = [] if room < 1 else [g] + (given_draft(drafts, ngen, room - 1, V) if drafts is not None
                                      else lookup_draft(ids, pos, G, room - 1, V))
    return out


def same_answer(out, plain, what):
    for k in ("ids", "n_generated"):
        assert torch.equal(out[k], plain[k]), (what, k)
    assert torch.equal(out["tokens"], trimmed(plain["tokens"])), what
    assert out["tokens"].dtype == torch.int32 and out["n_committed"].dtype == out["n_drafted"].dtype == torch.int32
    B = out["ids"].shape[0]
    assert tuple(out["n_committed"].shape) == tuple(out["n_drafted"].shape) == (B, out["steps"])
    assert torch.equal(out["n_committed"].sum(1).to(torch.int64), out["n_generated"]), what


def assert_commits(out, plain, batch, what, *, T, max_new, stop, drafts=None, G=2):
    tk = plain["tokens"].cpu().tolist()
    for b, p in enumerate(batch["prefix_index"]["vqa"]):
        want = predict_commits(tk[b], batch["text_id"]["vqa"][b, 0].tolist(), p, T=T, max_new=max_new, S=128, V=32000, stop=stop,
                               drafts=None if drafts is None else drafts[b].tolist(), G=G)
        got = out["n_committed"][b].tolist()
        assert got == want + [0] * (len(got) - len(want)), (what, b, got, want)


@pytest.mark.parametrize("stop,max_new", [(True, 31), (False, 12), (False, 31)])
def test_oracle_drafts_give_the_plain_answer_in_a_quarter_of_the_passes(tiny, stop, max_new):  # noqa: F811
    eng, batch, T = tiny.eng, tiny.batch, 4
    plain = generate.generate(eng, batch, temperature=0.0, stop_at_eos=stop, max_new_tokens=max_new)
    drafts = drafts_of(plain, max_new)
    out = generate.generate(eng, batch, temperature=0.0, stop_at_eos=stop, max_new_tokens=max_new, lookahead=T,
                            draft_tokens=drafts)
    assert set(out) == set(plain) | {"n_committed", "n_drafted"}
    same_answer(out, plain, "oracle")
    n = plain["n_generated"].tolist()
    print(f"plain: {plain['steps']} steps for {n} tokens; lookahead {T} with the answer as draft: {out['steps']} steps, "
          f"committed per step {out['n_committed'].tolist()}")
    for b in range(len(n)):
        got, left = out["n_committed"][b].tolist(), n[b] - 1
        assert got[0] == 1                                         # the first step has no draft: the prefill's row alone
        for s in range(1, out["steps"]):                           # every later pass: min(T, what is left)
            assert got[s] == min(T, left), (b, s, got)
            left -= got[s]
        assert left == 0
    assert out["steps"] <= 1 + -(-(max(n) - 1) // T) + 2 < plain["steps"]
    assert_commits(out, plain, batch, "oracle", T=T, max_new=max_new, stop=stop, drafts=drafts)
    assert out["n_drafted"][:, 0].tolist() == [0] * len(n) and int(out["n_drafted"].max()) == T - 1


@pytest.mark.parametrize("T", [2, 4, 16])
def test_corrupted_drafts_leave_the_ids_alone(tiny, T):  # noqa: F811
    """Wrong draft tokens at chosen indices: rejected drafts leave k / v in cache rows behind the row's position, and the next
    pass must not read them — a stale row would change a logit and, on these peaked rows, a token or at least a count."""
    eng, batch, max_new = tiny.eng, tiny.batch, 31
    plain = generate.generate(eng, batch, temperature=0.0, stop_at_eos=False, max_new_tokens=max_new)
    drafts = drafts_of(plain, max_new)
    for b, at in ((0, (1, 2, 9, 10, 11, 20)), (1, (3, 4, 7, 13, 30))):
        for k in at:
            drafts[b, k] = (drafts[b, k] + 1 + k) % 32000
    drafts[1, 17] = -1                                             # a draft that ends early
    drafts[0, 25] = 32000                                          # ... and one that ends at an id outside the vocabulary
    out = generate.generate(eng, batch, temperature=0.0, stop_at_eos=False, max_new_tokens=max_new, lookahead=T,
                            draft_tokens=drafts)
    same_answer(out, plain, f"corrupted T={T}")
    assert_commits(out, plain, batch, f"corrupted T={T}", T=T, max_new=max_new, stop=False, drafts=drafts)
    print(f"T={T}: {out['steps']} steps, committed per step {out['n_committed'].tolist()}, drafted {out['n_drafted'].tolist()}")
    assert int((out["n_committed"] < out["n_drafted"] + 1).sum()) >= 5         # drafts were rejected


@pytest.mark.parametrize("G", [1, 2])
def test_prompt_lookup_gives_the_plain_answer(tiny, G):  # noqa: F811
    eng, batch, T = tiny.eng, tiny.batch, 4
    for stop, max_new in ((True, 31), (False, 31)):
        plain = generate.generate(eng, batch, temperature=0.0, stop_at_eos=stop, max_new_tokens=max_new)
        out = generate.generate(eng, batch, temperature=0.0, stop_at_eos=stop, max_new_tokens=max_new, lookahead=T, lookup_ngram=G)
        same_answer(out, plain, f"lookup G={G}")
        assert_commits(out, plain, batch, f"lookup G={G}", T=T, max_new=max_new, stop=stop, G=G)
        drafted, accepted = int(out["n_drafted"].sum()), int((out["n_committed"] - 1).clamp(min=0).sum())
        print(f"G={G} stop_at_eos={stop}: {out['steps']} steps against {plain['steps']}, {drafted} tokens drafted, {accepted} "
              f"accepted; committed per step {out['n_committed'].tolist()}")


def test_logprobs_are_the_dense_forwards(tiny):  # noqa: F811
    eng, batch, T = tiny.eng, tiny.batch, 4
    tol = tiny.tol
    full = eos_batch("tiny_peakedperm", ROWS)
    plan = score.plan_options(full["text_id"]["vqa"], full["label"]["vqa"], None, full["video_start"]["vqa"], eng.F)
    if plan.shared:     # the suffix attention reduces in another order than the one-row kernel: what that costs EXISTING code
        il = [score.score_options(eng, full, route=r)["individual_losses"].double() for r in ("shared", "dense")]
        routes = float((il[0] - il[1]).abs().max())
        tol = max(tol, 4.0 * routes)
        print(f"score_options shared route against dense on this fixture: largest per-token difference {routes:.3e}")
    print(f"per-token tolerance {tol:.3e} (greedy decode against one dense forward, times 4, floor 1e-5: {tiny.tol:.3e})")
    plain = generate.generate(eng, batch, temperature=0.0, stop_at_eos=True, return_logprobs=True)
    worst = 0.0
    for kw in (dict(draft_tokens=drafts_of(plain, 31)), dict(lookup_ngram=2)):
        out = generate.generate(eng, batch, temperature=0.0, stop_at_eos=True, return_logprobs=True, lookahead=T, **kw)
        same_answer(out, plain, "logprobs")
        assert tuple(out["logprobs"].shape) == tuple(out["tokens"].shape) and out["logprobs"].dtype == torch.float32
        assert bool((out["logprobs"][out["tokens"] < 0] == 0).all()) and bool((out["logprobs"][out["tokens"] >= 0] < 0).all())
        assert torch.allclose(out["sum_logprob"], out["logprobs"].sum(1), rtol=0, atol=1e-6)
        lp = dense_logits(eng, batch, out["ids"]).double().log_softmax(-1)
        for b, p in enumerate(tiny.prefix):
            for t in range(int(out["n_generated"][b])):
                d = abs(float(lp[b, p - 1 + t, int(out["ids"][b, p + t])]) - float(out["logprobs"][b, t]))
                worst = max(worst, d)
                assert d <= tol, (b, t, d, tol)
    print(f"largest difference of a log-probability to the dense forward {worst:.3e}")


def dense_argmax_check(eng, batch, out, what):
    """Every generated token, teacher-forced through one dense forward, is the dense argmax wherever the dense top-two gap
    exceeds GAP; at most a quarter of the positions may lie within it."""
    dense = dense_logits(eng, batch, out["ids"]).float()
    left_out = total = 0
    for b, p in enumerate(batch["prefix_index"]["vqa"]):
        n = int(out["n_generated"][b])
        assert n >= 1 and out["tokens"][b, :n].tolist() == out["ids"][b, p:p + n].tolist(), (what, b)
        assert bool((out["tokens"][b, n:] == -1).all())
        for t in range(n):
            top = dense[b, p - 1 + t].topk(2)
            total += 1
            if float(top.values[0] - top.values[1]) > GAP:
                assert int(out["ids"][b, p + t]) == int(top.indices[0]), (what, b, t)
            else:
                left_out += 1
    print(f"{what}: {total} generated positions, {left_out} within {GAP} of a tie and left out; {out['steps']} steps, "
          f"committed per step (row 0) {out['n_committed'][0].tolist()}")
    assert 4 * left_out <= total, (what, left_out, total)
    assert torch.equal(out["n_committed"].sum(1).to(torch.int64), out["n_generated"])


@pytest.mark.parametrize("pname,dtype", [("tiny_peakedperm", torch.bfloat16), ("tiny_peakedperm", torch.float16),
                                         ("7b_l2_peakedperm", torch.bfloat16)])
def test_sixteen_bit_builds(pname, dtype):
    eng = model_of(pname, dtype).ensure_engine()
    batch = eos_batch(pname)
    plain = generate.generate(eng, batch, temperature=0.0, stop_at_eos=True)
    for kw in (dict(draft_tokens=drafts_of(plain, 31)), dict(lookup_ngram=2)):
        out = generate.generate(eng, batch, temperature=0.0, stop_at_eos=True, lookahead=4, **kw)
        dense_argmax_check(eng, batch, out, f"{pname} {dtype} {sorted(kw)}")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_eighty_rows_per_pass(dtype):
    """The 7b_l2_peaked batch five times over at T = 4: B * T = 80 rows, beyond the few-rows projections' 64."""
    eng = model_of("7b_l2_peaked", dtype).ensure_engine()
    one = golden_batch(GOLDS["7b_l2_peaked"])
    rep = lambda t: torch.cat([t] * 5)                  # noqa: E731
    batch = {"video": rep(one["video"]), "text_id": {"vqa": rep(one["text_id"]["vqa"])},
             "label": {"vqa": rep(one["label"]["vqa"])}, "video_start": {"vqa": one["video_start"]["vqa"] * 5},
             "prefix_index": {"vqa": one["prefix_index"]["vqa"] * 5}}
    plain = generate.generate(eng, batch, temperature=0.0, stop_at_eos=False, max_new_tokens=31)
    out = generate.generate(eng, batch, temperature=0.0, stop_at_eos=False, max_new_tokens=31, lookahead=4,
                            draft_tokens=drafts_of(plain, 31))
    assert tuple(out["ids"].shape) == (20, 128) and out["n_generated"].tolist() == [31] * 20
    dense_argmax_check(eng, batch, out, f"B = 20, T = 4, {dtype}")
    assert out["steps"] < plain["steps"]
