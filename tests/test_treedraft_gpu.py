"""Tree-shaped draft verification on the GPU: fvqa_tree_spec_step on synthetic logits against the numpy restatement
(tests/test_treedraft_cpu.py tree_step_ref), every output word for word; fvqa_kv_tree_commit against the bits
fvqa_attn_suffix_append stores for the same raw rows; generate(lookahead=R, draft_answers=C) end to end against the plain greedy
call, token for token."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from fvqa import generate, ops, vocab
from tests.test_beam_gpu import ROWS, dense_logits, eos_batch, tiny  # noqa: F401  (tiny: the fixture and its tolerance)
from tests.test_generate_gpu import model_of
from tests.test_lookahead_gpu import dense_argmax_check, trimmed
from tests.test_treedraft_cpu import plan_of, predict_passes, sample_plan, tree_step_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
EOS = 2
S_K, D_K, MAX_NEW = 48, 24, 40
WALK, TILE = 32, 32
BITS = lambda t: t.contiguous().view(torch.uint8)   # noqa: E731
GUARD = 64


# ------------------------------------------------------------------------------------------------ the step kernel
C30 = list(range(100, 131))                                        # a chain of 31 tokens
PLANS = {
    "sib": [[5, 6, 7], [5, 8, 9], [5, 9], [11]],                   # rows: 0 root 1 "5" 2 "5 6" 3 "5 6 7" 4 "5 8" 5 "5 8 9" 6 "5 9" 7 "11"
    "chain40": [list(range(100, 140))],                            # relative depth reaches 39: cut at 31
    "edge31": [C30 + [200], C30 + [201]],                          # under "100": local rows 31, 32 at relative depth 31
    "edge1": [[400, 300 + i] for i in range(40)],                  # under "400": local row 32 at relative depth 1
    "prefix": [[5, 6], [5, 6, 7, 8]],
}


def broken(kind):
    """The "sib" plan with one array out of range (a per-sample plan of 8 rows)."""
    n, tok, dep, end, par = sample_plan(plan_of(PLANS["sib"], V=509), 0)
    tok, dep, end, par = tok.copy(), dep.copy(), end.copy(), par.copy()
    if kind == "end":
        end[:] = [2 ** 30, -5, 1, 100, 0, 2 ** 31 - 1, -2 ** 31, 9]
    elif kind == "parent":
        par[:] = [7, 2 ** 30, -9, 1, 1, 1, 6, -2 ** 31]
    elif kind == "token":
        tok[:] = [-1, 5, 2 ** 30, -3, 8, 600, 9, 509]
    elif kind == "depth":
        dep[:] = [2 ** 31 - 1, -2 ** 31, 5, 0, 77, -1, 2 ** 30, 3]
    elif kind == "n_plan":
        n = 2 ** 30
    return n, tok, dep, end, par


def case(name, plan, node, m, peaks, *, pos=5, done=0, ngen=1, ties=()):
    return dict(name=name, plan=plan, node=node, m=m, peaks=peaks, pos=pos, done=done, ngen=ngen, ties=ties)


def cases_for(R):
    sib = lambda *a, **k: case(a[0], "sib", *a[1:], **k)           # noqa: E731
    out = [
        sib("whole member to its EOS (the middle sibling)", 1, 6, {0: 8, 3: 9, 4: EOS}),
        sib("first sibling", 1, 6, {0: 6, 1: 7, 2: EOS}),
        sib("last sibling", 1, 6, {0: 9, 5: EOS}),
        sib("leaves at the root", 0, 1, {0: 30}),
        sib("leaves at depth 1", 1, 6, {0: 30}),
        sib("leaves at depth 2", 1, 6, {0: 6, 1: 30}),
        sib("first step", 0, 1, {0: 5}),
        sib("first step to the last child of the root", 0, 1, {0: 11}),
        sib("from the root over the whole plan", 0, 8, {0: 5, 1: 8, 4: 9, 5: 7}),
        sib("eos inside the walk", 0, 8, {0: 5, 1: EOS}),
        sib("node -1", -1, 6, {0: 5, 1: 6}),
        sib("node outside the plan", 99, 6, {0: 5, 1: 6}),
        sib("len 0 reads as 1", 1, 0, {0: 8, 3: 9}),
        sib("len beyond the plan's end", 6, 6, {0: EOS}),
        sib("tie on the trie: the lower index is a child", 1, 6, {0: 6, 1: 7}, ties=[(0, 6, 8)]),
        sib("tie on the trie: the lower index is no child", 1, 6, {0: 4}, ties=[(0, 4, 8)]),
        sib("tie off the trie", -1, 1, {0: 17}, ties=[(0, 17, 300)]),
        sib("done row", 1, 6, {0: 8}, done=1),
        sib("budget spent", 1, 6, {0: 8}, ngen=MAX_NEW),
        sib("no room", 1, 6, {0: 8}, pos=S_K - 1),
        sib("position -1", 0, 1, {0: 5}, pos=-1, ngen=0),
        sib("budget: one token left", 1, 6, {0: 8, 3: 9}, ngen=MAX_NEW - 1),
        sib("budget: two left, the walk is cut", 1, 6, {0: 8, 3: 9, 4: 7}, ngen=MAX_NEW - 2),
        sib("budget: Dmax 0", 0, 1, {0: 5}, ngen=MAX_NEW - 2),
        sib("budget: Dmax 1", 0, 1, {0: 5}, ngen=MAX_NEW - 3),
        sib("sequence: fills", 1, 6, {0: 8, 3: 9}, pos=S_K - 2),
        sib("sequence: Dmax 0", 0, 1, {0: 5}, pos=S_K - 3),
        sib("sequence: Dmax 1", 0, 1, {0: 5}, pos=S_K - 4),
        sib("sequence: the walk stops at the end", 1, 6, {0: 8, 3: 9, 4: 7}, pos=S_K - 3),
        case("relative depth cut at 31", "chain40", 0, 1, {0: 100}),
        case("chain: 32 commits, the cap of the walk", "chain40", 1, 40, {j: 101 + j for j in range(40)}),
        case("tile edge: row 32 at depth 31", "edge31", 0, 1, {0: 100}),
        case("tile edge: row 32 at depth 1", "edge1", 0, 1, {0: 400}),
        case("walk to local row 32", "edge31", 1, 33, {**{j: 101 + j for j in range(30)}, 30: 201, 32: EOS}),
        case("walk to local row 31", "edge31", 1, 33, {**{j: 101 + j for j in range(30)}, 30: 200, 31: EOS}),
        case("fan: the last child, beyond a short pass", "edge1", 1, 41, {0: 339, 40: EOS}),
        case("a member that is a prefix of another", "prefix", 1, 4, {0: 6, 1: 7, 2: 8, 3: EOS}),
    ]
    out += [case(f"broken {k}", f"broken {k}", 1, 6, {0: 8, 3: 9, 4: EOS}) for k in ("end", "parent", "token", "depth", "n_plan")]
    out += [case(f"broken {k} from the root", f"broken {k}", 0, 8, {0: 5, 1: 6, 2: 7}) for k in ("end", "parent", "token", "depth")]
    return out


def plan1_of(c, V):
    return broken(c["plan"][7:]) if c["plan"].startswith("broken") else sample_plan(plan_of(PLANS[c["plan"]], V=V), 0)


def logits_of(c, R_in, V, rng, scale):
    lg = (scale * rng.standard_normal((R_in, V))).astype(np.float32)
    for j, tkn in c["peaks"].items():
        if j < R_in:
            lg[j, tkn] = lg[j].max() + np.float32(3)
    for j, t0, t1 in c["ties"]:
        lg[j, t0] = lg[j, t1] = np.float32(lg[j].max() + 1)
    return lg


def guarded(n, dtype, fill):
    big = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=DEV)
    return big, big[GUARD:GUARD + n]


def run_cases(cs, R_in, R_out, V, emb, *, stop=True, shared=None, counter=None, sync=True, seed=0):
    """One launch on B = len(cs) row cases, a plan per sequence (or `shared`: one plan for all) -> (rows with their logits and
    plans, dict of tensors: the in/out operands after the step and every output, the guarded buffers under "_guards")."""
    B = len(cs)
    rng = np.random.default_rng(seed + 7 * R_in + V)
    rows = [dict(c, logits=logits_of(c, R_in, V, rng, 3.0 if V < 1000 else 6.0), plan1=plan1_of(c, V) if shared is None else shared,
                 ids=rng.integers(3, 400, S_K).astype(np.int64)) for c in cs]
    t = lambda a, dt: torch.as_tensor(np.asarray(a), dtype=dt, device=DEV).contiguous()   # noqa: E731
    if shared is None:
        P = max(len(r["plan1"][1]) for r in rows)
        tab = lambda i, fill: t(np.stack([np.concatenate([r["plan1"][i], np.full(P - len(r["plan1"][i]), fill)])   # noqa: E731
                                          for r in rows]), torch.int32)
        plan = dict(n_plan=t([min(r["plan1"][0], 2 ** 31 - 1) for r in rows], torch.int32), token=tab(1, 0), depth=tab(2, 0),
                    end=tab(3, 0), parent=tab(4, -1))
        for r in rows:                                             # (the restatement sees the padded table, as the kernel does)
            r["plan1"] = (r["plan1"][0],) + tuple(np.concatenate([a, np.full(P - len(a), f)])
                                                 for a, f in zip(r["plan1"][1:], (0, 0, 0, -1)))
    else:
        plan = dict(n_plan=t([shared[0]], torch.int32), **{k: t(shared[i], torch.int32)
                                                          for i, k in ((1, "token"), (2, "depth"), (3, "end"), (4, "parent"))})
    tiles = (R_out + TILE - 1) // TILE
    guards, st = {}, {}
    for k, n, dt, fill in (("start", B, torch.int32, -7), ("depth", B * R_out, torch.int32, -7), ("end", B * R_out, torch.int32, -7),
                           ("tile_anc", B * tiles * TILE, torch.int32, -7), ("path", B * WALK, torch.int32, -7),
                           ("n_path", B, torch.int32, -7), ("start_old", B, torch.int32, -7), ("token", B * WALK, torch.int32, -7),
                           ("logprob", B * WALK, torch.float32, float("nan")), ("n_committed", B, torch.int32, -7),
                           ("n_drafted", B, torch.int32, -7), ("n_active", 1, torch.int32, -7), ("n_on_trie", 1, torch.int32, -7),
                           ("x", B * R_out * D_K, emb.dtype, float("nan")), ("pos64", B, torch.int64, -7)):
        guards[k], st[k] = guarded(n, dt, fill)
    st["x"] = st["x"].view(B * R_out, D_K)
    st.update(logits=t(np.stack([r["logits"] for r in rows]).reshape(B * R_in, V), torch.float32),
              ids=t(np.stack([r["ids"] for r in rows]), torch.int64), pos=t([r["pos"] for r in rows], torch.int32),
              done=t([r["done"] for r in rows], torch.int32), ngen=t([r["ngen"] for r in rows], torch.int32),
              node=t([r["node"] for r in rows], torch.int32), len=t([r["m"] for r in rows], torch.int32),
              counter=torch.zeros(2, dtype=torch.int32, device=DEV) if counter is None else counter)
    ops.tree_spec_step(st["logits"], emb, plan, st["ids"], st["pos"], st["done"], st["ngen"], st["node"], st["len"], st["start"],
                       st["x"], st["depth"], st["end"], st["tile_anc"], st["path"], st["n_path"], st["start_old"], st["token"],
                       st["logprob"], st["n_committed"], st["n_drafted"], st["n_active"], st["n_on_trie"], st["counter"],
                       max_new_tokens=MAX_NEW, pos64=st["pos64"], eos_id=EOS, stop_at_eos=stop)
    st["_guards"] = guards
    if sync:
        torch.cuda.synchronize()
    return rows, st


def check_cases(rows, st, R_in, R_out, V, emb, stop=True):
    """Every row of a launch against the restatement, every output; the words around every output untouched."""
    got = {k: v.cpu() for k, v in st.items() if k not in ("logits", "_guards")}
    for k, big in st["_guards"].items():
        big = big.cpu()
        n = big.numel() - 2 * GUARD
        for edge in (big[:GUARD], big[GUARD + n:]):
            assert bool(torch.isnan(edge).all()) if edge.is_floating_point() else bool((edge == -7).all()), ("guard", k)
    emb_h = emb.cpu()
    B, tiles = len(rows), (R_out + TILE - 1) // TILE
    running = on_trie = 0
    worst = 0.0
    for b, r in enumerate(rows):
        want = tree_step_ref(r["logits"], r["plan1"], r["ids"], r["pos"], r["done"], r["ngen"], r["node"], r["m"], R_in=R_in,
                             R_out=R_out, eos_id=EOS, stop_at_eos=stop, max_new_tokens=MAX_NEW)
        what = (r["name"], R_in, R_out, V, stop)
        nc = want["n_committed"]
        assert got["token"].view(B, WALK)[b].tolist() == want["tokens"] + [-1] * (WALK - nc), what
        assert got["path"].view(B, WALK)[b].tolist() == want["path"] + [0] * (WALK - nc), what
        assert int(got["n_committed"][b]) == nc == int(got["n_path"][b]) and int(got["n_drafted"][b]) == want["n_drafted"], what
        assert np.array_equal(got["ids"][b].numpy(), want["ids"]), what
        assert int(got["pos"][b]) == want["pos"] and int(got["ngen"][b]) == want["n_generated"], what
        assert int(got["done"][b]) == want["done"] and int(got["node"][b]) == want["node"], (what, int(got["node"][b]), want["node"])
        assert int(got["start"][b]) == want["start"] == int(got["pos64"][b]) and int(got["start_old"][b]) == want["start_old"], what
        assert int(got["len"][b]) == want["len"], (what, int(got["len"][b]), want["len"])
        assert got["depth"].view(B, R_out)[b].tolist() == want["depth"], what
        assert got["end"].view(B, R_out)[b].tolist() == want["end"], what
        assert got["tile_anc"].view(B, tiles, TILE)[b].tolist() == want["tile_anc"], what
        if not want["live"]:                                       # a row that committed nothing keeps its state
            assert np.array_equal(got["ids"][b].numpy(), r["ids"]) and int(got["node"][b]) == r["node"], what
        if r["plan"].startswith("broken"):                         # wrong drafts still give greedy's tokens, inside the arrays
            assert want["tokens"][0] == int(np.argmax(r["logits"][0])), what
            assert all(0 <= d <= 31 for d in want["depth"]) and all(j < e <= max(want["len"], j + 1) for j, e in enumerate(want["end"]))
        x = got["x"][b * R_out:(b + 1) * R_out]
        for j in range(R_out):
            ref = emb_h[want["x_tokens"][j]] if j < len(want["x_tokens"]) else torch.zeros_like(emb_h[0])
            assert torch.equal(BITS(x[j]), BITS(ref)), (what, j)
        lg32 = torch.from_numpy(r["logits"])
        dev32 = float((torch.log_softmax(lg32, -1).double() - torch.log_softmax(lg32.double(), -1)).abs().max())
        bound = max(4.0 * dev32, 1e-6)       # 4 x what torch's own fp32 log_softmax deviates from fp64 on these rows (floor 1e-6)
        lp = got["logprob"].view(B, WALK)[b]
        for i in range(WALK):
            if i < nc:
                worst = max(worst, abs(float(lp[i]) - want["logprobs"][i]))
                assert abs(float(lp[i]) - want["logprobs"][i]) <= bound, (what, i)
            else:
                assert float(lp[i]) == 0.0, (what, i)
        running += want["running"]
        on_trie += want["on_trie"]
    assert int(got["n_active"]) == running and int(got["n_on_trie"]) == on_trie, (int(got["n_active"]), running, on_trie)
    assert got["counter"].tolist() == [0, 0]
    return worst


def make_emb(V, dtype):
    return torch.randn(V, D_K, generator=torch.Generator().manual_seed(1)).to(dtype).to(DEV)


def ref_of(c, R, V=509, stop=True, seed=0):
    """The restatement's row for one case, as run_cases would draw it alone (the device is not needed)."""
    rng = np.random.default_rng(99)
    return tree_step_ref(logits_of(c, R, V, rng, 3.0), plan1_of(c, V), rng.integers(3, 400, S_K), c["pos"], c["done"], c["ngen"],
                         c["node"], c["m"], R_in=R, R_out=R, stop_at_eos=stop, max_new_tokens=MAX_NEW)


def test_the_cases_are_what_they_say():
    by = lambda R: {c["name"]: c for c in cases_for(R)}            # noqa: E731
    r = ref_of(by(64)["whole member to its EOS (the middle sibling)"], 64)
    assert r["tokens"] == [8, 9, EOS] and r["path"] == [0, 3, 4] and r["done"] == 1
    assert ref_of(by(64)["whole member to its EOS (the middle sibling)"], 64, stop=False)["done"] == 0
    for R, nxt in ((2, 4), (3, 4)):                                # the child lies beyond the pass: the next root
        r = ref_of(by(R)["whole member to its EOS (the middle sibling)"], R)
        assert r["tokens"] == [8] and r["node"] == nxt and r["len"] == 2
    assert ref_of(by(64)["leaves at the root"], 64)["node"] == -1 and ref_of(by(64)["leaves at depth 2"], 64)["tokens"] == [6, 30]
    r = ref_of(by(64)["relative depth cut at 31"], 64)
    assert r["len"] == 32 and r["depth"][:32] == list(range(32)) and r["tile_anc"][1] == [-1] * 32
    r = ref_of(by(64)["chain: 32 commits, the cap of the walk"], 64)
    assert r["n_committed"] == 32 and r["node"] == 33 and r["len"] == 7           # the budget leaves relative depths 0 .. 6
    for R in (33, 64):
        r = ref_of(by(R)["tile edge: row 32 at depth 31"], R)
        assert r["len"] == 33 and r["depth"][31:33] == [31, 31] and r["tile_anc"][1] == list(range(31)) + [-1]
        r = ref_of(by(R)["tile edge: row 32 at depth 1"], R)
        assert r["len"] == min(R, 41) and r["depth"][32] == 1 and r["tile_anc"][1] == [0] + [-1] * 31
        assert ref_of(by(R)["walk to local row 32"], R)["path"] == list(range(31)) + [32]
    assert ref_of(by(33)["fan: the last child, beyond a short pass"], 33)["node"] == 41
    assert ref_of(by(64)["fan: the last child, beyond a short pass"], 64)["tokens"] == [339, EOS]
    assert ref_of(by(64)["budget: Dmax 0"], 64)["len"] == 1 and ref_of(by(64)["budget: Dmax 1"], 64)["len"] == 2
    assert ref_of(by(64)["sequence: Dmax 0"], 64)["len"] == 1 and ref_of(by(64)["sequence: Dmax 1"], 64)["len"] == 2
    r = ref_of(by(64)["sequence: fills"], 64)
    assert r["len"] == 0 and r["done"] == 0 and r["n_committed"] == 1
    assert ref_of(by(64)["budget: two left, the walk is cut"], 64)["tokens"] == [8, 9]
    assert ref_of(by(64)["tie on the trie: the lower index is a child"], 64)["tokens"][:2] == [6, 7]
    assert ref_of(by(64)["tie on the trie: the lower index is no child"], 64)["node"] == -1
    for k in ("done row", "budget spent", "no room"):
        assert not ref_of(by(64)[k], 64)["live"]
    assert ref_of(by(64)["a member that is a prefix of another"], 64)["tokens"] == [6, 7, 8, EOS]


CASES_K = [(R, V, torch.float32) for R in (2, 3, 33, 64) for V in (509, 32000)] + \
          [(R, 509, dt) for R in (3, 64) for dt in (torch.bfloat16, torch.float16)]


@pytest.mark.parametrize("R,V,dtype", CASES_K)
def test_tree_spec_step_follows_the_rule(R, V, dtype):
    cs, emb = cases_for(R), make_emb(V, dtype)
    worst = 0.0
    for stop in (True, False):
        rows, st = run_cases(cs, R, R, V, emb, stop=stop)
        worst = max(worst, check_cases(rows, st, R, R, V, emb, stop))
    print(f"R={R} V={V} {dtype}: {len(cs)} row cases, stop_at_eos on and off, largest log-probability error {worst:.3e}")


@pytest.mark.parametrize("R_in,R_out", [(1, 64), (64, 1), (1, 2), (33, 64)])
def test_the_pass_before_and_the_pass_behind_may_differ_in_width(R_in, R_out):
    """The first step reads the prefill's row and feeds R rows; the step after the last row left its trie feeds one."""
    cs, emb = cases_for(R_in), make_emb(509, torch.float32)
    rows, st = run_cases(cs, R_in, R_out, 509, emb)
    check_cases(rows, st, R_in, R_out, 509, emb)


def test_a_shared_plan_is_read_with_stride_zero():
    shared = sample_plan(plan_of(PLANS["sib"], V=509), 0)
    cs = [c for c in cases_for(8) if c["plan"] == "sib"]
    emb = make_emb(509, torch.float32)
    rows, st = run_cases(cs, 8, 8, 509, emb, shared=shared)
    check_cases(rows, st, 8, 8, 509, emb)


def test_two_launches_back_to_back_on_one_counter():
    cs, emb = cases_for(33), make_emb(32000, torch.float32)
    counter = torch.zeros(2, dtype=torch.int32, device=DEV)
    rows, a = run_cases(cs, 33, 33, 32000, emb, counter=counter, sync=False)       # queued with nothing between them
    _, b = run_cases(cs, 33, 33, 32000, emb, counter=counter, sync=False)
    torch.cuda.synchronize()
    assert counter.tolist() == [0, 0]
    for k in a:
        if k not in ("_guards", "logits"):
            assert torch.equal(BITS(a[k]), BITS(b[k])), k
    check_cases(rows, a, 33, 33, 32000, emb)


DONE0 = [0, 0, 0, 1, 0]
POS0 = [3, S_K - 2, S_K - 1, 6, -1]                 # row 1 fills the sequence, row 2 has no room, row 4 starts at position 0


@pytest.mark.parametrize("node0", [0, -1])
@pytest.mark.parametrize("V,dtype", [(509, torch.float32), (32000, torch.float32), (509, torch.bfloat16), (509, torch.float16)])
def test_one_row_per_pass_is_decode_next_bit_for_bit(V, dtype, node0):
    B = 5
    rng = np.random.default_rng(V)
    lg = ((3.0 if V < 1000 else 6.0) * rng.standard_normal((B, V))).astype(np.float32)
    lg[1, EOS] = lg[1].max() + 3                                   # an EOS, written into the last position
    lg[4, 9] = lg[4, 200] = np.float32(lg[4].max() + 1)            # an exact tie
    lg[0, 5] = lg[0].max() + 3                                     # on the trie, where there is one
    ids0 = rng.integers(3, 400, (B, S_K)).astype(np.int64)
    ids0[3, 6] = V + 11                                            # a done row on an id outside the vocabulary: clamped alike
    emb = make_emb(V, dtype)
    t = lambda a, dt: torch.as_tensor(np.asarray(a), dtype=dt, device=DEV).contiguous()   # noqa: E731
    i32 = lambda *s: torch.full(s, -7, dtype=torch.int32, device=DEV)                      # noqa: E731
    n, tok, dep, end, par = sample_plan(plan_of(PLANS["sib"], V=V), 0)
    plan = dict(n_plan=t([n], torch.int32), token=t(tok, torch.int32), depth=t(dep, torch.int32), end=t(end, torch.int32),
                parent=t(par, torch.int32))
    for stop in (True, False):
        mk = lambda: dict(ids=t(ids0, torch.int64), pos=t(POS0, torch.int32), done=t(DONE0, torch.int32),   # noqa: E731
                          x=torch.full((B, D_K), float("nan"), dtype=dtype, device=DEV), token=i32(B), n_active=i32(1),
                          pos64=torch.full((B,), -7, dtype=torch.int64, device=DEV))
        a, b = mk(), mk()
        ops.decode_next(t(lg, torch.float32), emb, a["ids"], a["pos"], a["done"], a["x"], a["token"], i32(B), a["n_active"],
                        pos64=a["pos64"], temperature=0.0, eos_id=EOS, stop_at_eos=stop)
        counter = torch.zeros(2, dtype=torch.int32, device=DEV)
        token = i32(B, WALK)
        ops.tree_spec_step(t(lg, torch.float32), emb, plan, b["ids"], b["pos"], b["done"], torch.zeros(B, dtype=torch.int32, device=DEV),
                           t([node0] * B, torch.int32), torch.ones(B, dtype=torch.int32, device=DEV), i32(B), b["x"], i32(B),
                           i32(B), i32(TILE * B), i32(B, WALK), i32(B), i32(B), token, torch.empty(B, WALK, device=DEV), i32(B),
                           i32(B), b["n_active"], i32(1), counter, max_new_tokens=MAX_NEW, pos64=b["pos64"], eos_id=EOS,
                           stop_at_eos=stop)
        torch.cuda.synchronize()
        b["token"] = token[:, 0].contiguous()
        for k in a:
            assert torch.equal(BITS(a[k]), BITS(b[k])), (k, stop, a[k], b[k])
        assert a["token"].tolist()[2:4] == [-1, -1] and int(a["token"][4]) == 9 and counter.tolist() == [0, 0]
        assert bool((token[:, 1:] == -1).all())


def test_the_wrapper_refuses_bad_operands():
    cs, emb = cases_for(4)[:5], make_emb(509, torch.float32)
    with pytest.raises(ValueError):
        run_cases(cs, 65, 4, 509, emb)
    with pytest.raises(ValueError):
        run_cases(cs, 4, 65, 509, emb)
    with pytest.raises(ValueError):
        run_cases(cs, 4, 4, 509, make_emb(510, torch.float32))
    with pytest.raises(ValueError):
        run_cases(cs, 4, 4, 509, emb, counter=torch.zeros(1, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError):
        run_cases(cs, 4, 4, 509, emb.to(torch.bfloat16).float().cpu())


# ------------------------------------------------------------------------------------------------ the accepted path joins the cache
N_A, S_A, H_A, DH_A, A_A, F_A, L_A = 3, 32, 2, 128, 10, 10, 2
DT_ROT = [(torch.float32, True), (torch.bfloat16, True), (torch.bfloat16, False), (torch.float16, True), (torch.float16, False)]


def commit_setup(dtype, R, seed):
    D = H_A * DH_A
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: (1.5 * torch.randn(*s, generator=g)).to(dtype).to(DEV)      # noqa: E731
    before = rnd(L_A, N_A * S_A + A_A, 3 * D)                      # sentinels everywhere: whatever is written that should not be, shows
    rows = rnd(L_A, N_A * R, 3 * D)
    g1, g2 = torch.randn(H_A, generator=g).to(DEV), torch.randn(H_A, generator=g).to(DEV)
    ang = torch.arange(S_A).float()[:, None] * (10000.0 ** (-torch.arange(0, DH_A, 2).float() / DH_A))[None]
    rope = (ang.cos().contiguous().to(DEV), ang.sin().contiguous().to(DEV))
    return D, before, rows, g1, g2, rope


def appended(before, rows, picks, start, dtype, rotated, g1, g2, rope):
    """What fvqa_attn_suffix_append stores, layer by layer, when the raw rows picks[n] of sequence n are fed as ONE chain from
    start[n]: the yardstick (it writes the fed rows' k | v and nothing else: tests/test_lookahead_gpu.py)."""
    D, T = H_A * DH_A, max(1, max(len(p) for p in picks))
    R = rows.shape[1] // N_A
    want = before.clone()
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)               # noqa: E731
    for l in range(L_A):
        suf = torch.zeros(N_A * T, 3 * D, dtype=dtype, device=DEV)
        for n, p in enumerate(picks):
            for i, j in enumerate(p):
                suf[n * T + i] = rows[l, n * R + j]
        o = torch.empty(N_A * T, D, dtype=dtype, device=DEV)
        ops.attn_suffix_append(suf, want[l], o, g1, g2, i32([1, 3, 20]), i32(start), i32([len(p) for p in picks]), rope, N_A, T,
                               S_A, H_A, DH_A, A_A, F_A, cache_rotated=rotated)
    return want


def committed(before, rows, path, n_path, start, rotated, rope):
    cache = before.clone()
    p = torch.zeros(N_A, WALK, dtype=torch.int32)
    for n, row in enumerate(path):
        p[n, :len(row)] = torch.tensor(row, dtype=torch.int32)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)               # noqa: E731
    ops.kv_tree_commit(cache, rows, p.to(DEV), i32(n_path), i32(start), rope, n_seq=N_A, S=S_A, H=H_A, Dh=DH_A, A=A_A,
                       cache_rotated=rotated)
    torch.cuda.synchronize()
    return cache


CHAINS = [([5, S_A - 4, S_A - 1], [4, 4, 1]),                       # start + n_path reaches S for two sequences
          ([7, S_A - 1, S_A - 4], [0, 1, 4]),                       # a sequence that commits nothing
          ([0, 0, 12], [4, 1, 3])]                                  # an empty cache


@pytest.mark.parametrize("dtype,rotated", DT_ROT)
@pytest.mark.parametrize("start,n_path", CHAINS)
def test_commit_on_a_chain_stores_what_append_stores(start, n_path, dtype, rotated):
    """Bit for bit, k rotated included: the commit kernel restates the append kernel's rotation with contraction off."""
    D, before, rows, g1, g2, rope = commit_setup(dtype, 4, len(str(dtype)) + 7 * start[0])
    picks = [list(range(k)) for k in n_path]
    want = appended(before, rows, picks, start, dtype, rotated, g1, g2, rope)
    got = committed(before, rows, picks, n_path, start, rotated, rope)
    assert torch.equal(BITS(got), BITS(want))
    assert int((BITS(got) != BITS(before)).any(2).sum()) == L_A * sum(n_path)     # every layer's rows, and they differ from the sentinel
    assert torch.equal(BITS(got[:, :, :D]), BITS(before[:, :, :D]))               # the q third


@pytest.mark.parametrize("dtype,rotated", DT_ROT)
def test_commit_on_a_branching_path(dtype, rotated):
    """Rows 0, 3, 7 of a 12-row pass land at start .. start + 2; every other word of the sentinel cache is untouched. The defect
    that stores row i instead of path[i] gives other bits."""
    D, before, rows, g1, g2, rope = commit_setup(dtype, 12, 5)
    start, picks = [6, S_A - 3, 11], [[0, 3, 7], [0, 3, 7], [0, 11]]
    want = appended(before, rows, picks, start, dtype, rotated, g1, g2, rope)
    got = committed(before, rows, picks, [3, 3, 2], start, rotated, rope)
    assert torch.equal(BITS(got), BITS(want))
    changed = (BITS(got) != BITS(before)).any(2)
    for l in range(L_A):
        at = sorted(int(r) for r in changed[l].nonzero().flatten())
        assert at == [n * S_A + start[n] + i for n in range(N_A) for i in range(len(picks[n]))]
    assert torch.equal(BITS(got[:, :, :D]), BITS(before[:, :, :D]))
    defect = appended(before, rows, [[0, 1, 2], [0, 1, 2], [0, 1]], start, dtype, rotated, g1, g2, rope)
    assert not torch.equal(BITS(defect), BITS(want)) and not torch.equal(BITS(defect), BITS(got))
    # entries that lead outside an operand append nothing: a path row >= rows, a position >= S, n_path beyond 32
    odd = committed(before, rows, [[0, 99, 7], [0, 3, 7], [-1, 11]], [3, 3, 2], [6, S_A - 2, 11], rotated, rope)
    want_odd = appended(before, rows, [[0], [0, 3], []], [6, S_A - 2, 11], dtype, rotated, g1, g2, rope)
    second = appended(before, rows, [[7], [], [11]], [8, 0, 12], dtype, rotated, g1, g2, rope)
    assert torch.equal(BITS(odd), torch.where(BITS(second) != BITS(before), BITS(second), BITS(want_odd)))
    with pytest.raises(ValueError):
        ops.kv_tree_commit(before, before, torch.zeros(N_A, WALK, dtype=torch.int32, device=DEV),
                           torch.zeros(N_A, dtype=torch.int32, device=DEV), torch.zeros(N_A, dtype=torch.int32, device=DEV), rope,
                           n_seq=N_A, S=S_A, H=H_A, Dh=DH_A, A=A_A, cache_rotated=rotated)


# ------------------------------------------------------------------------------------------------ end to end
def answers_of(plain):
    """The plain call's generated tokens per row, without the EOS: what a draft set is built around."""
    tk, out = trimmed(plain["tokens"]).cpu().tolist(), []
    for row in tk:
        row = [t for t in row if t >= 0]
        out.append(row[:row.index(EOS)] if EOS in row else row)
    return out


def decoys(ans, k, V=32000):
    """Four answers that are not `ans`: sharing 0, 1 and k leading tokens with it, and one of another length. (An empty `ans` —
    the model's first token is the EOS — has decoys that share nothing.)"""
    o = lambda i, d: ((ans[min(i, len(ans) - 1)] if ans else 40 + i) + d) % (V - 3) + 3   # noqa: E731  (never ans[i], never the EOS)
    return [[o(0, 7), o(0, 8), 11], ans[:1] + [o(1, 5), 12, 13], ans[:k] + [o(k, 9), o(k, 10)], ans[:1] + [o(1, 6)]]


def same_answer(out, plain, what):
    for k in ("ids", "n_generated"):
        assert torch.equal(out[k], plain[k]), (what, k)
    assert torch.equal(out["tokens"], trimmed(plain["tokens"])), what
    B = out["ids"].shape[0]
    assert out["tokens"].dtype == out["n_committed"].dtype == out["n_drafted"].dtype == out["rows_per_pass"].dtype == torch.int32
    assert tuple(out["n_committed"].shape) == tuple(out["n_drafted"].shape) == (B, out["steps"])
    assert tuple(out["rows_per_pass"].shape) == (out["steps"],)
    assert torch.equal(out["n_committed"].sum(1).to(torch.int64), out["n_generated"]), what


def assert_passes(out, plain, batch, sets, what, *, R, max_new, stop):
    """n_committed is the host model's; rows_per_pass falls to 1 within two steps of the last row leaving its trie and stays."""
    tk = plain["tokens"].cpu().tolist()
    B = len(tk)
    plan = plan_of(sets, B=B)
    left = 0
    for b, p in enumerate(batch["prefix_index"]["vqa"]):
        trace = []
        want = predict_passes(tk[b], sample_plan(plan, b), p, R=R, max_new=max_new, S=128, stop=stop, trace=trace)
        got = out["n_committed"][b].tolist()
        assert got == want + [0] * (len(got) - len(want)), (what, b, got, want)
        left = max(left, trace.index(False) if False in trace else len(trace))
    w = out["rows_per_pass"].tolist()
    assert w[0] == 1 and all(x in (1, R) for x in w), (what, w)
    assert all(x == 1 for x in w[left + 3:]), (what, w, left)      # the count of step `left` is read at step left + 2
    if 1 in w[1:]:
        assert all(x == 1 for x in w[1 + w[1:].index(1):]), (what, w)              # ... and stays there
    return w


E2E = [(R, stop, max_new) for R in (2, 4, 33, 64) for stop, max_new in ((True, 31), (False, 31))] + [(4, False, 12)]


@pytest.mark.parametrize("R,stop,max_new", E2E)
def test_the_answer_among_four_decoys(tiny, R, stop, max_new):  # noqa: F811
    """Per-sample sets: each sample's greedy answer and four decoys. B * R reaches 66 and 128 rows (beyond the few-rows
    projections' 64) at R = 33 and 64."""
    eng, batch = tiny.eng, tiny.batch
    plain = generate.generate(eng, batch, temperature=0.0, stop_at_eos=True, max_new_tokens=31)
    sets = [[a] + decoys(a, max(2, len(a) // 2)) for a in answers_of(plain)]
    if not stop or max_new != 31:
        plain = generate.generate(eng, batch, temperature=0.0, stop_at_eos=stop, max_new_tokens=max_new)
    out = generate.generate(eng, batch, temperature=0.0, stop_at_eos=stop, max_new_tokens=max_new, lookahead=R, draft_answers=sets)
    assert set(out) == set(plain) | {"n_committed", "n_drafted", "rows_per_pass"}
    same_answer(out, plain, f"answer in the set R={R}")
    w = assert_passes(out, plain, batch, sets, f"answer in the set R={R}", R=R, max_new=max_new, stop=stop)
    print(f"R={R} stop={stop} max_new={max_new}: plain {plain['steps']} steps for {plain['n_generated'].tolist()} tokens; tree "
          f"draft {out['steps']} steps, committed {out['n_committed'].tolist()}, rows per pass {w}")
    if stop and R >= 33:
        assert out["steps"] <= 4 and 2 * out["steps"] <= plain["steps"]   # the prefill's token, the whole answer, the lagging stop
    assert int(out["n_drafted"].max()) <= R - 1 and out["n_drafted"][:, 0].tolist() == [0] * len(sets)


@pytest.mark.parametrize("R", [4, 64])
def test_sets_without_the_answer_and_a_prefix_of_it(tiny, R):  # noqa: F811
    eng, batch = tiny.eng, tiny.batch
    plain = generate.generate(eng, batch, temperature=0.0, stop_at_eos=True, max_new_tokens=31)
    ans = answers_of(plain)
    k = max(2, len(ans[0]) // 2)
    for what, sets in (("none of it", decoys(ans[0], k)[:1] + [[9, 9, 9]]),                # a shared set nobody's answer starts in
                       ("decoys only, per sample", [decoys(a, max(2, len(a) // 2)) for a in ans]),
                       ("a proper prefix of the answer", [[a[:max(2, len(a) // 2)]] + decoys(a, 2)[:1] for a in ans]),
                       ("shared: every sample's answer", [a for a in ans] + decoys(ans[0], k))):
        out = generate.generate(eng, batch, temperature=0.0, stop_at_eos=True, max_new_tokens=31, lookahead=R, draft_answers=sets)
        same_answer(out, plain, what)
        w = assert_passes(out, plain, batch, sets, what, R=R, max_new=31, stop=True)
        print(f"R={R} {what}: {out['steps']} steps (plain {plain['steps']}), committed {out['n_committed'].tolist()}, rows per pass {w}")
        if what == "none of it":
            assert w[:4] == [1, R, R, 1] and set(w[3:]) == {1}     # one wasted wide pass and the lag, then one row per sample
            assert int(out["n_committed"].max()) == 1


def test_logprobs_are_the_dense_forwards(tiny):  # noqa: F811
    eng, batch = tiny.eng, tiny.batch
    plain = generate.generate(eng, batch, temperature=0.0, stop_at_eos=True, return_logprobs=True)
    sets = [[a] + decoys(a, max(2, len(a) // 2)) for a in answers_of(plain)]
    # the tree attention reduces in another order than the one-row kernel: what that costs EXISTING code on this fixture
    el = [vocab.score_vocab(eng, batch, sets, route=r)["edge_logprob"].double() for r in ("tree", "dense")]
    routes = float((el[0] - el[1]).abs().max())
    tol = max(tiny.tol, 4.0 * routes)
    print(f"score_vocab tree route against dense on this fixture: largest per-edge difference {routes:.3e} -> tolerance {tol:.3e}")
    worst = 0.0
    for R in (4, 64):
        out = generate.generate(eng, batch, temperature=0.0, stop_at_eos=True, return_logprobs=True, lookahead=R, draft_answers=sets)
        same_answer({k: v for k, v in out.items() if k not in ("logprobs", "sum_logprob")}, plain, "logprobs")
        assert tuple(out["logprobs"].shape) == tuple(out["tokens"].shape) and out["logprobs"].dtype == torch.float32
        assert bool((out["logprobs"][out["tokens"] < 0] == 0).all()) and bool((out["logprobs"][out["tokens"] >= 0] < 0).all())
        assert torch.allclose(out["sum_logprob"], out["logprobs"].sum(1), rtol=0, atol=1e-6)
        lp = dense_logits(eng, batch, out["ids"]).double().log_softmax(-1)
        for b, p in enumerate(tiny.prefix):
            for t in range(int(out["n_generated"][b])):
                d = abs(float(lp[b, p - 1 + t, int(out["ids"][b, p + t])]) - float(out["logprobs"][b, t]))
                worst = max(worst, d)
                assert d <= tol, (R, b, t, d, tol)
    print(f"largest difference of a log-probability to the dense forward {worst:.3e}")


@pytest.mark.parametrize("pname,dtype", [("tiny_peakedperm", torch.bfloat16), ("tiny_peakedperm", torch.float16),
                                         ("7b_l2_peakedperm", torch.bfloat16)])
def test_sixteen_bit_builds(pname, dtype):
    eng = model_of(pname, dtype).ensure_engine()
    batch = eos_batch(pname)
    plain = generate.generate(eng, batch, temperature=0.0, stop_at_eos=True)
    sets = [[a] + decoys(a, max(2, len(a) // 2)) for a in answers_of(plain)]
    for R in (4, 33):
        out = generate.generate(eng, batch, temperature=0.0, stop_at_eos=True, lookahead=R, draft_answers=sets)
        dense_argmax_check(eng, batch, out, f"{pname} {dtype} R={R}")
        assert out["rows_per_pass"].tolist()[0] == 1 and out["steps"] <= plain["steps"]


def test_the_surface(tiny):  # noqa: F811
    m = model_of("tiny_peakedperm", torch.float32)
    plain = generate.generate(tiny.eng, tiny.batch, temperature=0.0, stop_at_eos=True)
    sets = [[a] + decoys(a, 2) for a in answers_of(plain)]
    want = m.generate(tiny.batch)
    assert m.generate(tiny.batch, lookahead=8, draft_answers=sets) == want
    assert "rows_per_pass" in m.last_generation and "n_committed" in m.last_generation


@pytest.mark.parametrize("stop_eos", [False, True])
def test_validation_with_gen_draft_keeps_its_answers(monkeypatch, stop_eos):
    """train.py --gen_draft options | vocab: `inference` returns what the plain protocol returns (with and without
    --gen_stop_eos) — the same ids, picks and extracted answers — in fewer token steps where the model answers with a drafted
    answer. The fixture's option texts are not what this model writes, so the sets are built around its own answers: per sample
    as 'options' has them, one shared list as 'vocab' has it."""
    from fvqa import constrain
    m = model_of("tiny_peakedperm", torch.float32)
    batch = eos_batch("tiny_peakedperm")
    eng = m.ensure_engine()
    own = m._answer_sets(batch, "options", eng)                    # the batch's own options: what the flag drafts
    assert len(own) == 4 and constrain.TokenTrie.from_sequences([[o for o in s_ if o] for s_ in own], EOS, eng.V).n_nodes > 4
    m.args.gen_stop_eos = stop_eos
    best0, ext0 = m(batch, inference=True)
    ids0 = m.last_generation["ids"].clone()
    ans = answers_of(generate.generate(eng, batch, temperature=0.0, stop_at_eos=True))
    sets = {"options": [[a] + decoys(a, 2) for a in ans], "vocab": [a for a in ans if a] + decoys(ans[1], 2)}
    monkeypatch.setattr(m, "_answer_sets", lambda data, mode, eng_: sets[mode])
    for mode in ("options", "vocab"):
        m.args.gen_draft, m.args.lookahead = mode, 33
        try:
            best, ext = m(batch, inference=True)
        finally:
            del m.args.gen_draft, m.args.lookahead
            m.__dict__.pop("_draft_vocab_trie", None)              # (the module's shared model keeps nothing of this test)
        g = m.last_generation
        assert torch.equal(g["ids"], ids0) and torch.equal(best, best0) and ext == ext0, mode
        assert tuple(g["rows_per_pass"].shape) == (g["steps"],) and "n_committed" in g
        if stop_eos:
            assert g["steps"] <= 4, (mode, g["steps"])
    m.args.gen_stop_eos = False


def test_answer_cli_with_a_draft():
    """answer.py --draft options --lookahead R answers and prints the tokens committed per step."""
    r = subprocess.run([sys.executable, "answer.py", "--random_init", "--synthetic", "--question", "what is the man doing",
                        "--options", "a", "b", "c", "--max_new_tokens", "6", "--draft", "options", "--lookahead", "8"],
                       cwd=os.path.join(ROOT, "flipped-vqa_amd"), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    at = max(i for i, ln in enumerate(lines) if ln.startswith("["))
    head = re.fullmatch(r"\[(\d+) tokens, (\d+) steps, committed per step((?: \d+)+)\]", lines[at])
    assert head, lines[at]
    n, committed = int(head.group(1)), [int(x) for x in head.group(3).split()]
    toks = lines[at + 1].split() if at + 1 < len(lines) else []
    assert 1 <= n <= 6 and sum(committed) == n and len(committed) == int(head.group(2))
    assert len(toks) in (n, n - 1) and all(t.isdigit() for t in toks)           # (an EOS is counted, not printed)
