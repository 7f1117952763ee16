"""Answer-vocabulary scoring on the GPU: fvqa_attn_suffix_tree per row against fp64 (tests/vocab_util.py over
tests/cached_attn_util.py's one_row_ref and bounds), restated defects that must miss the bound, the chain case against
fvqa_attn_suffix, fvqa_trie_score against its fp64 restatement, and score_vocab's two routes against each other and against
generate(constraints=...)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from fvqa import ops, vocab  # noqa: E402
from tests import cached_attn_util as U  # noqa: E402
from tests import vocab_util as VU  # noqa: E402

DEV = "cuda"
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
MODES = [(d, r) for d in DTYPES for r in (False, True)]


def dev(x):
    return x.to(DEV).contiguous()


def run_tree(what, c, rot):
    """Two launches with equal bits; the live rows held to fp64 per row, the padding rows zeros, the cache untouched."""
    dtype, t = c["dtype"], c["plan"].tables(DEV)
    cache_d, suf_d = dev(c["cache"]), dev(c["suf"])
    outs = []
    for _ in range(2):
        o = torch.full((c["N"] * c["R"], c["D"]), U.NAN, dtype=dtype, device=DEV)
        ops.attn_suffix_tree(suf_d, cache_d, o, dev(c["g1"]), dev(c["g2"]), dev(c["vstart"]), dev(c["start"]), t["n_rows"],
                             t["depth"], t["end"], t["tile_anc"], (dev(c["cos"]), dev(c["sin"])), c["N"], c["R"], c["S"], c["H"],
                             U.DH, c["A"], c["F"], cache_rotated=rot)
        outs.append(o.cpu())
    got = outs[0]
    assert torch.equal(U.bits(outs[0]), U.bits(outs[1]))
    assert torch.equal(U.bits(cache_d.cpu()), U.bits(c["cache"]))
    assert not bool(got[~c["valid"]].float().any())
    live, want = got[c["valid"]], c["want"][c["valid"]]
    assert U.ref_floor(want) >= U.FLOOR, what
    assert bool(torch.isfinite(live.float()).all()), what
    fig = U.row_figures(live, want)
    print(f"{what}: worst row {float(fig.max()):.3e} (bound {U.BOUND[dtype]:.1e})")
    assert float(fig.max()) < U.BOUND[dtype], what
    return got


# ------------------------------------------------------------------------------------------------ 1. the kernel against fp64
ROW_SETS = [VU.chain_members(0), VU.random_members(31, 1), VU.random_members(32, 2), VU.random_members(33, 3),
            VU.random_members(65, 4, max_depth=12)]


@pytest.mark.parametrize("dtype,rot", MODES)
def test_tree_rows_per_sample_and_padding(dtype, rot):
    """1, 31, 32, 33 and 65 rows in one batch (R = 65: three tiles; every shorter sample has padding rows, NaN on the way in,
    zeros on the way out), frame windows in front of, across and behind start and absent."""
    c = VU.tree_case(dtype, rot, ROW_SETS, start=[40, 96, 33, 64, 100], vstart=[19, 90, -1, 60, 5], seed=11)
    assert c["R"] == 65 and list(c["plan"].n_rows) == [1, 31, 32, 33, 65]
    run_tree(f"tree rows 1..65 {dtype} rot={rot}", c, rot)


@pytest.mark.parametrize("dtype,rot", MODES)
def test_tree_chains_and_the_crossing(dtype, rot):
    """Chains of depth 0, 1, 30 and 31 (the deepest row a plan may hold: its chain fills the chunk), and the tree whose second
    tile starts inside a subtree that lies between a chain's head and its tail."""
    sets = [VU.chain_members(0), VU.chain_members(1), VU.chain_members(30), VU.chain_members(31), VU.crossing_members()]
    c = VU.tree_case(dtype, rot, sets, start=[50, 127, 64, 100, 70], vstart=[30, 120, 60, -1, 66], seed=13)
    assert list(c["plan"].n_rows) == [1, 2, 31, 32, 46] and int(c["plan"].depth.max()) == 31
    run_tree(f"tree chains {dtype} rot={rot}", c, rot)


@pytest.mark.parametrize("dtype,rot", MODES)
def test_tree_start_edges(dtype, rot):
    """One sample per start in START_EDGES (an empty cache, one key, prompts that end on and around a chunk of 32 keys), 33 rows."""
    n = len(U.START_EDGES)
    c = VU.tree_case(dtype, rot, [VU.random_members(33, 7, max_depth=6)] * n, start=U.START_EDGES,
                     vstart=[-1, 0, 19, 30, 25, -1, 60, 120], seed=17)
    run_tree(f"tree start edges {dtype} rot={rot}", c, rot)


@pytest.mark.parametrize("dtype,rot", [(torch.float32, True), (torch.bfloat16, False), (torch.float16, True)])
@pytest.mark.parametrize("A,F", U.AF_PAIRS)
def test_tree_adapter_and_window_lengths(A, F, dtype, rot):
    """(A, F) of AF_PAIRS; the window ends inside the tree's positions, straddles start, lies behind it, or is absent."""
    st = 30
    c = VU.tree_case(dtype, rot, [VU.random_members(33, 9, max_depth=14)] * 4, start=[st] * 4,
                     vstart=[st + 5 - F, st - F // 2, st + 2, -1], A=A, F=F, seed=19 + A + F)
    run_tree(f"tree A={A} F={F} {dtype} rot={rot}", c, rot)


# ------------------------------------------------------------------------------------------------ 2. defects miss the bound
PLANT = (4, 36, 3, 6, 37)          # the crossing tree: query 36 (X's second child, tile 1), key on ancestor 3 (tile 0: the chain),
                                   # decoys on its sibling 6 (in tile 1's chain, hidden by the interval test) and its child 37


@pytest.mark.parametrize("dtype,rot", MODES)
def test_tree_planted_keys_and_restated_defects(dtype, rot):
    sets = [VU.chain_members(0), VU.chain_members(1), VU.chain_members(30), VU.chain_members(31), VU.crossing_members()]
    c = VU.tree_case(dtype, rot, sets, start=[50, 127, 64, 100, 70], vstart=[30, 120, 60, -1, 66], seed=13, plant=PLANT)
    n, q, key_row, sib, desc = PLANT
    p = c["plan"]
    assert p.parent[n, sib] == p.parent[n, q] and p.parent[n, desc] == q and key_row < 32 <= q          # what PLANT claims
    assert sib in p.tile_anc[n, 1] and key_row in p.tile_anc[n, 1]
    o_ref, pt = VU.tree_row_ref(c, n, q)
    st = int(c["start"][n])
    assert float(pt[:, st + int(p.depth[n, key_row])].min()) >= 0.99                                     # the planted key decides
    got = run_tree(f"tree planted {dtype} rot={rot}", c, rot).view(c["N"], c["R"], -1)[n, q]
    for d in VU.DEFECTS:
        bad = VU.tree_row_ref(c, n, q, defect=d)[0]
        fig = float(U.row_figures(got[None], bad[None]).max())
        print(f"defect {d}: {fig:.3e}")
        assert fig > U.BOUND[dtype], d


# ------------------------------------------------------------------------------------------------ 3. the chain = fvqa_attn_suffix
@pytest.mark.parametrize("dtype,rot", MODES)
@pytest.mark.parametrize("T", [1, 7, 16])
def test_tree_chain_gives_the_suffix_kernels_rows(T, dtype, rot):
    c = VU.tree_case(dtype, rot, [VU.chain_members(T - 1)] * 2, start=[40, 120], vstart=[19, -1], seed=23 + T)
    assert c["R"] == T
    got = run_tree(f"tree chain T={T} {dtype} rot={rot}", c, rot)
    o = torch.full((2 * T, c["D"]), U.NAN, dtype=dtype, device=DEV)
    ops.attn_suffix(dev(c["suf"]), dev(c["cache"]), o, dev(c["g1"]), dev(c["g2"]), dev(c["vstart"]), dev(c["start"]),
                    torch.full((2,), T, dtype=torch.int32, device=DEV), (dev(c["cos"]), dev(c["sin"])), 2, 1, T, c["S"], c["H"],
                    U.DH, c["A"], c["F"], cache_rotated=rot)
    assert float(U.row_figures(got, o.cpu()).max()) < U.BOUND[dtype]


# ------------------------------------------------------------------------------------------------ 4. fvqa_trie_score
def score_inputs(seed, nan_row=False, ties=False):
    sets = [VU.random_members(40, seed, max_depth=10), VU.random_members(3, seed + 1), [[]], VU.random_members(300, seed + 2)]
    plan = vocab.plan_vocab(VU.trie_of(sets), len(sets), n_listed=[len(s) + 2 for s in sets])
    g = torch.Generator().manual_seed(seed)
    B, R, Vv = plan.B, plan.R, 64
    logits = torch.randn(B * R, Vv, generator=g) * 3
    if ties:
        logits = logits.round()                                         # small integers: equal sums and means happen
    if nan_row:
        logits[0 * R + 1] = float("nan")                                # every edge out of row 1 of sample 0
    tok = torch.as_tensor(plan.edge_token.astype(np.int64)) % Vv
    plan.edge_token[:] = tok.numpy()                                    # (tokens of the small test vocabulary)
    plan._dev.clear()
    lse = torch.logsumexp(logits.double(), -1)
    par = torch.as_tensor(plan.edge_parent.astype(np.int64)) + torch.arange(B)[:, None] * R
    lp64 = logits.double()[par, tok] - lse[par]
    return plan, logits, lse.float(), lp64.numpy(), Vv


@pytest.mark.parametrize("by_mean", [True, False])
@pytest.mark.parametrize("kind", ["plain", "ties", "nan"])
def test_trie_score_against_fp64(kind, by_mean):
    plan, logits, lse, lp64, Vv = score_inputs(31, nan_row=kind == "nan", ties=kind == "ties")
    B, R, top = plan.B, plan.R, 8
    t = plan.tables(DEV)
    outs = []
    for _ in range(2):
        edge_lp = torch.zeros(B, plan.E, dtype=torch.float32, device=DEV)
        out, blk = None, 50                                             # blocks of rows that cut through the samples
        for r0 in range(0, B * R, blk):
            n = min(blk, B * R - r0)
            out = ops.trie_score(t, edge_lp, B, R, Vv, logits=dev(logits[r0:r0 + n]), lse=dev(lse[r0:r0 + n]), row0=r0,
                                 n_block_rows=n, reduce=r0 + n >= B * R, n_columns=plan.M, top=top, by_mean=by_mean)
        out["edge_logprob"] = edge_lp
        outs.append({k: v.cpu() for k, v in out.items()})
    for k in outs[0]:
        assert torch.equal(U.bits(outs[0][k]), U.bits(outs[1][k])), k
    got = outs[0]
    # the edges in fp64 from the fp32 lse the kernel was handed; the members from the kernel's own fp32 edges
    ref = VU.score_ref(plan, got["edge_logprob"].double().numpy(), top, by_mean)
    live = torch.arange(plan.E)[None, :] < torch.as_tensor(plan.n_edges.astype(np.int64))[:, None]
    e_got, e_want = got["edge_logprob"].double()[live], torch.as_tensor(lp64)[live]
    ok = ~torch.isnan(e_want)
    assert torch.equal(torch.isnan(e_got), torch.isnan(e_want))
    assert float(((e_got - e_want)[ok].abs() / e_want[ok].abs().clamp_min(1.0)).max()) < 1e-5
    for k in ("logprob_sum", "log_posterior", "mean"):
        a, b = got[k].double().numpy(), ref[k]
        assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.isinf(a), np.isinf(b)), k
        fin = np.isfinite(b)
        # relative to the value; log_posterior = sum - logsumexp is a difference of fp32 numbers and may lie near 0 (a member
        # that takes the whole mass): relative to the larger of the value and the sum it was taken from
        scale = np.abs(b) if k != "log_posterior" else np.maximum(np.abs(b), np.abs(ref["logprob_sum"]))
        assert np.array_equal(a[fin & (scale == 0)], b[fin & (scale == 0)]), k
        fin &= scale > 0
        assert float((np.abs(a[fin] - b[fin]) / scale[fin]).max()) < 1e-5, k
    assert np.array_equal(got["count"].numpy(), ref["count"])
    for b in range(B):
        keys = ref["keys"][b]
        rk, rr = got["ranking"][b].tolist(), ref["ranking"][b].tolist()
        assert [x < 0 for x in rk] == [x < 0 for x in rr]
        for i, (x, y) in enumerate(zip(rk, rr)):
            if x < 0 or x == y:
                continue
            # a different member at rank i: only where the fp64 keys are closer than the bound allows to tell
            assert abs(keys[x] - keys[y]) <= 1e-5 * max(abs(keys[y]), 1.0), (b, i, x, y)
        assert int(got["prediction"][b]) == max(rk[0], 0)
    if kind == "nan":
        assert int(got["prediction"][0]) == ref["prediction"][0] and np.isnan(ref["keys"][0][ref["prediction"][0]])
    if kind == "ties":
        # integer logits are not enough for exact ties of sums of log-softmaxes: tie two members by hand through edge_lp
        edge_lp = torch.zeros(B, plan.E, dtype=torch.float32, device=DEV)
        edge_lp[:] = -1.0                                               # every member's mean is -1: the lowest column wins
        out = ops.trie_score(t, edge_lp, B, R, Vv, reduce=True, n_columns=plan.M, top=top, by_mean=True)
        for b in range(B):
            cols = sorted(int(c) for c in plan.member_index[b, :plan.n_members[b]])
            assert [x for x in out["ranking"][b].tolist() if x >= 0] == cols[:top]


# ------------------------------------------------------------------------------------------------ 5. end to end against the reference
def scale_err(got, want, mask):
    """max |got - want| over the masked entries of each sample, relative to the sample's largest |want|. A log-probability is a
    logit minus the row's logsumexp: its absolute error scales with the logits, not with the result, and the preferred member's
    mean is 0.004 at tiny width and exactly 0 at 7B width next to -17 / -64 for its rivals — no entry-wise relative figure exists."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    worst = 0.0
    for b in range(want.shape[0]):
        m = mask[b]
        worst = max(worst, float(np.abs(got[b][m] - want[b][m]).max() / np.abs(want[b][m]).max()))
    return worst


def bound_of(name, dtype):
    if dtype == torch.float32:
        return VU.FP32_RTOL
    assert VU.DENSE_MEAN_ERR[name][dtype] > 0, "measure the parent's dense pass first (tools/score_bench.py --vocab_errors)"
    return 4 * VU.DENSE_MEAN_ERR[name][dtype]


def engine_of(name, dtype):
    from tests.test_generate_gpu import model_of
    return model_of(VU.MODEL_OF[name], dtype).ensure_engine()


def test_the_parents_dense_error_is_what_the_constants_say():
    """DENSE_MEAN_ERR is measured, positive, and still what score_options(route="dense") — the parent's teacher-forced pass —
    gives on the members written out as options (printed; held within 1.5 x, the kernels are deterministic)."""
    from fvqa import score
    for name in VU.FIXTURES:
        g = VU.load(name)
        cols = VU.first_columns(g)
        for dtype in (torch.bfloat16, torch.float16):
            r = score.score_options(engine_of(name, dtype), VU.option_batch(g), route="dense")
            # (its sums over the members' known lengths: its own count leaves out a token whose loss is exactly 0)
            err = scale_err(-r["sum"].cpu().numpy() / np.maximum(g["count"], 1), g["mean"], cols)
            print(f"{name} {dtype}: the parent's dense pass, mean err {err:.4e} (constant {VU.DENSE_MEAN_ERR[name][dtype]:.3e})")
            assert 0 < VU.DENSE_MEAN_ERR[name][dtype] and err <= 1.5 * VU.DENSE_MEAN_ERR[name][dtype]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", VU.FIXTURES)
def test_both_routes_against_the_reference(name, dtype):
    """fp32: mean and sum within FP32_RTOL of the reference's training forward, equal counts; 16 bit: within 4 x the parent's dense
    error. The routes agree within twice the bound; predictions are the fixture's wherever its gap exceeds four times the bound —
    at least three samples, asserted."""
    g = VU.load(name)
    eng, batch, sets, cols = engine_of(name, dtype), VU.fixture_batch(g), VU.fixture_sets(g), VU.first_columns(g)
    bound = bound_of(name, dtype)
    decided = g["gap"] > 4 * bound
    assert int(decided.sum()) >= 3
    out = {}
    for route in vocab.ROUTES:
        r = vocab.score_vocab(eng, batch, sets, route=route, top=5)
        assert r["route"] == route and r["mean"].is_cuda
        out[route] = {k: r[k].cpu().numpy() for k in ("mean", "logprob_sum", "count", "prediction", "ranking", "log_posterior")}
        o = out[route]
        e_mean, e_sum = scale_err(o["mean"], g["mean"], cols), scale_err(o["logprob_sum"], g["logprob_sum"], cols)
        print(f"{name} {dtype} {route}: mean err {e_mean:.3e} sum err {e_sum:.3e} (bound {bound:.3e})")
        assert e_mean <= bound and e_sum <= bound
        assert np.array_equal(o["count"][cols], g["count"][cols]) and not o["count"][~cols].any()
        assert np.isneginf(o["mean"][~cols]).all() and np.isneginf(o["log_posterior"][~cols]).all()
        assert np.array_equal(o["prediction"][decided], g["prediction"][decided])
        assert np.array_equal(o["ranking"][:, 0], o["prediction"])
        post = np.where(cols, np.exp(o["log_posterior"].astype(np.float64)), 0.0).sum(1)
        assert np.allclose(post, 1.0, atol=1e-5)
    assert scale_err(out["tree"]["mean"], out["dense"]["mean"], cols) <= 2 * bound


# ------------------------------------------------------------------------------------------------ 6. routes and neighbours
@pytest.mark.parametrize("dtype", DTYPES)
def test_edges_are_the_constrained_decoders_logprobs(dtype):
    """Along the member the constrained greedy decoder picks, edge_logprob is that call's per-token log-probability."""
    from fvqa import generate
    name = "vocab_tiny"
    g = VU.load(name)
    eng, batch, sets = engine_of(name, dtype), VU.fixture_batch(g), VU.fixture_sets(g)
    r = vocab.score_vocab(eng, batch, sets)
    gen = generate.generate(eng, batch, temperature=0.0, constraints=sets, return_logprobs=True, max_new_tokens=32)
    plan, lp = r["plan"], r["edge_logprob"].cpu().numpy()
    bound = bound_of(name, dtype)
    for b in range(plan.B):
        c = int(gen["choice"][b])
        m = list(plan.member_index[b, :plan.n_members[b]]).index(c)
        n = int(plan.member_len[b, m])
        mine = lp[b, plan.member_path[b, m, :n]]
        theirs = gen["logprobs"][b, :n].cpu().numpy()
        assert gen["tokens"][b, :n].tolist() == plan.members(b)[m]
        scale = float(np.abs(g["mean"][b][VU.first_columns(g)[b]]).max())
        print(f"{dtype} sample {b}: member {c}, worst edge difference {float(np.abs(mine - theirs).max()):.3e}")
        assert float(np.abs(mine - theirs).max()) <= bound * scale


@pytest.mark.parametrize("dtype", DTYPES)
def test_eight_members_and_the_full_beam_agree(dtype):
    """On a set of <= 8 members the constrained beam with a slot per member is exact: its choice is score_vocab's prediction."""
    from fvqa import generate
    name = "vocab_tiny"
    g = VU.load(name)
    eng, batch = engine_of(name, dtype), VU.fixture_batch(g)
    sets = []
    for s in VU.fixture_sets(g):
        short, seen = [], set()
        for seq in s:
            if len(seq) <= 6 and tuple(seq) not in seen and len(short) < 8:
                short.append(seq)
                seen.add(tuple(seq))
        sets.append(short)
    r = vocab.score_vocab(eng, batch, sets, top=8)
    beam = generate.generate(eng, batch, temperature=0.0, constraints=sets, num_beams=8, length_penalty=1.0, max_new_tokens=8)
    mean = r["mean"].cpu().numpy().astype(np.float64)
    two = -np.sort(-mean, axis=1)[:, :2]
    decided = (two[:, 0] - two[:, 1]) > 4 * bound_of(name, dtype) * np.abs(two[:, 1])
    assert int(decided.sum()) >= 3
    assert np.array_equal(r["prediction"].cpu().numpy()[decided], beam["choice"].cpu().numpy()[decided])


def test_blind_contrast_of_a_blind_batch_changes_nothing():
    name = "vocab_tiny"
    g = VU.load(name)
    eng, batch, sets = engine_of(name, torch.bfloat16), VU.fixture_batch(g, blind=True), VU.fixture_sets(g)
    plain = vocab.score_vocab(eng, batch, sets)
    for route in vocab.ROUTES:
        r = vocab.score_vocab(eng, batch, sets, route=route, contrast="blind", contrast_alpha=0.7)
        assert torch.equal(U.bits(r["mean_blind"]), U.bits(r["mean"]))
        assert torch.equal(r["prediction"], r["prediction_plain"]) and torch.equal(r["prediction_blind"], r["prediction_plain"])
    assert torch.equal(r["prediction_plain"], plain["prediction"])


def test_model_wrapper_leaves_the_reductions_behind():
    from tests.test_generate_gpu import model_of
    g = VU.load("vocab_tiny")
    model = model_of("tiny_peakedperm", torch.float32)
    r = model.score_vocab(VU.fixture_batch(g), VU.fixture_sets(g), top=3)
    assert tuple(r["ranking"].shape) == (3, 3) and model.last_scoring["route"] == "tree"
    assert torch.equal(model.last_scoring["prediction"], r["prediction"])
    assert np.array_equal(r["prediction"].cpu().numpy(), g["prediction"])


def test_val_one_epoch_classifies_over_the_vocabulary(monkeypatch):
    """engine.val_one_epoch under --val_vocab on the tiny fixture (fp32): the gold answer is the preferred member for sample 0, a
    member the model ranks behind it for sample 1 and no member at all for sample 2 — acc, acc_top5, gold_in_vocab and gold_nll
    are what the fixture's own numbers give."""
    import types

    import engine
    from tests.test_generate_gpu import model_of
    g = VU.load("vocab_tiny")
    sets, cols = VU.fixture_sets(g), VU.first_columns(g)
    shared = sets[1]                                                    # one vocabulary for the batch: sample 1's list
    answers = [f"answer {m}" for m in range(len(shared))]
    model = model_of("tiny_peakedperm", torch.float32)
    monkeypatch.setattr(model, "answer_vocab", lambda: (answers, shared), raising=False)
    batch = VU.fixture_batch(g)
    keep = torch.tensor([1])                                            # sample 1 three times: its list is the vocabulary
    one = {"video": batch["video"][keep].repeat(3, 1, 1), "text_id": {"vqa": batch["text_id"]["vqa"][keep].repeat(3, 1, 1)},
           "label": {"vqa": batch["label"]["vqa"][keep].repeat(3, 1, 1)}, "video_start": {"vqa": [batch["video_start"]["vqa"][1]] * 3},
           "prefix_index": {"vqa": [batch["prefix_index"]["vqa"][1]] * 3}, "vid": [None] * 3}
    best = int(g["prediction"][1])
    order = sorted((m for m in range(len(shared)) if cols[1, m]), key=lambda m: (-g["mean"][1, m], m))
    far = order[10]                                                     # a member outside the top five
    one.update(answer=torch.tensor([0, 0, 0]), qtype=torch.zeros(3, dtype=torch.int64),
               text=[{"options": [answers[best]]}, {"options": [answers[far]]}, {"options": ["no member"]}])
    opt = types.SimpleNamespace(param_groups=[{"lr": 0.25}])
    args = types.SimpleNamespace(is_generation_task=True, val_vocab=True, dataset="musicavqa", debug=False, output_dir=None)
    stats = engine.val_one_epoch(model, [one], opt, epoch=1, args=args)
    lp = g["logprob_sum"][1].astype(np.float64)
    post = lp - np.log(np.exp(lp[cols[1]]).sum())
    assert stats["acc"] == pytest.approx(1 / 3) and stats["acc_top5"] == pytest.approx(1 / 3)
    assert stats["gold_in_vocab"] == pytest.approx(2 / 3)
    assert stats["gold_nll"] == pytest.approx(-(post[best] + post[far]) / 2, rel=VU.FP32_RTOL)
    assert model.last_scoring["route"] == "tree" and tuple(model.last_scoring["ranking"].shape) == (3, 5)
