"""Option scoring by all three flipped tasks (fvqa/flipped.py, csrc/flipped.hip), the parts that need no GPU: the per-option
labels against the reference reader's own, the widened planner, the pick rule, the test's fp64 restatement of the wide suffix
attention against the oracle, the flags, `engine.val_one_epoch`'s bookkeeping under --val_flipped, the C ABI."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import engine
import train
from fvqa import _lib, flipped, ops, score
from tests import flipped_util as FU
from tests.test_score_cpu import F, hand_case, loader_case

NAN = float("nan")


# ------------------------------------------------------------------------------------------------ option_rows
@pytest.mark.parametrize("name", ["flipped_tiny", "flipped_7b_l2_peakedperm"])
def test_option_rows_equal_the_readers_on_equal_length_options(name):
    """Multiple-choice reader: every option is a letter, all options of a sample have one length, and each option's own
    positions are the gold option's — option_rows gives the reader's own label["vaq"], label["qav"], prefix_index and
    video_index["qav"], for every option."""
    g = FU.load(name)
    rows = flipped.option_rows(FU.golden_batch(g), F)
    B, O, S = g["text_id_vaq"].shape
    assert (B, O, S) == (4, 5, FU.S_FIX)
    assert np.array_equal(rows["label"]["vaq"].numpy(), g["reader_label_vaq"])
    assert np.array_equal(rows["label"]["qav"].numpy(), g["reader_label_qav"])
    for t in ("vaq", "qav"):
        assert np.array_equal(rows["prefix_index"][t].numpy(), np.repeat(g[f"reader_prefix_{t}"][:, None], O, 1))
    assert np.array_equal(rows["video_index"]["qav"].numpy(), np.repeat(g["reader_video_index_qav"][:, None], O, 1))
    assert rows["video_index"]["qav"].shape == (B, O, F)


def test_option_rows_take_each_options_own_positions():
    """Options of different lengths. Hand-made: the marker sits at another index in every option. Generation-task reader
    (free-text options): the reader's positions are the gold option's, option_rows' differ between the options."""
    Q, V, S = 16492, 15167, 24
    ids = torch.arange(100, 100 + 2 * 3 * S).view(2, 3, S)
    qpos = torch.tensor([[3, 5, 9], [4, 4, 20]])
    vpos = torch.tensor([[2, 7, 12], [0, 15, 21]])                    # (1, 2): the frames run over the end of the sequence
    vaq, qav = ids.clone(), ids.clone()
    for n in range(2):
        for c in range(3):
            vaq[n, c, qpos[n, c]] = Q
            vaq[n, c, min(int(qpos[n, c]) + 3, S - 1)] = Q                # a later occurrence does not count
            qav[n, c, vpos[n, c]] = V
    rows = flipped.option_rows({"text_id": {"vaq": vaq, "qav": qav}}, F)
    assert torch.equal(rows["prefix_index"]["vaq"], qpos + 2) and torch.equal(rows["prefix_index"]["qav"], vpos + 2)
    for n in range(2):
        for c in range(3):
            p = int(qpos[n, c]) + 2
            assert not bool(rows["label"]["vaq"][n, c, :p].any()) and torch.equal(rows["label"]["vaq"][n, c, p:], vaq[n, c, p:])
            p = int(vpos[n, c]) + 2
            k = min(F, S - p)
            want = torch.full((S,), -1)
            want[p:p + k] = torch.arange(k)
            assert torch.equal(rows["label"]["qav"][n, c], want)
            assert torch.equal(rows["video_index"]["qav"][n, c], p + torch.arange(F))
    assert int(rows["video_index"]["qav"][1, 2].max()) >= S           # score_flipped refuses such a batch (below)
    with pytest.raises(ValueError):
        flipped.option_rows({"text_id": {"vaq": ids}}, F)             # no marker
    g = FU.load("flipped_tiny_gen")
    assert bool(g["is_generation_task"])
    rows = flipped.option_rows(FU.golden_batch(g), F)
    own, gold = rows["prefix_index"]["qav"].numpy(), g["reader_prefix_qav"]
    ans = g["answer"]
    assert np.array_equal(own[np.arange(4), ans], gold)               # the reader's positions are the gold option's
    assert (own != gold[:, None]).any()                               # ... and not every option's
    assert np.array_equal(rows["label"]["qav"].numpy()[np.arange(4), ans], g["reader_label_qav"][np.arange(4), ans])


# ------------------------------------------------------------------------------------------------ the planner
def same_plan(a, b):
    return (torch.equal(a.start, b.start) and torch.equal(a.length, b.length) and a.T == b.T and a.shared == b.shared
            and a.why_dense == b.why_dense and torch.equal(a.rows, b.rows))


def test_planner_defaults_decide_as_before():
    """Without the new keywords — and with them at their defaults — plan_options decides what tests/test_score_cpu.py pins."""
    for name, T in (("s128_val", 4), ("s128_gen_val", 9)):
        ids, lab, prefix, vs = loader_case(name)
        p = score.plan_options(ids, lab, prefix.tolist(), vs.tolist(), F)
        q = score.plan_options(ids, lab, prefix.tolist(), vs.tolist(), F, suffix_max=None, frames_in_suffix=False, qav=False)
        assert same_plan(p, q) and p.shared and p.T == T and torch.equal(p.start, prefix - 1)
    ids, lab = hand_case()
    bad = ids.clone()
    bad[0, 1, 7] = 999
    ids17, lab17 = hand_case(n_ans=17)
    ids2, lab2 = torch.cat([ids, ids]), torch.cat([lab, torch.zeros_like(lab)])
    for (i, l, pf, v), shared, word in (((ids, lab, [40], [5]), True, ""), ((bad, lab, [40], [5]), False, "frame"),
                                        ((ids17, lab17, [40], [5]), False, "17"), ((ids2, lab2, [40, 40], [5, 5]), False, "no scored")):
        p = score.plan_options(i, l, pf, v, F)
        assert p.shared == shared and word in p.why_dense
        assert same_plan(p, score.plan_options(i, l, pf, v, F, suffix_max=ops.SUFFIX_MAX, frames_in_suffix=False, qav=False))
    assert ops.SUFFIX_MAX == 16 and ops.SUFFIX_WIDE_MAX == 64


def test_planner_widened():
    ids17, lab17 = hand_case(n_ans=17)
    p = score.plan_options(ids17, lab17, [40], [5], F, suffix_max=64)
    assert p.shared and p.T == 17 and p.start.tolist() == [39]
    # a frame slot in the suffix: turned down as ever, taken with the keyword (start, length and rows are the same)
    ids, lab = hand_case()
    bad = ids.clone()
    bad[0, 1, 7] = 999
    p0 = score.plan_options(bad, lab, [40], [5], F, suffix_max=64)
    p1 = score.plan_options(bad, lab, [40], [5], F, suffix_max=64, frames_in_suffix=True)
    assert not p0.shared and p1.shared and p1.start.tolist() == [7] and p1.length.tolist() == [35] and torch.equal(p0.rows, p1.rows)
    assert not score.plan_options(bad, lab, [40], [5], F, suffix_max=34, frames_in_suffix=True).shared
    # the QAV head's rule: label[t + 1] >= 0 scores row t (a frame index 0 counts), -1 does not
    qlab = torch.full_like(lab, -1)
    qlab[0, :, 42:42 + F] = torch.arange(F)
    p = score.plan_options(ids, qlab, None, None, F, suffix_max=63, frames_in_suffix=True, qav=True)
    assert p.shared and p.start.tolist() == [41] and p.length.tolist() == [F] and p.rows.shape[0] == 3 * F
    assert not score.plan_options(ids, qlab, None, None, F, suffix_max=63, frames_in_suffix=True).rows[:, 2].eq(41).any()


def test_fixture_suffixes_fall_in_the_four_buckets():
    """The fixtures' VAQ suffixes: below 16 rows, 17..32, 33..64 and above 64 — the last sends the batch the dense way, the first
    three samples alone take the shared form; the QAV suffixes are F + 4 rows with their frame slots inside."""
    g = FU.load("flipped_tiny")
    batch = FU.golden_batch(g)
    rows = flipped.option_rows(batch, F)
    ids, lab = batch["text_id"]["vaq"], rows["label"]["vaq"]
    p = score.plan_options(ids, lab, None, batch["video_start"]["vaq"], F, suffix_max=flipped.SUFFIX_LIMIT["vaq"])
    L = p.length.tolist()
    assert L[0] < 16 and 17 <= L[1] <= 32 and 33 <= L[2] <= 64 and L[3] > 64, L
    assert not p.shared and str(L[3]) in p.why_dense and flipped._route("vaq", p, None) == "dense"
    with pytest.raises(ValueError):
        flipped._route("vaq", p, "shared")
    p3 = score.plan_options(ids[:3], lab[:3], None, batch["video_start"]["vaq"][:3], F, suffix_max=flipped.SUFFIX_LIMIT["vaq"])
    assert p3.shared and p3.T == L[2]
    q = score.plan_options(batch["text_id"]["qav"], rows["label"]["qav"], None, None, F, suffix_max=flipped.SUFFIX_LIMIT["qav"],
                           frames_in_suffix=True, qav=True)
    assert q.shared and q.length.tolist() == [F + 4] * 4            # the answer letter's rows, the marker's two, F - 1 frame rows
    assert torch.equal(q.start + q.length, rows["prefix_index"]["qav"].max(1).values + F - 1)
    assert bool((q.start < rows["prefix_index"]["qav"].min(1).values).all())
    # counts in the fixture are the labels' scored rows
    assert np.array_equal(g["count_vaq"], (lab[:, :, 1:] > 0).sum(-1).numpy())
    assert np.array_equal(g["count_qav"], np.full((4, 5), F))


def test_route_defaults(monkeypatch):
    ids, lab = hand_case()
    p = score.plan_options(ids, lab, [40], [5], F, suffix_max=64)
    monkeypatch.delenv("FVQA_SCORE", raising=False)
    assert [flipped._route(t, p, None) for t in flipped.TASKS] == [flipped.DEFAULT_ROUTE[t] for t in flipped.TASKS]
    monkeypatch.setenv("FVQA_SCORE", "shared")
    assert flipped._route("vaq", p, None) == "shared" and flipped._route("qav", p, "dense") == "dense"
    monkeypatch.setenv("FVQA_SCORE", "fastest")
    with pytest.raises(ValueError):
        flipped._route("vaq", p, None)
    with pytest.raises(ValueError):
        flipped._route("vaq", p, "fastest")


# ------------------------------------------------------------------------------------------------ the pick rule
def pick_case():
    """B = 6, O = 4. Sample 0: plain; 1: options 0 and 2 tie in the total (-> 0); 2: a NaN mean at an eligible option (-> it);
    3: no option is eligible (-> 0); 4: the lowest total sits at an option one task did not score (skipped); 5: the tasks
    disagree."""
    m = {"vqa": np.array([[3, 1, 2, 4], [1, 5, 2, 9], [1, 2, 3, 4], [1, 2, 3, 4], [0.5, 2, 3, 4], [1, 2, 3, 4]], np.float32),
         "vaq": np.array([[1, 1, 1, 1], [2, 5, 1, 9], [1, NAN, 1, 1], [1, 1, 1, 1], [0.5, 1, 1, 1], [4, 3, 2, 1.5]], np.float32),
         "qav": np.array([[2, 2, 2, 2], [1, 5, 1, 9], [1, 1, 1, 1], [1, 1, 1, 1], [0.5, 1, 1, 1], [2, 2, 1, 2.25]], np.float32)}
    c = {t: np.full((6, 4), 3, np.int64) for t in m}
    c["vaq"][3] = 0
    c["qav"][4, 0] = 0
    return m, c, np.array([1, 2, 0, 3, 0, 7], np.int64)


def test_pick_rule_on_hand_made_cases():
    m, c, ans = pick_case()
    total, pred, pred_t, gold = flipped.pick_rule(m, c, (1.0, 1.0, 1.0), ans)
    assert pred.tolist() == [1, 0, 1, 0, 1, 2]
    assert pred_t.tolist() == [[1, 0, 0, 0, 0, 0], [0, 2, 1, 0, 0, 3], [0, 0, 0, 0, 1, 2]]
    assert np.array_equal(total[0], np.array([6, 4, 5, 7], np.float32)) and np.isnan(total[2, 1])
    assert gold[0].tolist() == [1, 1, 2] and np.isnan(gold[5]).all() and gold.shape == (6, 3)
    # a zero weight drops a task from the total but not from eligibility; a negative one turns its order round
    _, pred, _, _ = flipped.pick_rule(m, c, (0.0, 1.0, 0.0), ans)
    assert pred.tolist() == [0, 2, 1, 0, 1, 3]
    _, pred, _, _ = flipped.pick_rule(m, c, (1.0, -1.0, 0.0), None)
    assert pred[5] == 0 and pred[0] == 1
    # an absent task: skipped in the total, -1 in prediction_t, NaN in gold_loss
    two = {t: m[t] for t in ("vqa", "qav")}
    total, pred, pred_t, gold = flipped.pick_rule(two, {t: c[t] for t in two}, (1.0, 5.0, 2.0), ans)
    assert np.array_equal(total, m["vqa"] + 2 * m["qav"]) and pred_t[1].tolist() == [-1] * 6 and np.isnan(gold[:, 1]).all()
    assert pred[3] == 0 and pred[2] == 0                             # (vaq's zero counts and NaN are out of the picture)


# ------------------------------------------------------------------------------------------------ the test's own restatement
@pytest.mark.parametrize("cache_rotated", [False, True])
def test_wide_restatement_is_the_oracle_and_its_defects_show(cache_rotated):
    """tests/flipped_util.wide_restated — the kernel's contract from the operands it is handed — equals the rows of the full-sequence
    fp64 oracle wherever the oracle exists (A = 10), and each planted defect moves it by far more than any bound."""
    dt = torch.float32
    seen = set()
    for T in (17, 64):
        for O, st, ln, A, Fw, vs in FU.wide_schedule(T):
            if A == 0:
                continue
            c = FU.wide_case(dt, cache_rotated, T, O, st, ln, A, Fw, vs, seed=7 + T)
            v = c["valid"]
            assert float((FU.wide_restated(c, dt, cache_rotated)[v] - c["want"][v]).abs().max()) < 1e-12
            for d in ("causal", "option", "gate2"):
                if float(FU.wide_restated(c, dt, cache_rotated, defect=d)[v].sub(c["want"][v]).abs().max()) > 0.05:
                    seen.add(d)
    assert seen == {"causal", "option", "gate2"}


# ------------------------------------------------------------------------------------------------ flags
def test_parser_refusals(capsys):
    P = train.get_args_parser()
    a = P.parse_args(["--val_flipped"])
    assert a.val_flipped and a.val_flipped_weights is None
    a = P.parse_args(["--val_flipped", "--val_flipped_weights", "0.5", "0.25"])
    assert a.val_flipped_weights == [0.5, 0.25]
    assert not P.parse_args([]).val_flipped
    for bad in (["--val_flipped", "--is_generation_task"], ["--val_flipped", "--contrast", "blind"],
                ["--val_flipped", "--val_frame_attention"], ["--val_flipped_weights", "1", "1"],
                ["--val_flipped", "--val_flipped_weights", "1"]):
        with pytest.raises(SystemExit):
            P.parse_args(bad)
    capsys.readouterr()


def test_score_flipped_refuses_before_any_launch():
    g = FU.load("flipped_tiny")
    batch = FU.golden_batch(g)
    for kw in ({"tasks": ()}, {"tasks": ("vqa", "qva")}, {"tasks": ("vaq", "vaq")}, {"weights": (1.0, 1.0)}):
        with pytest.raises(ValueError):
            flipped.score_flipped(None, batch, **kw)
    with pytest.raises(ValueError):
        flipped.score_flipped(None, {"text_id": {"vqa": batch["text_id"]["vqa"]}}, tasks=("vaq",))


# ------------------------------------------------------------------------------------------------ val_one_epoch
class _FlippedStub(torch.nn.Module):
    """The total picks the answer except in sample 0; vqa alone is always right, vaq never, qav on even samples."""

    def score_options(self, data):
        raise AssertionError("--val_flipped scores through score_flipped")

    def score_flipped(self, data, **kw):
        self.kw = kw
        ans = data["answer"]
        B = ans.shape[0]
        miss = (ans + 1) % 5
        total = ans.clone()
        total[0] = miss[0]
        qav = torch.where(torch.arange(B) % 2 == 0, ans, miss)
        gold = torch.stack([torch.full((B,), 1.0), torch.arange(B).float(), torch.full((B,), 0.25)], 1)
        return {"prediction": total, "prediction_vqa": ans, "prediction_vaq": miss, "prediction_qav": qav, "gold_loss": gold}


def test_val_one_epoch_flipped_bookkeeping():
    stub = _FlippedStub()
    batches = [{"answer": torch.tensor([0, 1, 2, 3]), "qtype": torch.tensor([1, 3, 6, 8]), "vid": list("abcd")}] * 2
    opt = types.SimpleNamespace(param_groups=[{"lr": 0.5}])
    args = types.SimpleNamespace(is_generation_task=False, dataset="nextqa", debug=False, output_dir=None, val_flipped=True,
                                 val_flipped_weights=[0.5, 2.0])
    stats = engine.val_one_epoch(stub, batches, opt, epoch=0, args=args)
    assert stub.kw["weights"] == (1.0, 0.5, 2.0) and torch.equal(stub.kw["answer"], batches[0]["answer"])
    assert stats["acc"] == pytest.approx(0.75) and stats["Total"] == pytest.approx(0.75) and stats["lr"] == 0.5
    assert stats["acc_vqa"] == pytest.approx(1.0) and stats["acc_vaq"] == 0.0 and stats["acc_qav"] == pytest.approx(0.5)
    assert stats["vaq_loss"] == pytest.approx(1.5) and stats["qav_loss"] == pytest.approx(0.25)
    assert stats["C"] == pytest.approx(0.0, abs=1e-9)                 # qtype 1 is the sample the total misses
    args.val_flipped_weights = None
    engine.val_one_epoch(stub, batches[:1], opt, epoch=0, args=args)
    assert stub.kw["weights"] == (1.0, 1.0, 1.0)


# ------------------------------------------------------------------------------------------------ C ABI
def test_cabi_flipped_entry_points():
    """The three new symbols are exported by both builds at ABI 18 (entries are only added) with the signatures of fvqa/_lib.py;
    operands are checked before any launch, so the checks can be called with made-up addresses and no GPU."""
    p, i, f = C.c_void_p, C.c_int, C.c_float
    assert _lib.SIGNATURES["fvqa_attn_suffix_wide"] == _lib.SIGNATURES["fvqa_attn_suffix"]
    assert _lib.SIGNATURES["fvqa_suffix_embed"] == (i, [p] * 6 + [i] * 7 + [p])
    assert _lib.SIGNATURES["fvqa_flipped_pick"] == (i, [p] * 6 + [f] * 3 + [p] * 5 + [i] * 2 + [p])
    one = C.c_void_p(256)
    for which, code, other in (("bf16", _lib.BF16, _lib.F16), ("f16", _lib.F16, _lib.BF16)):
        lib = _lib.load(which)
        assert lib.fvqa_version() == _lib.ABI_VERSION == 18
        ptrs = [one] * 10
        wide = lib.fvqa_attn_suffix_wide
        assert wide(*([None] + ptrs[1:]), 2, 5, 40, 128, 2, 128, 10, 10, 1, code, None) == -1               # null pointer
        assert wide(*ptrs, 2, 5, 40, 128, 2, 128, 10, 10, 1, other, None) == -1                             # the other build's type
        assert wide(*ptrs, 2, 5, 65, 128, 2, 128, 10, 10, 1, code, None) == -2                              # 65 suffix rows
        assert wide(*ptrs, 2, 5, 0, 128, 2, 128, 10, 10, 1, code, None) == -2
        assert wide(*ptrs, 2, 4097, 33, 128, 2, 128, 10, 10, 1, code, None) == -2                           # > 4096 options
        assert wide(*ptrs, 2, 5, 40, 4097, 2, 128, 10, 10, 1, code, None) == -2                             # S > 4096
        assert wide(*ptrs, 2, 5, 40, 128, 2, 64, 10, 10, 1, _lib.F32, None) == -2                           # head_dim != 128
        assert wide(*([C.c_void_p(260)] + ptrs[1:]), 2, 5, 40, 128, 2, 128, 10, 10, 1, code, None) == -3
        emb = lib.fvqa_suffix_embed
        assert emb(None, one, one, one, one, one, 2, 5, 40, 512, 32000, 10, code, None) == -1
        assert emb(one, one, one, None, one, one, 2, 5, 40, 512, 32000, 10, code, None) == -1               # a slot map, no frames
        assert emb(one, one, one, one, one, one, 2, 5, 40, 512, 32000, 10, other, None) == -1
        assert emb(one, one, one, one, one, one, 2, 5, 40, 512, 32000, 0, code, None) == -2                 # ... or no frame count
        assert emb(one, None, one, None, one, one, 2, 5, 0, 512, 32000, 10, code, None) == -2
        assert emb(one, None, one, None, one, one, 2, 5, 40, 4, 32000, 10, code, None) == -2                # rows of 8 bytes
        assert emb(one, None, one, None, one, C.c_void_p(264), 2, 5, 40, 512, 32000, 10, code, None) == -3
        pick = lib.fvqa_flipped_pick
        assert pick(one, None, None, one, None, None, 1.0, 1.0, 1.0, None, None, one, one, None, 4, 5, None) == -1     # no total
        assert pick(None, None, None, None, None, None, 1.0, 1.0, 1.0, None, one, one, one, None, 4, 5, None) == -1    # no task
        assert pick(one, one, None, one, None, None, 1.0, 1.0, 1.0, None, one, one, one, None, 4, 5, None) == -1       # mean, no count
        assert pick(one, None, None, one, None, None, 1.0, 1.0, 1.0, one, one, one, one, None, 4, 5, None) == -1       # answer, no gold
        assert pick(one, None, None, one, None, None, 1.0, 1.0, 1.0, None, one, one, one, None, 4, 65, None) == -2     # > 64 options
        assert pick(one, None, None, one, None, None, 1.0, 1.0, 1.0, None, one, one, one, None, 0, 5, None) == -2


def test_ops_refuse_on_the_host():
    """ops' checks come before the library is touched: CPU tensors, wrong counts."""
    x = torch.zeros(4, 8)
    with pytest.raises(ValueError):
        ops.suffix_embed(torch.zeros(4, dtype=torch.int64), None, torch.zeros(16, 8), None, torch.zeros(1, dtype=torch.int32), x,
                         1, 1, 4, 0)
    with pytest.raises(ValueError):
        ops.flipped_pick({"vqa": torch.zeros(2, 3)}, {"vqa": torch.zeros(2, 3, dtype=torch.int64)}, (1.0, 1.0, 1.0))
    with pytest.raises(ValueError):
        ops.flipped_pick({"vqa": torch.zeros(2, 3)}, {"vaq": torch.zeros(2, 3, dtype=torch.int64)}, (1.0, 1.0, 1.0))
    with pytest.raises(ValueError):
        ops.flipped_pick({}, {}, (1.0, 1.0, 1.0))
