"""Option scoring (fvqa/score.py, csrc/score.hip), the parts that need no GPU: the planner, the reference-generated fixtures
checked against themselves, `engine.val_one_epoch`'s bookkeeping in the multiple-choice mode, the C ABI."""
import ctypes as C
import os
import types

import numpy as np
import pytest
import torch

import engine
from fvqa import _lib, ops, score, synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F = 10


def loader_case(name):
    g = np.load(os.path.join(GOLDEN, "loader_nextqa.npz"))
    t = lambda k: torch.from_numpy(g[f"{name}__{k}__vqa"])          # noqa: E731
    return t("text_id"), t("label"), t("prefix_index"), t("video_start")


def test_planner_on_the_loader_fixture():
    """The reference reader's validation batches: the five options of a sample are equal up to prefix + 1 and the scored rows are
    prefix-1 .. prefix+2, so start = prefix - 1 and four suffix rows; the generation-mode reader (free-text options of 1..8
    tokens) gives 2..9 rows. Both take the shared form."""
    ids, lab, prefix, vs = loader_case("s128_val")
    p = score.plan_options(ids, lab, prefix.tolist(), vs.tolist(), F)
    assert p.shared and p.why_dense == "" and p.T == 4
    assert torch.equal(p.start, prefix - 1) and torch.equal(p.length, torch.full_like(prefix, 4))
    n, c, t = p.rows.unbind(1)
    assert p.rows.shape[0] == ids.shape[0] * ids.shape[1] * 4
    assert bool(((t >= p.start[n]) & (t < p.start[n] + p.length[n])).all())          # every scored row lies in its suffix
    ids, lab, prefix, vs = loader_case("s128_gen_val")
    p = score.plan_options(ids, lab, prefix.tolist(), vs.tolist(), F)
    assert p.shared and int(p.length.min()) == 2 and int(p.length.max()) == 9 and p.T == 9
    assert torch.equal(p.start, prefix - 1)
    # the options really are equal in front of `start`, and the rows behind start + length are read by no scored row
    assert bool((ids[:, :, :int(p.start.min())] == ids[:, :1, :int(p.start.min())]).all())
    for b in range(ids.shape[0]):
        s, e = int(p.start[b]), int(p.start[b] + p.length[b])
        assert bool((ids[b, :, :s] == ids[b, :1, :s]).all()) and not bool((lab[b, :, e + 1:] > 0).any())


def hand_case(S=64, O=3, vs=5, prefix=40, n_ans=3):
    ids = torch.arange(3, 3 + S).repeat(1, O, 1)
    ids[0, :, vs:vs + F] = 0
    lab = torch.zeros(1, O, S, dtype=torch.int64)
    for c in range(O):
        ids[0, c, prefix + 1] = 1000 + c
        ids[0, c, prefix + n_ans:] = 0
        lab[0, c, prefix:prefix + n_ans] = ids[0, c, prefix:prefix + n_ans]
    return ids, lab


def test_planner_hand_made_cases():
    ids, lab = hand_case()
    p = score.plan_options(ids, lab, [40], [5], F)
    assert p.shared and p.start.tolist() == [39] and p.length.tolist() == [3]
    assert score.route_of(p) == score.DEFAULT_ROUTE
    # an option that differs inside the frame slots
    bad = ids.clone()
    bad[0, 1, 7] = 999
    p = score.plan_options(bad, lab, [40], [5], F)
    assert not p.shared and "frame" in p.why_dense and p.start.tolist() == [7]
    assert score.route_of(p) == "dense"
    # ... or right behind them: the first row after the frames still belongs to the prompt (start >= vs + F + 1)
    ids18, lab18 = hand_case(prefix=18)
    edge = ids18.clone()
    edge[0, 2, 5 + F] = 999
    p = score.plan_options(edge, lab18, [18], [5], F)
    assert not p.shared and p.start.tolist() == [15] and p.length.tolist() == [5]
    edge = ids18.clone()
    edge[0, 2, 5 + F + 1] = 999
    p = score.plan_options(edge, lab18, [18], [5], F)
    assert p.shared and p.start.tolist() == [16] and p.length.tolist() == [4]
    # 17 suffix rows: one more than the attention kernel takes
    ids17, lab17 = hand_case(n_ans=17)
    p = score.plan_options(ids17, lab17, [40], [5], F)
    assert p.length.tolist() == [17] and not p.shared and "17" in p.why_dense
    ids16, lab16 = hand_case(n_ans=16)
    assert score.plan_options(ids16, lab16, [40], [5], F).shared and ops.SUFFIX_MAX == 16
    # a sample with no scored row sends the whole batch the dense way
    ids2 = torch.cat([ids, ids]); lab2 = torch.cat([lab, torch.zeros_like(lab)])
    p = score.plan_options(ids2, lab2, [40, 40], [5, 5], F)
    assert not p.shared and "no scored row" in p.why_dense and p.length.tolist() == [3, 0]
    with pytest.raises(ValueError):
        score.plan_options(ids, lab[:, :2], [40], [5], F)


def test_route_switch(monkeypatch):
    ids, lab = hand_case()
    p = score.plan_options(ids, lab, [40], [5], F)
    monkeypatch.setenv("FVQA_SCORE", "dense")
    assert score.route_of(p) == "dense"
    monkeypatch.setenv("FVQA_SCORE", "shared")
    assert score.route_of(p) == "shared"
    monkeypatch.setenv("FVQA_SCORE", "fastest")
    with pytest.raises(ValueError):
        score.route_of(p)


def test_make_option_batch_is_validation_shaped():
    cfg = synth.preset("7b")
    b = synth.make_option_batch(cfg, n_options=5, seed=3)
    ids, lab = b["text_id"]["vqa"], b["label"]["vqa"]
    assert ids.shape == (8, 5, 128) and lab.shape == ids.shape and b["answer"].shape == (8,)
    assert torch.equal(ids, synth.make_option_batch(cfg, n_options=5, seed=3)["text_id"]["vqa"])     # closed form
    p = score.plan_options(ids, lab, b["prefix_index"]["vqa"], b["video_start"]["vqa"], cfg.max_feats)
    assert p.shared and 3 <= int(p.length.min()) and int(p.length.max()) <= 5
    assert p.start.tolist() == [x - 1 for x in b["prefix_index"]["vqa"]]
    for n in range(8):                                       # the options differ, and only from the answer's second token on
        first = int(b["prefix_index"]["vqa"][n]) + 1
        assert len({int(x) for x in ids[n, :, first]}) == 5 and bool((ids[n, :, :first] == ids[n, :1, :first]).all())
    assert bool(((lab == 0) | (lab == ids)).all()) and int(ids.min()) >= 0 and int(ids.max()) < cfg.vocab_size


SCORE_FIXTURES = ["score_tiny", "score_7b_l2", "score_7b_l2_peakedperm"]


@pytest.mark.parametrize("name", SCORE_FIXTURES)
def test_goldens_checked_alone(name):
    """What the reference left in the fixture is consistent with its own protocol (engine.py:88-93), and its batch is one the
    shared form takes."""
    g = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
    il = torch.from_numpy(g["individual_losses"])
    B, O, S1 = il.shape
    assert (B, O, S1) == (4, 5, 127) and g["text_id_vqa"].shape == (4, 5, 128)
    count = (il != 0).sum(-1)
    mean = il.sum(-1) / count
    assert np.array_equal(count.numpy(), g["count"]) and np.allclose(mean.numpy(), g["mean"], rtol=1e-6)
    assert np.array_equal(mean.argmin(-1).numpy(), g["prediction"])
    two = mean.sort(-1).values[:, :2]
    assert np.allclose(((two[:, 1] - two[:, 0]) / two[:, 0]).numpy(), g["gap"], rtol=1e-4, atol=1e-7)
    assert float(g["gap"].min()) > 1e-4                      # every sample's choice is decided at fp32 precision
    if name.endswith("peakedperm"):                          # the variant kept for the 16-bit pins: the largest gaps of the three
        assert float(g["gap"].min()) > 5e-3
    # zeros exactly where the labels ignore the row
    lab = torch.from_numpy(g["label_vqa"])
    assert torch.equal(il != 0, lab[:, :, 1:] > 0)
    p = score.plan_options(torch.from_numpy(g["text_id_vqa"]), lab, g["prefix_vqa"].tolist(), g["vstart_vqa"].tolist(), F)
    assert p.shared and p.T == 4 and torch.equal(p.start, torch.from_numpy(g["prefix_vqa"]) - 1)


class _ScoringStub(torch.nn.Module):
    """A model with the multiple-choice branch: option (answer + miss) % 5 gets the lowest loss."""

    def __init__(self, with_last=True):
        super().__init__()
        self.with_last, self.calls = with_last, 0

    def score_options(self, data):
        self.calls += 1
        ans = data["answer"].clone()
        ans[0] = (ans[0] + 1) % 5                            # one miss per batch
        il = torch.zeros(ans.shape[0], 5, 7)
        il[:, :, 2:5] = 2.0
        il[torch.arange(ans.shape[0]), ans, 2:5] = 1.0
        if self.with_last:
            self.last_scoring = {"prediction": ans, "mean": il.sum(-1) / 3, "count": (il != 0).sum(-1), "route": "dense"}
        return il

    def forward(self, data, inference=False):
        raise AssertionError("the multiple-choice mode must not call the generation path")


@pytest.mark.parametrize("with_last", [True, False])
@pytest.mark.parametrize("wrapped", [False, True])
def test_val_one_epoch_scoring_bookkeeping(with_last, wrapped):
    """Accuracy, the C / T / D / Total meters and lr as reference engine.py:86-93,122-136 computes them — from the device-side
    prediction when the model leaves one, from the returned losses otherwise; score_options may sit on `model.module`."""
    stub = _ScoringStub(with_last)
    model = stub
    if wrapped:
        model = torch.nn.Module()
        model.module = stub
    batches = [{"answer": torch.tensor([0, 1, 2, 3]), "qtype": torch.tensor([1, 3, 6, 8]), "vid": list("abcd")}] * 3
    opt = types.SimpleNamespace(param_groups=[{"lr": 0.5}])
    args = types.SimpleNamespace(is_generation_task=False, dataset="nextqa", debug=False, output_dir=None)
    stats = engine.val_one_epoch(model, batches, opt, epoch=2, args=args)
    assert stub.calls == 3
    assert stats["acc"] == pytest.approx(0.75) and stats["Total"] == pytest.approx(0.75) and stats["lr"] == 0.5
    eps = 1e-10
    assert stats["C"] == pytest.approx(0.0, abs=1e-9)                        # qtype 1 is the sample that misses
    assert stats["T"] == pytest.approx(1 / (1 + eps)) and stats["D"] == pytest.approx(2 / (2 + eps))
    # args without the flag at all (a plain `train.py` run) take the same branch
    stats = engine.val_one_epoch(model, batches, opt, epoch=2, args=types.SimpleNamespace(dataset="nextqa", debug=True))
    assert stub.calls == 4 and stats["acc"] == pytest.approx(0.75)


def test_val_one_epoch_without_score_options_is_rejected():
    class Stub(torch.nn.Module):
        def forward(self, data, inference=False):
            return data["answer"], []

    batches = [{"answer": torch.tensor([0, 1]), "qtype": torch.tensor([1, 3]), "vid": list("ab")}]
    opt = types.SimpleNamespace(param_groups=[{"lr": 0.5}])
    with pytest.raises(NotImplementedError):
        engine.val_one_epoch(Stub(), batches, opt, 0, args=types.SimpleNamespace(is_generation_task=False))


def test_cabi_score_entry_points():
    """Both new symbols are exported by both builds at ABI 18 with the signatures of fvqa/_lib.py; argument validation comes
    before any launch, so they can be called without a GPU."""
    assert _lib.ABI_VERSION == 18
    p, i = C.c_void_p, C.c_int
    assert _lib.SIGNATURES["fvqa_attn_suffix"] == (i, [p] * 10 + [i] * 10 + [p])
    assert _lib.SIGNATURES["fvqa_option_pick"] == (i, [p, p, i, p, p, p, p, p, i, i, i, p])
    one = C.c_void_p(256)
    for which, code, other in (("bf16", _lib.BF16, _lib.F16), ("f16", _lib.F16, _lib.BF16)):
        lib = _lib.load(which)
        assert lib.fvqa_version() == 18
        ptrs = [one] * 10
        assert lib.fvqa_attn_suffix(*([None] + ptrs[1:]), 2, 5, 4, 128, 2, 128, 10, 10, 1, code, None) == -1     # null pointer
        assert lib.fvqa_attn_suffix(*ptrs, 2, 5, 4, 128, 2, 128, 10, 10, 1, other, None) == -1     # the other build's type
        assert lib.fvqa_attn_suffix(*ptrs, 2, 5, 17, 128, 2, 128, 10, 10, 1, code, None) == -2     # 17 suffix rows
        assert lib.fvqa_attn_suffix(*ptrs, 2, 5, 4, 4097, 2, 128, 10, 10, 1, code, None) == -2     # S > 4096
        assert lib.fvqa_attn_suffix(*ptrs, 2, 5, 4, 128, 2, 64, 10, 10, 1, _lib.F32, None) == -2   # head_dim != 128
        assert lib.fvqa_attn_suffix(*([C.c_void_p(260)] + ptrs[1:]), 2, 5, 4, 128, 2, 128, 10, 10, 1, code, None) == -3
        assert lib.fvqa_option_pick(None, one, 4, one, one, one, one, one, 2, 5, 128, None) == -1
        assert lib.fvqa_option_pick(one, one, 4, one, one, one, one, one, 2, 65, 128, None) == -2  # > 64 options
        assert lib.fvqa_option_pick(one, one, 4, one, one, one, one, one, 2, 5, 1, None) == -2
