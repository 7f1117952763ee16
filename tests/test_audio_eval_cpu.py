"""MusicAVQA validation bookkeeping (no GPU): the hit rule of the one-option dataset and its question-type meters
(reference engine.py:100-116, util/misc.py:495-524)."""
import types

import pytest
import torch

import engine
from util import misc


def test_log_qtype_musicavqa_groups():
    log = misc.MetricLogger(delimiter="  ")
    data = {"qtype": torch.tensor([1, 6, 11, 5, 15, 15])}     # Audio_Temporal, Visual_Temporal, AV_Temporal, Audio_Counting, 2 x AV_Counting
    hit = torch.tensor([1, 0, 1, 1, 0, 1])
    misc.log_qtype(data, hit, log, types.SimpleNamespace(dataset="musicavqa"))
    got = {k: m.global_avg for k, m in log.meters.items()}
    assert set(got) == set(misc.MUSICAVQA_GROUPS)
    assert got["audio"] == pytest.approx(1.0) and got["visual"] == pytest.approx(0.0)
    assert got["audio_visual"] == pytest.approx(2 / 3) and got["temporal"] == pytest.approx(2 / 3)
    assert got["counting"] == pytest.approx(2 / 3)
    ids = sorted(i for g in ("audio", "visual", "audio_visual") for i in misc.MUSICAVQA_GROUPS[g])
    assert ids == list(range(1, 16)) == sorted(i for g in ("temporal", "existential", "comparative", "location", "counting")
                                                 for i in misc.MUSICAVQA_GROUPS[g])


def test_val_one_epoch_musicavqa_hit_rule(tmp_path):
    class Stub(torch.nn.Module):
        def forward(self, data, inference=False):
            assert inference
            gen = ["two violins", "no", "piano and more", ""]
            return torch.zeros(4, dtype=torch.long), [{"video_id": v, "question": "", "generated_answer": g}
                                                      for v, g in zip(data["vid"], gen)]

    batch = {"answer": torch.zeros(4, dtype=torch.long), "qtype": torch.tensor([5, 2, 11, 14]), "vid": list("abcd"),
             "text": [{"options": [o]} for o in ("two", "yes", "piano", "indoor")]}
    opt = types.SimpleNamespace(param_groups=[{"lr": 0.5}])
    args = types.SimpleNamespace(is_generation_task=True, dataset="musicavqa", debug=False, output_dir=str(tmp_path))
    stats = engine.val_one_epoch(Stub(), [batch], opt, epoch=0, args=args)
    assert stats["acc"] == pytest.approx(0.5)                 # "two violins" and "piano and more" start with the answer
    assert stats["audio"] == pytest.approx(0.5) and stats["audio_visual"] == pytest.approx(0.5)
    assert "Total" not in stats
