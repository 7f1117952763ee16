"""Audio fusion, host side (no GPU): the four modes' parameter containers against the reference's own state-dict records (stored
in the audio goldens by tools/gen_golden_audio.py), the flat trainable buffer per mode, the synthetic generator's defaults, the
MusicAVQA reader + collate against the reference's (tests/golden/audio_loader_musicavqa.npz), and the batch staging."""
import hashlib
import json
import math
import os
import types

import numpy as np
import pytest
import torch

import dataloader
import train
from fvqa import synth
from fvqa.step import FlatParams, audio_mode, stage_batch
from llama import Tokenizer
from oracle.fake_sp import FakeSentencePiece
from tests import audio_util

TASKS = ("vqa", "vaq", "qav")
MODE_GOLDEN = {"only": "audio_tiny_only", "concat": "audio_tiny_concat", "sum": "audio_tiny_sum",
               "attention": "audio_tiny_attn1"}


# ------------------------------------------------------------------------------ model
@pytest.mark.parametrize("name", audio_util.GOLDENS)
def test_modes_construct_with_the_reference_state_dict(name):
    """Names, shapes and requires_grad (after the freeze policy, llama_vqa.py:72) equal the reference's, read from the fixture."""
    g, cfg = audio_util.golden_cfg(name)
    if cfg.dim > 1024:
        cfg = synth.preset("tiny", **{k: v for k, v in json.loads(str(g["case_over"])).items() if k != "batch_size"})
        g, _ = audio_util.golden_cfg(MODE_GOLDEN[cfg.audio])        # (the same mode at a width that builds in no time)
    model, _ = audio_util.build_model(cfg, torch.bfloat16, device="cpu", fill=False)
    want = {str(n): (tuple(int(d) for d in str(s).split("x")), bool(t))
            for n, s, t in zip(g["param_names"], g["param_shapes"], g["param_trainable"])}
    have = {n: (tuple(p.shape), p.requires_grad) for n, p in model.named_parameters()}
    assert have == want, set(have.items()) ^ set(want.items())
    assert set(model.state_dict()) == set(want)
    # frozen front-end weights: fp32 whatever the storage type, nn.Linear's default rule
    for n, p in model.named_parameters():
        if n.startswith(("audio_proj", "video_audio_cross_attn")):
            assert p.dtype == torch.float32 and not p.requires_grad, n
            fan_in = p.shape[-1] if p.dim() == 2 else model.video_audio_cross_attn.query.weight.shape[1]
            assert 0.9 / math.sqrt(fan_in) < float(p.abs().max()) <= 1 / math.sqrt(fan_in), n


def test_frozen_audio_weights_come_from_the_seed():
    cfg = synth.preset("tiny", audio="attention")
    draws = []
    for seed in (5, 5, 6):
        torch.manual_seed(seed)
        m, _ = audio_util.build_model(cfg, device="cpu", fill=False)
        draws.append(torch.cat([m.audio_proj.weight.flatten(), m.video_audio_cross_attn.key.bias]))
    assert torch.equal(draws[0], draws[1]) and not torch.equal(draws[0], draws[2])


def test_audio_mode_decoding():
    ns = types.SimpleNamespace
    assert audio_mode(ns(audio=False, audio_only=False, audio_merge="none")) == "none"
    assert audio_mode(ns()) == "none"
    assert audio_mode(ns(audio=True, audio_only=True, audio_merge=None)) == "only"
    for m in ("concat", "sum", "attention"):
        assert audio_mode(ns(audio=True, audio_only=False, audio_merge=m)) == m
    for bad in ("none", None, "su", "m"):                   # (the reference's `in 'sum'` would take "su" and "m")
        with pytest.raises(ValueError):
            audio_mode(ns(audio=True, audio_only=False, audio_merge=bad))
    a = train.get_args_parser().parse_args(["--audio", "--audio_only"])
    train.validate_args(a)
    assert audio_mode(a) == "only"
    a = train.get_args_parser().parse_args(["--audio", "--audio_merge", "concat"])
    train.validate_args(a)
    assert audio_mode(a) == "concat"


@pytest.mark.parametrize("mode", synth.AUDIO_MODES)
def test_flat_params_layout_per_mode(mode):
    cfg = synth.preset("tiny", vaq=True, qav=True, audio=mode)
    model, _ = audio_util.build_model(cfg, device="cpu")
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    flat = FlatParams(model)
    D, A, L, F, H = cfg.dim, cfg.adapter_len, cfg.adapter_layer, cfg.max_feats, cfg.n_heads
    vp = {"none": 768, "only": 0, "concat": 1792, "sum": 768, "attention": 768}[mode]
    want = [("adapter_query.weight", A * L * D, (A * L, D))]
    if vp:
        want.append(("visual_proj.weight", D * vp, (D, vp)))
    want.append(("temporal_emb.weight", F * D, (F, D)))
    off = 0
    for n, sz, shape in want:
        assert flat.offsets[n] == (off, sz, shape), n
        off += sz
    assert flat.names == [n for n, _, _ in want] and flat.gate_off == off
    assert ("visual_proj.weight" in flat.offsets) == (mode != "only")
    total = off + cfg.n_layers * 2 * H
    assert flat.flat.numel() == total and flat.flat_grad.numel() == total and flat.err_lane.numel() == 1
    assert flat.seg_off.tolist() == sorted(v[0] for v in flat.offsets.values()) + [total]
    named = dict(model.named_parameters())
    trainable = {n for n, p in named.items() if p.requires_grad}
    assert set(flat.offsets) == trainable                   # the frozen audio_proj / cross-attention are not in the buffer
    for n in trainable:                                     # values kept, storage moved, .grad a view of the flat gradient
        o = flat.offsets[n][0]
        assert torch.equal(named[n].detach(), before[n].float()) and named[n].data_ptr() == flat.flat.data_ptr() + 4 * o
        assert named[n].grad.data_ptr() == flat.flat_grad.data_ptr() + 4 * o
    from fvqa.optim import param_groups_weight_decay
    no_decay, decay = param_groups_weight_decay(model, 0.1)
    decayed = {id(p) for p in decay["params"]}
    assert all((id(named[n]) in decayed) == (named[n].ndim > 1) for n in trainable)
    assert len(no_decay["params"]) + len(decay["params"]) == len(trainable)


# ------------------------------------------------------------------------------ synthetic generator
def _digest(tree) -> str:
    h = hashlib.sha256()

    def walk(k, v):
        if torch.is_tensor(v):
            for part in (k, str(v.dtype), str(tuple(v.shape))):
                h.update(part.encode())
            h.update(v.contiguous().numpy().tobytes())
        elif isinstance(v, dict):
            for kk in sorted(v):
                walk(k + "." + kk, v[kk])
        else:
            h.update(k.encode())
            h.update(repr(v).encode())

    for k in sorted(tree):
        walk(k, tree[k])
    return h.hexdigest()


def test_synth_defaults_are_unchanged():
    """The tiny batch and state dict hash to what they did before the audio fields existed (digests taken on the parent
    commit's generator), with the fields left out and with them spelled out at their defaults."""
    for cfg in (synth.preset("tiny"), synth.preset("tiny", audio="none", audio_len=0, audio_dim=1024)):
        assert _digest(synth.make_batch(cfg)) == "1a8450a0d3a8acda2c6a2bcd7f0ff64f9c3abf4cd1cf65ab27034c6071c90b11"
        assert _digest(synth.state_dict(cfg)) == "ddb7002c0af6fc1ba3337a765998327e0168d3a2684de4119c48684cc380b5be"


@pytest.mark.parametrize("mode,T", [("only", 0), ("concat", 0), ("sum", 0), ("attention", 1), ("attention", 0)])
def test_synth_audio_batches(mode, T):
    cfg = synth.preset("tiny", vaq=True, qav=True, audio=mode, audio_len=T)
    b, base = synth.make_batch(cfg, seed=3), synth.make_batch(synth.preset("tiny", vaq=True, qav=True), seed=3)
    assert tuple(b["audio"].shape) == (cfg.batch_size, T or cfg.max_feats, 1024) and b["audio"].dtype == torch.float32
    assert b["audio_len"].tolist() == [T or cfg.max_feats] * cfg.batch_size
    assert ("video" in b) == ("video_len" in b) == (mode != "only")
    for k, v in base.items():                                # everything else is the video-only batch
        if k in ("video", "video_len") and mode == "only":
            continue
        assert _digest({k: b[k]}) == _digest({k: v}), k
    assert not torch.equal(b["audio"][:, :, :768], base["video"][:, : b["audio"].shape[1]])    # its own hash tag
    assert torch.equal(b["audio"], synth.make_batch(cfg, seed=3)["audio"])
    spec = {n: s for n, s, _ in synth.state_spec(cfg)}
    assert ("visual_proj.weight" in spec) == (mode != "only")
    with pytest.raises(ValueError):
        list(synth.state_spec(synth.preset("tiny", audio="mix")))


# ------------------------------------------------------------------------------ MusicAVQA reader + collate
GOLD = dict(np.load(os.path.join(os.path.dirname(__file__), "golden", "audio_loader_musicavqa.npz")))
LOADER_CASES = [("video_train", "train", False, False, "none"), ("video_val", "val", False, False, "none"),
                ("sum_train", "train", True, False, "sum"), ("sum_val", "val", True, False, "sum"),
                ("attention_train", "train", True, False, "attention"), ("only_train", "train", True, True, None)]


@pytest.fixture(scope="module")
def data_root(tmp_path_factory):
    root = tmp_path_factory.mktemp("data")
    items = json.loads(str(GOLD["items_json"]))
    table = [dict(video_id=v, question_content=q, templ_values=tv, type=ty, anser=a) for v, q, tv, ty, a in items]
    base = root / "musicavqa"
    for sub in ("video", "audio_features_imagebind_10_frames/features", "audio_features_imagebind/features"):
        os.makedirs(base / sub)
    for split in ("train", "val"):
        json.dump(table, open(base / f"avqa-{split}.json", "w"))
    feats = {tag: {str(k): torch.from_numpy(GOLD[f"{tag}__{k}"]) for k in GOLD[f"{tag}_names"]}
             for tag in ("video", "audio10", "audio1")}
    torch.save(feats["video"], base / "video" / "clipvitl14.pth")
    torch.save(feats["audio10"], base / "audio_features_imagebind_10_frames" / "features" / "imagebind.pth")
    torch.save(feats["audio1"], base / "audio_features_imagebind" / "features" / "imagebind.pth")
    return str(root)


def make_dataset(data_root, split, audio, audio_only, merge):
    args = types.SimpleNamespace(max_feats=10, max_seq_len=128, dataset="musicavqa", audio=audio, audio_only=audio_only,
                                 audio_merge=merge, debug=False, is_generation_task=False, synthetic=True,
                                 data_root=data_root)
    tok = Tokenizer("/nonexistent/tokenizer.model", args)
    tok.sp_model = FakeSentencePiece()
    return dataloader.dataset_mapping["musicavqa"](args=args, tokenizer=tok, split=split)


@pytest.mark.parametrize("name,split,audio,audio_only,merge", LOADER_CASES)
def test_musicavqa_matches_reference(data_root, name, split, audio, audio_only, merge):
    ds = make_dataset(data_root, split, audio, audio_only, merge)
    assert dataloader.num_options_mapping["musicavqa"] == 1 and len(ds) == GOLD[f"{name}__qtype"].shape[0]
    samples = [ds[i] for i in range(len(ds))]
    assert sorted(samples[0]) == GOLD[f"{name}__sample_keys"].tolist()
    for key in ("text_id", "label", "label_mask", "video_index"):
        for t in TASKS:
            got, ref = torch.stack([s[key][t] for s in samples]).numpy(), GOLD[f"{name}__{key}__{t}"]
            assert got.dtype == ref.dtype and np.array_equal(got, ref), (key, t)
    for key in ("video_start", "prefix_index"):
        for t in TASKS:
            assert [s[key][t] for s in samples] == GOLD[f"{name}__{key}__{t}"].tolist(), (key, t)
    for key in ("video", "audio"):
        assert (key in samples[0]) == (f"{name}__{key}" in GOLD)
        if key in samples[0]:
            got, ref = torch.stack([s[key] for s in samples]).numpy(), GOLD[f"{name}__{key}"]
            assert got.dtype == ref.dtype and np.array_equal(got, ref), key
            assert [s[f"{key}_len"] for s in samples] == GOLD[f"{name}__{key}_len"].tolist()
    assert [s["qtype"] for s in samples] == GOLD[f"{name}__qtype"].tolist()
    assert [s["text"]["q_text"] for s in samples] == GOLD[f"{name}__q_text"].tolist()      # placeholders filled
    b = dataloader.batch_collate(samples[:4])
    assert sorted(b) == GOLD[f"{name}__batch_keys"].tolist()
    for key in ("text_id", "label", "label_mask", "video_index"):
        for t in TASKS:
            ref = GOLD[f"{name}__batch__{key}__{t}"]
            assert b[key][t].numpy().dtype == ref.dtype and np.array_equal(b[key][t].numpy(), ref), (key, t)
    for t in TASKS:
        assert b["video_start"][t] == GOLD[f"{name}__batch__video_start__{t}"].tolist()
    for key in ("video", "video_len", "audio", "audio_len", "answer", "qtype"):
        assert (key in b) == (f"{name}__batch__{key}" in GOLD), key
        if key in b:
            ref = GOLD[f"{name}__batch__{key}"]
            assert b[key].numpy().dtype == ref.dtype and np.array_equal(b[key].numpy(), ref), key


def test_musicavqa_pads_short_audio_with_its_own_width(data_root):
    ds = make_dataset(data_root, "train", True, False, "sum")
    ds.audio_features = {**ds.audio_features, "v3": ds.audio_features["v3"][:4]}
    a, n = ds._get_audio("v3")
    assert tuple(a.shape) == (10, 1024) and n == 4 and float(a[4:].abs().max()) == 0.0
    a, n = ds._get_audio("absent")
    assert tuple(a.shape) == (10, 1024) and n == 1


# ------------------------------------------------------------------------------ staging
def _equal(got, ref):
    assert set(got) >= set(ref)
    for k, v in ref.items():
        if torch.is_tensor(v):
            assert torch.equal(got[k].cpu(), v), k
        elif isinstance(v, dict):
            for t, x in v.items():
                assert torch.equal(got[k][t].cpu(), x) if torch.is_tensor(x) else got[k][t] == x, (k, t)
        else:
            assert got[k] == v, k


@pytest.mark.parametrize("mode", ["only", "concat", "attention"])
def test_producer_and_stage_batch_carry_audio(mode):
    from fvqa.batch_producer import DeviceBatchProducer
    cfg = synth.preset("tiny", vaq=True, qav=True, audio=mode, audio_len=1 if mode == "attention" else 0)
    src = [synth.make_batch(cfg, seed=s) for s in range(4)]
    seen = 0
    for got, ref in zip(DeviceBatchProducer(src, "cpu", depth=2), src):
        _equal(got, ref)
        assert ("video" in got) == (mode != "only") and got["audio"].shape == ref["audio"].shape
        seen += 1
    assert seen == len(src)
    staged = stage_batch(src[0], torch.device("cpu"))
    _equal(staged, src[0])
    assert ("video" in staged) == (mode != "only")


def test_collate_omits_video_for_audio_only_samples():
    s = {"vid": "a", "audio": torch.ones(10, 1024), "audio_len": 10, "text": {}, "qid": 0, "answer": 0, "qtype": 3}
    for key in ("text_id", "label", "video_index", "label_mask"):
        s[key] = {t: torch.zeros(1, 8, dtype=torch.int64) for t in TASKS}
    for key in ("video_start", "prefix_index"):
        s[key] = {t: 2 for t in TASKS}
    b = dataloader.batch_collate([s, s])
    assert "video" not in b and "video_len" not in b
    assert tuple(b["audio"].shape) == (2, 10, 1024) and b["audio_len"].tolist() == [10, 10] and b["audio_len"].dtype == torch.long
