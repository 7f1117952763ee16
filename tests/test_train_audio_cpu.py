"""--train_audio, host side (no GPU): the flag, the freeze policy, the product model's parameters against the records of the
reference run with the audio front end trainable (tools/gen_golden_audio_train.py), the flat layout with the flag on and off,
the optimizer's groups and ranges, the checkpoint's contents, and the new C entry points' operand checks."""
import ctypes as C
import json
import types

import pytest
import torch

import train
import util.misc as misc
from fvqa import _lib, synth
from fvqa.optim import FusedAdamW, param_groups_weight_decay
from fvqa.step import FlatParams
from tests import audio_util
from tests import train_audio_util as U

OFF_GOLDEN = {"only": "audio_tiny_only", "sum": "audio_tiny_sum", "attention": "audio_tiny_attn1"}
ON_GOLDEN = {"only": "audio_train_tiny_only", "sum": "audio_train_tiny_sum", "attention": "audio_train_tiny_attn1"}


# ------------------------------------------------------------------------------ flag and freeze policy
def test_flag_parses_and_needs_audio(capsys):
    P = train.get_args_parser()
    assert P.parse_args([]).train_audio is False
    for extra in (["--audio", "--audio_only"], ["--audio", "--audio_merge", "sum"], ["--audio", "--audio_merge", "attention"]):
        a = P.parse_args(extra + ["--train_audio"])
        train.validate_args(a)
        assert a.train_audio is True
    assert "changes nothing" not in capsys.readouterr().out
    with pytest.raises(AssertionError):
        train.validate_args(P.parse_args(["--train_audio"]))


def test_flag_is_a_noop_with_concat(capsys):
    a = train.get_args_parser().parse_args(["--audio", "--audio_merge", "concat", "--train_audio"])
    train.validate_args(a)
    out = capsys.readouterr().out
    assert out.count("\n") == 1 and "--train_audio changes nothing" in out
    cfg = synth.preset("tiny", vaq=True, qav=True, audio="concat")
    on, _ = U.build_model(cfg, device="cpu", train_audio=True)
    off, _ = U.build_model(cfg, device="cpu", train_audio=False)
    assert on.train_audio is False
    assert [(n, p.requires_grad) for n, p in on.named_parameters()] == [(n, p.requires_grad) for n, p in off.named_parameters()]
    assert FlatParams(on).offsets == FlatParams(off).offsets


def test_is_trainable_with_and_without_the_flag():
    audio = ["audio_proj.weight"] + [f"video_audio_cross_attn.{m}.{w}" for m in ("query", "key", "value")
                                     for w in ("weight", "bias")]
    old = ["adapter_query.weight", "visual_proj.weight", "temporal_emb.weight", "layers.3.attention.gate1",
           "layers.0.attention.gate2"]
    frozen = ["tok_embeddings.weight", "layers.0.attention.wq.weight", "norm.weight", "output.weight"]
    for n in audio:
        assert not synth.is_trainable(n) and not synth.is_trainable(n, False) and synth.is_trainable(n, True)
        assert synth.is_trainable(n, train_audio=True)
    for n in old:
        assert synth.is_trainable(n) and synth.is_trainable(n, True)
    for n in frozen:
        assert not synth.is_trainable(n) and not synth.is_trainable(n, True)


# ------------------------------------------------------------------------------ model against the reference's records
def _tiny_cfg(name):
    g, cfg = audio_util.golden_cfg(name)
    if cfg.dim > 1024:                                       # the same mode at a width that builds in no time
        over = {k: v for k, v in json.loads(str(g["case_over"])).items() if k != "batch_size"}
        cfg = synth.preset("tiny", **over)
        g, _ = audio_util.golden_cfg(ON_GOLDEN[cfg.audio])
    return g, cfg


def _records(g):
    return {str(n): (tuple(int(d) for d in str(s).split("x")), bool(t))
            for n, s, t in zip(g["param_names"], g["param_shapes"], g["param_trainable"])}


@pytest.mark.parametrize("name", U.GOLDENS)
def test_model_with_the_flag_equals_the_trainable_reference(name):
    g, cfg = _tiny_cfg(name)
    model, _ = U.build_model(cfg, torch.bfloat16, device="cpu", fill=False)
    want = _records(g)
    have = {n: (tuple(p.shape), p.requires_grad) for n, p in model.named_parameters()}
    assert have == want, set(have.items()) ^ set(want.items())
    assert [n for n, _ in model.named_parameters()] == [str(n) for n in g["param_names"]]
    audio = U.audio_names(model)
    assert audio and all(want[n][1] for n in audio)
    named = dict(model.named_parameters())
    assert all(named[n].dtype == torch.float32 for n in audio)           # fp32 whatever the storage type
    flat = FlatParams(model)
    assert set(flat.offsets) == {n for n, (_, t) in want.items() if t}
    # every gradient the reference produced has a segment to land in
    for k in g:
        if k.startswith("gradnorm__"):
            assert k[len("gradnorm__"):].replace("__", ".") in flat.offsets, k


@pytest.mark.parametrize("mode", sorted(OFF_GOLDEN))
def test_model_without_the_flag_equals_the_existing_records(mode):
    g, cfg = audio_util.golden_cfg(OFF_GOLDEN[mode])
    for kw in (dict(train_audio=False), None):
        if kw is None:
            model, _ = audio_util.build_model(cfg, torch.bfloat16, device="cpu", fill=False)      # args without the attribute
        else:
            model, _ = U.build_model(cfg, torch.bfloat16, device="cpu", fill=False, **kw)
        assert model.train_audio is False
        have = {n: (tuple(p.shape), p.requires_grad) for n, p in model.named_parameters()}
        assert have == _records(g)


# ------------------------------------------------------------------------------ flat layout
@pytest.mark.parametrize("mode,T", U.MODES)
def test_flat_layout_with_and_without_the_flag(mode, T):
    cfg = synth.preset("tiny", vaq=True, qav=True, audio=mode, audio_len=T)
    D, A, L, F, H, E, Ka = cfg.dim, cfg.adapter_len, cfg.adapter_layer, cfg.max_feats, cfg.n_heads, 768, 1024
    head = [("adapter_query.weight", (A * L, D))] + ([("visual_proj.weight", (D, E))] if mode != "only" else []) + \
        [("temporal_emb.weight", (F, D))]
    extra = [("audio_proj.weight", (E if mode == "attention" else D, Ka))]
    if mode == "attention":
        extra += [(f"video_audio_cross_attn.{m}.weight", (E, E)) for m in ("query", "key", "value")]
        extra += [(f"video_audio_cross_attn.{m}.bias", (E,)) for m in ("query", "key", "value")]

    def expect(segs):
        out, off = {}, 0
        for n, shape in segs:
            sz = 1
            for d in shape:
                sz *= d
            out[n] = (off, sz, shape)
            off += sz
        return out, off

    # off: the parent's layout, offsets, segment table and size
    model, _ = U.build_model(cfg, device="cpu", train_audio=False)
    flat = FlatParams(model)
    want, off = expect(head)
    assert {n: flat.offsets[n] for n in want} == want and flat.names == list(want) and flat.gate_off == off
    total = off + cfg.n_layers * 2 * H
    assert flat.flat.numel() == total == flat.flat_grad.numel() and flat.grad_store.numel() == total + 4
    assert len(flat.offsets) == len(want) + 2 * cfg.n_layers
    assert flat.seg_off.tolist() == sorted(v[0] for v in flat.offsets.values()) + [total]
    assert not any(n.startswith(U.AUDIO_PREFIXES) for n in flat.offsets)

    # on: the audio segments follow temporal_emb and precede the gates; q | k | v weights adjacent, the biases adjacent
    model, _ = U.build_model(cfg, device="cpu", train_audio=True)
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    flat = FlatParams(model)
    want, off = expect(head + extra)
    assert {n: flat.offsets[n] for n in want} == want and flat.names == list(want) and flat.gate_off == off
    total = off + cfg.n_layers * 2 * H
    assert flat.flat.numel() == total and flat.seg_off.tolist() == sorted(v[0] for v in flat.offsets.values()) + [total]
    named = dict(model.named_parameters())
    assert set(flat.offsets) == {n for n, p in named.items() if p.requires_grad}
    for n in want:
        o = flat.offsets[n][0]
        assert torch.equal(named[n].detach(), before[n].float()) and named[n].data_ptr() == flat.flat.data_ptr() + 4 * o
        assert named[n].grad.data_ptr() == flat.flat_grad.data_ptr() + 4 * o
        assert o % 4 == 0                                    # 16-byte rows for the kernels' float4 loads
    if mode == "attention":
        parts = ("query", "key", "value")
        w = flat.span([f"video_audio_cross_attn.{m}.weight" for m in parts], flat.flat)
        b = flat.span([f"video_audio_cross_attn.{m}.bias" for m in parts], flat.flat_grad)
        assert tuple(w.shape) == (3 * E, E) and tuple(b.shape) == (3 * E,)
        ca = model.video_audio_cross_attn
        assert w.data_ptr() == ca.query.weight.data_ptr() and w[E:].data_ptr() == ca.key.weight.data_ptr()
        assert w[2 * E:].data_ptr() == ca.value.weight.data_ptr() and b[E:].data_ptr() == ca.key.bias.grad.data_ptr()
        with pytest.raises(ValueError):
            flat.span(["video_audio_cross_attn.query.weight", "video_audio_cross_attn.value.weight"], flat.flat)


# ------------------------------------------------------------------------------ optimizer
def test_biases_land_in_the_no_decay_group_and_ranges_cover_the_segments():
    cfg = synth.preset("tiny", vaq=True, qav=True, audio="attention")
    model, _ = U.build_model(cfg, device="cpu", train_audio=True)
    flat = FlatParams(model)
    named = dict(model.named_parameters())
    no_decay, decay = param_groups_weight_decay(model, 0.1)
    nd, dc = {id(p) for p in no_decay["params"]}, {id(p) for p in decay["params"]}
    for m in ("query", "key", "value"):
        assert id(named[f"video_audio_cross_attn.{m}.bias"]) in nd
        assert id(named[f"video_audio_cross_attn.{m}.weight"]) in dc
    assert id(named["audio_proj.weight"]) in dc
    assert no_decay["weight_decay"] == 0.0 and decay["weight_decay"] == 0.1
    opt = FusedAdamW([no_decay, decay], lr=1e-3, flat=flat)
    covered = torch.zeros(flat.flat.numel(), dtype=torch.int32)
    for ranges in opt._ranges:
        for lo, hi in ranges:
            covered[lo:hi] += 1
    assert int(covered.max()) == 1 and int(covered.min()) == 1          # every element stepped exactly once
    # the three biases are ONE merged range of the no-decay group; everything ahead of them one range of the other, the gates
    # (4-D, decayed as ever) its second
    b0 = flat.offsets["video_audio_cross_attn.query.bias"][0]
    assert opt._ranges[0] == [(b0, b0 + 3 * 768)]
    assert opt._ranges[1] == [(0, b0), (b0 + 3 * 768, flat.flat.numel())]
    # moments round-trip through state_dict / load_state_dict, the new segments included
    for i, p in enumerate(flat.params()):
        opt.state[p]["exp_avg"].fill_(float(i + 1))
        opt.state[p]["exp_avg_sq"].fill_(float(i + 1) / 7)
    sd = opt.state_dict()
    model2, _ = U.build_model(cfg, device="cpu", train_audio=True)
    flat2 = FlatParams(model2)
    opt2 = FusedAdamW(param_groups_weight_decay(model2, 0.1), lr=1e-3, flat=flat2)
    opt2.load_state_dict(sd)
    assert torch.equal(opt2.exp_avg, opt.exp_avg) and torch.equal(opt2.exp_avg_sq, opt.exp_avg_sq)
    o, sz, _ = flat2.offsets["video_audio_cross_attn.key.bias"]
    assert float(opt2.exp_avg[o:o + sz].min()) > 0


# ------------------------------------------------------------------------------ checkpoint
@pytest.mark.parametrize("mode", ["sum", "attention"])
def test_checkpoint_holds_the_audio_tensors_and_loads_without_the_flag(tmp_path, mode):
    cfg = synth.preset("tiny", vaq=True, qav=True, audio=mode)
    model, _ = U.build_model(cfg, device="cpu", train_audio=True)
    audio = U.audio_names(model)
    state = misc.trainable_state(model)
    assert set(state) == {n for n, p in model.named_parameters() if p.requires_grad} and set(audio) <= set(state)
    off_model, _ = U.build_model(cfg, device="cpu", train_audio=False)
    assert not set(audio) & set(misc.trainable_state(off_model))        # flag off: the checkpoint's contents are the parent's
    torch.save({"model": state}, tmp_path / "ck.pth")
    torch.manual_seed(77)
    other, _ = U.build_model(cfg, device="cpu", train_audio=False, fill=False)
    own = dict(other.named_parameters())
    assert not torch.equal(own[audio[0]], state[audio[0]])
    misc.load_model(types.SimpleNamespace(resume=str(tmp_path / "ck.pth")), other, None, None)
    for n in state:
        assert torch.equal(own[n].detach().float(), state[n]), n


# ------------------------------------------------------------------------------ C ABI
def test_cabi_train_audio_entry_points():
    """The three new symbols are exported by both builds at ABI 18; operands are checked before any launch, so the checks can be
    called without a GPU."""
    assert _lib.ABI_VERSION == 18
    p, i, f = C.c_void_p, C.c_int, C.c_float
    assert _lib.SIGNATURES["fvqa_av_cross_attn_bwd"] == (i, [p] * 7 + [i] * 10 + [f, p])
    assert _lib.SIGNATURES["fvqa_av_proj_dx"] == (i, [p, p, p, p, i, i, i, i, i, i, p])
    assert _lib.SIGNATURES["fvqa_av_linear_bwd"] == (i, [p, i, p, i, p, i, i, p])
    one, odd = C.c_void_p(256), C.c_void_p(260)
    for which in ("bf16", "f16"):
        lib = _lib.load(which)
        assert lib.fvqa_version() == 18
        seven = [one] * 7
        ok = (3, 10, 16, 768, 768, 1536, 1536, 768, 1536, 1536)
        assert lib.fvqa_av_cross_attn_bwd(*([None] + seven[1:]), *ok, 0.1, None) == -1
        assert lib.fvqa_av_cross_attn_bwd(*seven, 3, 10, 17, *ok[3:], 0.1, None) == -2            # 17 keys
        assert lib.fvqa_av_cross_attn_bwd(*seven, 3, 10, 16, 768, 764, *ok[5:], 0.1, None) == -2   # pitch below dim
        assert lib.fvqa_av_cross_attn_bwd(*seven, 3, 10, 16, 768, 770, *ok[5:], 0.1, None) == -3   # pitch not 16 bytes
        assert lib.fvqa_av_cross_attn_bwd(*(seven[:4] + [odd] + seven[5:]), *ok, 0.1, None) == -3
        assert lib.fvqa_av_proj_dx(one, None, None, one, 80, 4096, 768, 4096, 768, 768, None) == -1
        assert lib.fvqa_av_proj_dx(one, None, one, one, 80, 4000, 768, 4000, 768, 768, None) == -2  # dim % 64
        assert lib.fvqa_av_proj_dx(one, None, one, one, 80, 4096, 768, 4096, 760, 768, None) == -2  # ldw < k
        assert lib.fvqa_av_proj_dx(one, odd, one, one, 80, 4096, 768, 4096, 768, 768, None) == -3
        src = (_lib.ProjSrc * 1)()
        src[0].x, src[0].w, src[0].ldx, src[0].ldw, src[0].k = 256, 256, 768, 768, 768
        assert lib.fvqa_av_linear_bwd(None, 768, C.addressof(src), 1, None, 80, 768, None) == -1
        assert lib.fvqa_av_linear_bwd(one, 768, C.addressof(src), 0, None, 80, 768, None) == -1     # no source
        assert lib.fvqa_av_linear_bwd(one, 512, C.addressof(src), 1, None, 80, 768, None) == -2     # ldg < dim
        assert lib.fvqa_av_linear_bwd(one, 768, C.addressof(src), 1, odd, 80, 768, None) == -3
        src[0].k = 4096
        src[0].ldx = src[0].ldw = 4096
        assert lib.fvqa_av_linear_bwd(one, 768, C.addressof(src), 1, None, 80, 768, None) == -2     # source wider than 2048


# ------------------------------------------------------------------------------ the model factory
def test_llama_vqa_freezes_by_the_models_rule(tmp_path):
    """llama_vqa.LLaMA_VQA (what train.py builds) with --train_audio: the audio front end is trainable fp32, everything the name
    rule freezes stays frozen; without the flag the audio front end is frozen as ever."""
    import llama_vqa
    (tmp_path / "tinyX").mkdir()
    (tmp_path / "tinyX" / "params.json").write_text(json.dumps(dict(dim=256, multiple_of=128, n_heads=2, n_layers=2,
                                                                    norm_eps=1e-5, vocab_size=-1)))
    for flag in (True, False):
        a = train.get_args_parser().parse_args(
            ["--llama_model_path", str(tmp_path) + "/", "--model", "tinyX", "--random_init", "--synthetic", "--adapter_layer", "2",
             "--max_seq_len", "32", "--audio", "--audio_merge", "attention", "--dtype", "bf16"] + (["--train_audio"] if flag else []))
        train.validate_args(a)
        model = llama_vqa.LLaMA_VQA(a).to("cpu")
        assert model.train_audio is flag
        for n, p in model.named_parameters():
            assert p.requires_grad == synth.is_trainable(n, flag), n
            if n.startswith(U.AUDIO_PREFIXES):
                assert p.requires_grad is flag and p.dtype == torch.float32, n
        groups = param_groups_weight_decay(model, 0.1)
        assert len(groups[0]["params"]) == (3 if flag else 0)              # the three biases, undecayed
