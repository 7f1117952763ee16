"""--train_norm, host side (no GPU): the flag, the freeze policy with adapter_layer == and < n_layers, the product model's
parameters against the records of the reference run with its norm weights trainable (tools/gen_golden_norm_train.py), the flat
layout's one contiguous (2L + 1, D) block, the optimizer's groups, the checkpoint's names, and the new C entry points' operand
checks."""
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
from tests import train_norm_util as U


# ------------------------------------------------------------------------------ flag and freeze policy
def test_flag_parses_and_sets_the_model():
    P = train.get_args_parser()
    assert P.parse_args([]).train_norm is False
    a = P.parse_args(["--train_norm"])
    train.validate_args(a)
    assert a.train_norm is True
    cfg = synth.preset("tiny", vaq=True, qav=True)
    assert U.build_model(cfg, device="cpu", train_norm=True, fill=False)[0].train_norm is True
    assert U.build_model(cfg, device="cpu", train_norm=False, fill=False)[0].train_norm is False
    plain, _ = audio_util.build_model(cfg, device="cpu", fill=False)           # args without the attribute
    assert plain.train_norm is False


def test_is_trainable_with_and_without_the_flag():
    walked = [1, 2]                                                            # n_layers 3, adapter_layer 2
    on = ["norm.weight"] + [f"layers.{i}.{m}.weight" for i in walked for m in ("attention_norm", "ffn_norm")]
    unwalked = ["layers.0.attention_norm.weight", "layers.0.ffn_norm.weight"]
    old = ["adapter_query.weight", "visual_proj.weight", "temporal_emb.weight", "layers.0.attention.gate1",
           "layers.2.attention.gate2"]
    frozen = ["tok_embeddings.weight", "layers.1.attention.wq.weight", "layers.2.feed_forward.w2.weight", "output.weight"]
    for n in on:
        assert not synth.is_trainable(n) and not synth.is_trainable(n, False, None) and not synth.is_trainable(n, True)
        assert synth.is_trainable(n, False, walked) and synth.is_trainable(n, train_norm=walked)
    for n in unwalked + frozen:
        assert not synth.is_trainable(n) and not synth.is_trainable(n, False, walked)
    for n in old:
        assert synth.is_trainable(n) and synth.is_trainable(n, False, walked)
    assert synth.is_trainable("audio_proj.weight", True, walked) and not synth.is_trainable("audio_proj.weight", False, walked)
    assert synth.norm_train_names(walked) == ["layers.1.attention_norm.weight", "layers.2.attention_norm.weight",
                                              "layers.1.ffn_norm.weight", "layers.2.ffn_norm.weight", "norm.weight"]


def _records(g):
    return {str(n): (tuple(int(d) for d in str(s).split("x")), bool(t))
            for n, s, t in zip(g["param_names"], g["param_shapes"], g["param_trainable"])}


@pytest.mark.parametrize("name", U.TINY)
def test_model_with_the_flag_trains_what_the_reference_gave_a_gradient(name):
    """The generator unfreezes EVERY norm of the reference; the product trains the ones that received a gradient there — a layer
    the reference never walks left a `gradnone__` record and stays frozen here."""
    g, cfg = audio_util.golden_cfg(name)
    model, _ = U.build_model(cfg, torch.bfloat16, device="cpu", fill=False)
    want = _records(g)
    have = {n: (tuple(p.shape), p.requires_grad) for n, p in model.named_parameters()}
    assert [n for n, _ in model.named_parameters()] == [str(n) for n in g["param_names"]]
    no_grad = {k[len("gradnone__"):].replace("__", ".") for k in g if k.startswith("gradnone__")}
    norms = U.all_norm_names(model)
    assert all(want[n][1] for n in norms)
    for n, (shape, trainable) in want.items():
        assert have[n] == (shape, trainable and not (n in norms and n in no_grad)), n
    trained = U.norm_names(model)
    assert set(trained) == set(norms) - no_grad and len(trained) == 2 * cfg.adapter_layer + 1
    if cfg.adapter_layer < cfg.n_layers:
        assert {n for n in no_grad if n in norms} == {f"layers.{i}.{m}.weight" for i in range(cfg.n_layers - cfg.adapter_layer)
                                                      for m in ("attention_norm", "ffn_norm")}
    else:
        assert not no_grad & set(norms)
    named = dict(model.named_parameters())
    assert all(named[n].dtype == torch.float32 for n in trained)               # fp32 masters whatever the storage type
    assert all(named[n].dtype == torch.bfloat16 for n in set(norms) - set(trained))
    flat = FlatParams(model)
    for k in g:                                                                # every gradient of the reference has a segment
        if k.startswith("gradnorm__"):
            assert k[len("gradnorm__"):].replace("__", ".") in flat.offsets, k


def test_model_without_the_flag_is_the_parent():
    cfg = synth.preset("tiny", n_layers=3, adapter_layer=2, vaq=True, qav=True)
    off, _ = U.build_model(cfg, torch.bfloat16, device="cpu", train_norm=False, fill=False)
    plain, _ = audio_util.build_model(cfg, torch.bfloat16, device="cpu", fill=False)
    sig = lambda m: [(n, tuple(p.shape), p.dtype, p.requires_grad) for n, p in m.named_parameters()]      # noqa: E731
    assert sig(off) == sig(plain)
    assert FlatParams(off).offsets == FlatParams(plain).offsets
    assert not any(n in FlatParams(off).offsets for n in U.all_norm_names(off))


# ------------------------------------------------------------------------------ flat layout
@pytest.mark.parametrize("n_layers,adapter_layer", [(2, 2), (3, 2)])
def test_flat_layout_is_one_contiguous_block(n_layers, adapter_layer):
    cfg = synth.preset("tiny", n_layers=n_layers, adapter_layer=adapter_layer, vaq=True, qav=True)
    D, A, L, F, H = cfg.dim, cfg.adapter_len, cfg.adapter_layer, cfg.max_feats, cfg.n_heads
    model, _ = U.build_model(cfg, torch.bfloat16, device="cpu")
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    flat = FlatParams(model)
    head = A * L * D + D * 768 + F * D                                         # adapter_query | visual_proj | temporal_emb
    names = U.norm_names(model)
    walked = model.engine_layer_ids()
    assert walked == list(range(n_layers))[-adapter_layer:]
    assert names == [f"layers.{i}.attention_norm.weight" for i in walked] + [f"layers.{i}.ffn_norm.weight" for i in walked] + \
        ["norm.weight"]
    assert flat.names[-len(names):] == names
    for r, n in enumerate(names):                                              # row r of the block, then the gates
        assert flat.offsets[n] == (head + r * D, D, (D,)), n
    assert flat.gate_off == head + (2 * L + 1) * D
    total = flat.gate_off + cfg.n_layers * 2 * H
    assert flat.flat.numel() == total and flat.seg_off.tolist() == sorted(v[0] for v in flat.offsets.values()) + [total]
    blk, gblk = flat.norm_block(flat.flat), flat.norm_block(flat.flat_grad)
    assert tuple(blk.shape) == tuple(gblk.shape) == (2 * L + 1, D) and blk.is_contiguous() and blk.data_ptr() % 16 == 0
    assert blk.data_ptr() == flat.flat.data_ptr() + 4 * head and gblk.data_ptr() == flat.flat_grad.data_ptr() + 4 * head
    named = dict(model.named_parameters())
    for r, n in enumerate(names):
        assert named[n].data_ptr() == blk[r].data_ptr() and named[n].grad.data_ptr() == gblk[r].data_ptr()
        assert torch.equal(named[n].detach(), before[n].float())               # the masters start from the model's own weights
        assert float((named[n].detach() - 1).abs().max()) <= 0.1 + 1e-6 and float(named[n].detach().std()) > 0.01
    assert set(flat.offsets) == {n for n, p in named.items() if p.requires_grad}
    # the norms of a layer the engine never walks are outside the buffer, frozen, in the storage type
    for i in range(n_layers - adapter_layer):
        for m in ("attention_norm", "ffn_norm"):
            p = named[f"layers.{i}.{m}.weight"]
            assert not p.requires_grad and p.dtype == torch.bfloat16 and f"layers.{i}.{m}.weight" not in flat.offsets


# ------------------------------------------------------------------------------ optimizer
def test_norm_weights_land_in_the_no_decay_group():
    cfg = synth.preset("tiny", n_layers=3, adapter_layer=2, vaq=True, qav=True)
    model, _ = U.build_model(cfg, device="cpu")
    flat = FlatParams(model)
    named = dict(model.named_parameters())
    no_decay, decay = param_groups_weight_decay(model, 0.1)
    nd, dc = {id(p) for p in no_decay["params"]}, {id(p) for p in decay["params"]}
    names = U.norm_names(model)
    assert all(id(named[n]) in nd and id(named[n]) not in dc for n in names) and len(nd) == len(names) == 5
    assert no_decay["weight_decay"] == 0.0 and decay["weight_decay"] == 0.1
    off_model, _ = U.build_model(cfg, device="cpu", train_norm=False)
    assert param_groups_weight_decay(off_model, 0.1)[0]["params"] == []          # flag off: the parent's groups
    opt = FusedAdamW([no_decay, decay], lr=1e-3, flat=flat)
    b0 = flat.offsets[names[0]][0]
    assert opt._ranges[0] == [(b0, b0 + 5 * cfg.dim)]                           # the block is ONE launch of the no-decay group
    covered = torch.zeros(flat.flat.numel(), dtype=torch.int32)
    for ranges in opt._ranges:
        for lo, hi in ranges:
            covered[lo:hi] += 1
    idle = set(flat.idle_offsets())
    assert int(covered.max()) == 1
    for n, (o, sz, _) in flat.offsets.items():                                  # all but the gates of the unwalked layer
        assert int(covered[o:o + sz].min()) == (0 if o in idle else 1), n
    # moments round-trip through state_dict / load_state_dict, the new segments included
    for i, p in enumerate(flat.params()):
        opt.state[p]["exp_avg"].fill_(float(i + 1))
        opt.state[p]["exp_avg_sq"].fill_(float(i + 1) / 7)
    model2, _ = U.build_model(cfg, device="cpu")
    opt2 = FusedAdamW(param_groups_weight_decay(model2, 0.1), lr=1e-3, flat=FlatParams(model2))
    opt2.load_state_dict(opt.state_dict())
    assert torch.equal(opt2.exp_avg, opt.exp_avg) and torch.equal(opt2.exp_avg_sq, opt.exp_avg_sq)


# ------------------------------------------------------------------------------ checkpoint
def test_checkpoint_names_round_trip(tmp_path):
    cfg = synth.preset("tiny", n_layers=3, adapter_layer=2, vaq=True, qav=True)
    model, _ = U.build_model(cfg, torch.bfloat16, device="cpu")
    FlatParams(model)
    names = U.norm_names(model)
    state = misc.trainable_state(model)
    assert set(state) == {n for n, p in model.named_parameters() if p.requires_grad} and set(names) <= set(state)
    assert all(state[n].dtype == torch.float32 for n in names)
    off_model, _ = U.build_model(cfg, torch.bfloat16, device="cpu", train_norm=False)
    assert not set(U.all_norm_names(off_model)) & set(misc.trainable_state(off_model))      # flag off: the parent's contents
    with torch.no_grad():
        for k, n in enumerate(names):
            state[n] = state[n] + 0.25 * (k + 1)
    torch.save({"model": state}, tmp_path / "ck.pth")
    ns = types.SimpleNamespace(resume=str(tmp_path / "ck.pth"))
    # a run with the flag: the masters come back bit for bit
    on2, _ = U.build_model(cfg, torch.bfloat16, device="cpu", fill=False)
    FlatParams(on2)
    misc.load_model(ns, on2, None, None)
    own = dict(on2.named_parameters())
    assert all(torch.equal(own[n].detach(), state[n]) for n in state)
    # a run WITHOUT the flag takes them as frozen values of the storage type
    other, _ = U.build_model(cfg, torch.bfloat16, device="cpu", train_norm=False, fill=False)
    misc.load_model(ns, other, None, None)
    own = dict(other.named_parameters())
    for n in names:
        assert own[n].dtype == torch.bfloat16 and not own[n].requires_grad
        assert torch.equal(own[n].detach(), state[n].to(torch.bfloat16)), n
    # a run with the flag that loads a checkpoint without them keeps the model's own norm weights as masters
    with_flag, _ = U.build_model(cfg, torch.bfloat16, device="cpu")
    FlatParams(with_flag)
    keep = {n: p.detach().clone() for n, p in with_flag.named_parameters()}
    torch.save({"model": misc.trainable_state(off_model)}, tmp_path / "old.pth")
    misc.load_model(types.SimpleNamespace(resume=str(tmp_path / "old.pth")), with_flag, None, None)
    own = dict(with_flag.named_parameters())
    assert all(torch.equal(own[n].detach(), keep[n]) for n in names)


# ------------------------------------------------------------------------------ C ABI
def test_cabi_train_norm_entry_points():
    """The new symbols are exported by both builds at ABI 18; operands are checked before any launch, so the checks can be called
    without a GPU."""
    assert _lib.ABI_VERSION == 18
    p, i, sz = C.c_void_p, C.c_int, C.c_size_t
    assert _lib.SIGNATURES["fvqa_rmsnorm_dw_workspace"] == (sz, [i, i])
    assert _lib.SIGNATURES["fvqa_rmsnorm_dw"] == (i, [p, p, p, p, p, sz, i, i, i, i, p])
    assert _lib.SIGNATURES["fvqa_layers_bwd_norm"] == (i, [p, p, p, p, p])
    assert _lib.SIGNATURES["fvqa_layers_bwd"] == (i, [p, p, p, p])              # the existing entry keeps its signature
    one, odd, odd4 = C.c_void_p(256), C.c_void_p(264), C.c_void_p(258)
    for which, h16, other in (("bf16", _lib.BF16, _lib.F16), ("f16", _lib.F16, _lib.BF16)):
        lib = _lib.load(which)
        assert lib.fvqa_version() == 18
        ws = lib.fvqa_rmsnorm_dw_workspace
        assert ws(1, 256) == 256 * 4 and ws(16, 256) == 256 * 4 and ws(17, 256) == 2 * 256 * 4
        assert ws(1024, 4096) == 64 * 4096 * 4 and ws(1025, 8192) == 65 * 8192 * 4
        assert ws(0, 256) == 0 and ws(8, 260) == 0 and ws(8, 8200) == 0 and ws(8, 0) == 0
        big = 1 << 30
        ok = (one, one, one, one, one, big, 130, 4096)
        for k in range(5):                                                   # every pointer is needed
            a = list(ok)
            a[k] = None
            assert lib.fvqa_rmsnorm_dw(*a, 1, h16, None) == -1
        assert lib.fvqa_rmsnorm_dw(*ok, 1, other, None) == -1                   # the other build's 16-bit code
        assert lib.fvqa_rmsnorm_dw(*ok, 1, 7, None) == -1
        for rows, dim in ((0, 4096), (-1, 4096), (8, 4100), (8, 8200), (8, 0), (16 * 65535 + 1, 256)):
            assert lib.fvqa_rmsnorm_dw(one, one, one, one, one, big * 8, rows, dim, 1, h16, None) == -2, (rows, dim)
        for k, bad in ((0, odd), (1, odd), (2, odd4), (3, odd4), (4, odd)):     # 16-byte operands, 4-byte rstd and dw
            a = list(ok)
            a[k] = bad
            assert lib.fvqa_rmsnorm_dw(*a, 1, h16, None) == -3, k
        assert lib.fvqa_rmsnorm_dw(one, one, one, one, one, ws(130, 4096) - 1, 130, 4096, 1, h16, None) == -3      # short workspace
        # the schedule entry refuses a null plan, and a plan is checked before the new struct is read
        out = C.c_void_p()
        assert lib.fvqa_layers_bwd_norm(None, one, C.addressof(out), None, None) == -1
        ng = _lib.NormGrads()
        assert lib.fvqa_layers_bwd_norm(None, one, C.addressof(out), C.addressof(ng), None) == -1
    assert [f for f, _ in _lib.NormGrads._fields_] == ["d_an", "d_fn", "d_norm", "dw_ws", "dw_ws_bytes"]


# ------------------------------------------------------------------------------ the model factory
@pytest.mark.parametrize("n_layers", [2, 3])
def test_llama_vqa_freezes_by_the_models_rule(tmp_path, n_layers):
    """llama_vqa.LLaMA_VQA (what train.py builds) with --train_norm: the walked layers' norms and the final norm are trainable
    fp32, an unwalked layer's stay frozen in the storage type; without the flag every norm is frozen as ever."""
    import llama_vqa
    (tmp_path / "tinyX").mkdir()
    (tmp_path / "tinyX" / "params.json").write_text(json.dumps(dict(dim=256, multiple_of=128, n_heads=2, n_layers=n_layers,
                                                                    norm_eps=1e-5, vocab_size=-1)))
    for flag in (True, False):
        a = train.get_args_parser().parse_args(
            ["--llama_model_path", str(tmp_path) + "/", "--model", "tinyX", "--random_init", "--synthetic", "--adapter_layer", "2",
             "--max_seq_len", "32", "--dtype", "bf16"] + (["--train_norm"] if flag else []))
        train.validate_args(a)
        model = llama_vqa.LLaMA_VQA(a).to("cpu")
        assert model.train_norm is flag
        walked = model.engine_layer_ids()
        assert walked == list(range(n_layers))[-2:]
        for n, p in model.named_parameters():
            assert p.requires_grad == synth.is_trainable(n, False, walked if flag else None), n
        named = dict(model.named_parameters())
        for n in U.all_norm_names(model):
            on = flag and n in U.norm_names(model)
            assert named[n].requires_grad is on and named[n].dtype == (torch.float32 if on else torch.bfloat16), n
        groups = param_groups_weight_decay(model, 0.1)
        assert len(groups[0]["params"]) == (5 if flag else 0)
