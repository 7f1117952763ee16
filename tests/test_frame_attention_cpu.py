"""Frame attention without a GPU: header / bindings / exports of fvqa_attn_decode_mass and fvqa_attn_row_mass, every refusal of
their operands on the host, the reference fixture (tests/golden/attn_mass_tiny_peakedperm.npz, tools/gen_golden_attention.py)
against oracle/ref_cpu.attn_fwd — which is pinned to the reference on its own —, `attribution.summarize` against a numpy
restatement, and the parsers' refusals."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest
import torch

from fvqa import _lib, attribution, generate, ops, synth
from oracle import ref_cpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIX = dict(np.load(os.path.join(GOLDEN, "attn_mass_tiny_peakedperm.npz")))
A = C.c_void_p(256)
BUILDS = [("bf16", _lib.BF16), ("f16", _lib.F16)]
N_NEW = 31


# ------------------------------------------------------------------------------------------------ header, bindings, exports
def _declared_args(name):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fvqa.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, text, flags=re.S)
    assert m, name
    return [a.strip() for a in m.group(1).split(",")]


def _ctype_of(decl):
    return C.c_void_p if "*" in decl else {"int": C.c_int, "float": C.c_float}[decl.split()[0]]


@pytest.mark.parametrize("name", ["fvqa_attn_decode_mass", "fvqa_attn_row_mass"])
def test_header_bindings_and_exports_agree(name):
    res, args = _lib.SIGNATURES[name]
    assert res is C.c_int and args == [_ctype_of(d) for d in _declared_args(name)], name
    for which, _ in BUILDS:
        lib = _lib.load(which)
        assert lib.fvqa_version() == _lib.ABI_VERSION == 18       # entries are only added
        assert callable(getattr(lib, name))
    assert callable(ops.attn_decode_mass) and callable(ops.attn_row_mass)
    # the entry the first one extends keeps its declaration, and gains exactly the summary
    old, new = _declared_args("fvqa_attn_decode"), _declared_args("fvqa_attn_decode_mass")
    assert len(old) == 18 and new[:9] == old[:9] and new[9] == "float* mass" and new[10:] == old[9:]


def _decode_args(dt, n_seq=3, S=128, H=2, Dh=128, A_=10, F=10):
    #       row cache o g1 g2 vstart pos cos sin mass
    return [A, A, A, A, A, A, A, A, A, A, n_seq, S, H, Dh, A_, F, 1, dt, None]


def _row_args(dt, R=5, n_seq=3, S=128, H=2, Dh=128, A_=10, F=10):
    #       qkv seq pos g2 vstart cos sin mass
    return [A, A, A, A, A, A, A, A, R, n_seq, S, H, Dh, A_, F, 1, dt, None]


@pytest.mark.parametrize("which,h16", BUILDS)
def test_the_entries_check_their_operands_on_the_host(which, h16):
    """Every call here must be refused: one that passed validation would launch a kernel on fake addresses."""
    lib = _lib.load(which)
    for fn, make, n_ptr, shapes, align16, align4 in (
            (lib.fvqa_attn_decode_mass, _decode_args, 10,
             ((10, 0), (10, 65536), (11, 0), (11, 4097), (12, 0), (12, 65536), (13, 64), (14, -1), (14, 17), (15, -1), (15, 4097)),
             (0, 1, 2), (9,)),
            (lib.fvqa_attn_row_mass, _row_args, 8,
             ((8, 0), (8, 65536), (9, 0), (9, 65536), (10, 0), (10, 4097), (11, 0), (11, 65536), (12, 64), (13, -1), (13, 17),
              (14, -1), (14, 4097)),
             (0,), (1, 2, 7))):
        assert len(make(h16)) == len(_lib.SIGNATURES[fn.__name__][1])
        for dt in (h16, _lib.F32):
            for at in range(n_ptr):                           # every pointer is required
                a = make(dt)
                a[at] = None
                assert fn(*a) == -1, (fn.__name__, dt, at)
            for at, v in shapes:
                a = make(dt)
                a[at] = v
                assert fn(*a) == -2, (fn.__name__, at, v)
            for at in align16:
                a = make(dt)
                a[at] = C.c_void_p(264)
                assert fn(*a) == -3, (fn.__name__, at)
            for at in align4:
                a = make(dt)
                a[at] = C.c_void_p(258)
                assert fn(*a) == -3, (fn.__name__, at)
        other = _lib.F16 if h16 == _lib.BF16 else _lib.BF16
        assert fn(*make(other)) == -1 and fn(*make(7)) == -1   # the other build's 16-bit code; no such code


def test_the_wrappers_refuse_host_tensors_and_generate_refuses_before_it_reads_the_batch():
    z = torch.zeros
    with pytest.raises(ValueError, match="device"):
        ops.attn_row_mass(z(138, 384), z(2, dtype=torch.int32), z(2, dtype=torch.int32), z(2, 1, 12), z(1), z(1, dtype=torch.int32),
                          (z(128, 64), z(128, 64)), 1, 128, 1, 128, 10, 10, cache_rotated=True)
    for kw, word in ((dict(num_beams=2), "num_beams"), (dict(contrast="blind"), "contrast"), (dict(lookahead=4), "lookahead"),
                     (dict(constraints=[[5]], jump_forward=4), "jump_forward")):
        with pytest.raises(ValueError, match="frame_attention is not built for " + word):
            generate.generate(None, {}, frame_attention=True, **kw)
    eng = types.SimpleNamespace(saved=None)
    with pytest.raises(ValueError, match="arena_mass"):
        attribution.arena_mass(eng, 1, 128, [0], [5])
    import inspect
    from fvqa import stream
    assert "frame_attention" in inspect.signature(generate.generate).parameters
    assert "frame_attention" not in inspect.signature(stream.generate_stream).parameters


# ------------------------------------------------------------------------------------------------ the fixture
def test_the_fixture_is_a_summary():
    mass, prefix, vstart = FIX["mass"], FIX["prefix_vqa"], FIX["vstart_vqa"]
    B, T, L, H, F2 = mass.shape
    F = F2 - 2
    assert (B, T, F) == (4, N_NEW, 10) and mass.dtype == np.float32 and (mass >= 0).all()
    assert np.abs(mass.astype(np.float64).sum(-1) - 1).max() < 1e-5
    for b in range(B):
        vs = int(vstart[b])
        for t in range(T):
            p = int(prefix[b]) - 1 + t
            dead = [f for f in range(F) if vs < 0 or vs + f > p]
            assert not mass[b, t, :, :, dead].any()
            if vs < 0:
                assert not mass[b, t, :, :, F].any()
    E = dict(np.load(os.path.join(GOLDEN, "eval_tiny_peakedperm.npz")))       # the batch the fixture was made on
    for k in ("text_id_vqa", "prefix_vqa", "vstart_vqa", "ids_after"):
        assert np.array_equal(E[k], FIX[k]), k
    # neighbouring entries differ by more than m x the build's end-to-end bound in >= 90 % of the pairs: a misplaced summary
    # misses the bound (tools/gen_golden_attention.py BOUNDS; no committed configuration reaches 4 b at the bf16 bound)
    sep = np.concatenate([FIX[k].reshape(-1) for k in ("sep_step", "sep_layer", "sep_head")])
    d = np.abs(np.diff(mass, axis=1)).max(-1)
    assert np.array_equal(FIX["sep_step"], d.astype(np.float32))
    for b, m in ((3e-5, 4), (3.151e-4, 4), (2.051e-3, 1)):
        assert float((sep > m * b).mean()) >= 0.9, (b, m)


def summary_np(P, vs, F, p):
    """P (H, S) one row of text probabilities -> (H, F + 2), from the definition."""
    out = np.zeros((P.shape[0], F + 2), dtype=P.dtype)
    if vs < 0:
        out[:, F + 1] = P[:, :p + 1].sum(-1)
        return out
    for f in range(F):
        if vs + f <= p:
            out[:, f] = P[:, vs + f]
    out[:, F] = P[:, :min(vs, p + 1)].sum(-1)
    out[:, F + 1] = P[:, vs + F:p + 1].sum(-1)
    return out


def test_the_oracle_reproduces_the_fixture():
    """oracle/ref_cpu (RefModel.block_fwd -> attn_fwd, which returns the text probabilities) on the fixture's configuration and
    ids, fp32 on the CPU like the reference run that made the fixture: the same summary within 1e-5."""
    E = dict(np.load(os.path.join(GOLDEN, "eval_tiny_peakedperm.npz")))
    cfg = synth.preset("tiny", vaq=False, qav=False, vocab_size=32000, max_seq_len=128, batch_size=4, peaked_perm=True)
    model = ref_cpu.RefModel(cfg, synth.state_dict(cfg), dtype=torch.float32)
    ids = torch.from_numpy(FIX["ids_after"])
    vs, F = int(FIX["vstart_vqa"][0]), cfg.max_feats
    assert (FIX["vstart_vqa"] == vs).all()
    vf = torch.from_numpy(E["video"]).float() @ model.sd["visual_proj.weight"].T + model.sd["temporal_emb.weight"][None]
    x = model.embed("vqa", ids, None, vf, vs, None)
    worst = 0.0
    for i, li in enumerate(model.layer_ids()):
        x, sv = model.block_fwd(i, li, x, [vs] * ids.shape[0])
        Pt = sv["cache"][1].numpy()                            # (B, H, S, S)
        for b, px in enumerate(FIX["prefix_vqa"]):
            for t in range(N_NEW):
                p = int(px) - 1 + t
                worst = max(worst, float(np.abs(summary_np(Pt[b, :, p], vs, F, p) - FIX["mass"][b, t, i]).max()))
    print(f"oracle against the fixture: {worst:.2e}")
    assert worst < 1e-5


# ------------------------------------------------------------------------------------------------ summarize
def test_summarize_against_numpy():
    rng = np.random.default_rng(3)
    for lead in ((3,), (2, 3)):
        steps, L, H, F = 5, 2, 4, 6
        fa = rng.random(lead + (steps, L, H, F + 2)).astype(np.float32)
        tok = rng.integers(3, 50, lead + (steps,)).astype(np.int32)
        tok[..., 3:] = np.where(rng.random(lead + (2,)) < 0.6, -1, tok[..., 3:])
        tok.reshape(-1, steps)[0] = -1                        # a row without a token: zeros, not 0 / 0
        s = attribution.summarize({"frame_attention": torch.from_numpy(fa), "tokens": torch.from_numpy(tok)})
        want = np.zeros(lead + (F,))
        for at in np.ndindex(*lead):
            live = tok[at] != -1
            if live.any():
                want[at] = fa[at][live][..., :F].astype(np.float64).mean(axis=(0, 1, 2))
        assert tuple(s["frame_share"].shape) == lead + (F,) and tuple(s["video_mass"].shape) == lead
        assert np.allclose(s["frame_share"].numpy(), want, atol=1e-6)
        assert np.allclose(s["video_mass"].numpy(), want.sum(-1), atol=1e-6)
        assert not s["frame_share"].reshape(-1, F)[0].any()
    with pytest.raises(ValueError, match="frame_attention"):
        attribution.summarize({"tokens": torch.zeros(2, 3)})
    with pytest.raises(ValueError, match="tokens"):
        attribution.summarize({"frame_attention": torch.zeros(2, 3, 1, 1, 4), "tokens": torch.zeros(2, 4)})


# ------------------------------------------------------------------------------------------------ parsers, the model
def test_the_parsers_accept_the_flags_and_refuse_what_is_not_built(capsys):
    import answer
    import train
    base = ["--is_generation_task"]
    assert train.get_args_parser().parse_args(base).gen_frame_attention is False
    for how in (["--gen_stop_eos"], ["--gen_constrain", "options"]):
        assert train.get_args_parser().parse_args(base + how + ["--gen_frame_attention"]).gen_frame_attention is True
    with pytest.raises(SystemExit):
        train.get_args_parser().parse_args(base + ["--gen_frame_attention"])
    assert "--gen_stop_eos or --gen_constrain" in capsys.readouterr().err
    for bad in (["--num_beams", "2"], ["--contrast", "blind"], ["--lookahead", "4"],
                ["--gen_constrain", "options", "--gen_jump_forward", "4"], ["--gen_stream", "8"]):
        with pytest.raises(SystemExit):
            train.get_args_parser().parse_args(base + ["--gen_stop_eos", "--gen_frame_attention"] + bad)
        assert "--gen_frame_attention" in capsys.readouterr().err
    q = ["--random_init", "--synthetic", "--question", "why"]
    a = answer.get_args_parser().parse_args(q)
    assert a.frame_attention is False and a.json is None
    a = answer.get_args_parser().parse_args(q + ["--frame_attention", "--json", "out.json", "--temperature", "0.7", "--num_samples", "2"])
    assert a.frame_attention is True and a.json == "out.json"
    for bad in (["--num_beams", "2"], ["--contrast", "blind"], ["--lookahead", "4"],
                ["--options", "a", "b", "--constrain", "--jump_forward", "4"]):
        with pytest.raises(SystemExit):
            answer.get_args_parser().parse_args(q + ["--frame_attention"] + bad)
        assert "--frame_attention" in capsys.readouterr().err


def test_the_model_passes_the_keyword_and_reports_the_summary(monkeypatch):
    import llama.model as LM
    from llama.model import Transformer
    m = types.SimpleNamespace(args=types.SimpleNamespace(gen_frame_attention=True))
    assert LM._frame_attention_kw(m.args) == {"frame_attention": True}
    m.args.gen_frame_attention = False
    assert LM._frame_attention_kw(m.args) == {} and LM._frame_attention_kw(types.SimpleNamespace()) == {}
    fa = torch.zeros(2, 3, 1, 2, 6)
    fa[..., 1] = 0.25
    out = {"frame_attention": fa, "tokens": torch.tensor([[5, 6, -1], [7, -1, -1]], dtype=torch.int32)}
    m.last_generation = {}
    extracted = [{"generated_answer": "a"}, {"generated_answer": "b"}]
    LM._report_frame_attention(m, out, extracted)
    assert set(m.last_generation) == {"frame_attention", "tokens", "frame_share", "video_mass"}
    assert extracted[0]["frame_share"] == [0.0, 0.25, 0.0, 0.0] and extracted[1]["video_mass"] == 0.25
    untouched = [{"generated_answer": "a"}]
    LM._report_frame_attention(m, {}, untouched)
    assert untouched == [{"generated_answer": "a"}]
    m.args = types.SimpleNamespace(gen_frame_attention=True)
    m.ensure_engine = lambda: None
    with pytest.raises(ValueError, match="--gen_stop_eos or --gen_constrain"):
        Transformer.inference(m, {})
    for extra in (dict(num_beams=2), dict(contrast="blind"), dict(lookahead=4), dict(gen_constrain="options", gen_jump_forward=4)):
        m.args = types.SimpleNamespace(gen_frame_attention=True, gen_stop_eos=True, **extra)
        with pytest.raises(ValueError, match="plain token loop"):      # set from code, past the parser: refused, not ignored
            Transformer.inference(m, {})
