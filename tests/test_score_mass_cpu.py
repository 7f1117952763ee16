"""Frame attention of option scoring without a GPU: header / binding / export of fvqa_attn_suffix_mass, every refusal of its
operands on the host, `attribution.summarize_options` on hand-made arrays, the plan-shaped zero rows, the refusals of
score_options and of the parser, the reference fixtures (tests/golden/score_mass_*.npz, tools/gen_golden_score_attention.py) as
summaries, and the test helpers' fp64 restatement against oracle/ref_cpu.attn_fwd."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest
import torch

from fvqa import _lib, attribution, ops, score
from tests import cached_attn_util as U
from tests import score_mass_util as MU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A = C.c_void_p(256)
BUILDS = [("bf16", _lib.BF16), ("f16", _lib.F16)]


def _declared_args(name):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fvqa.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, text, flags=re.S)
    assert m, name
    return [a.strip() for a in m.group(1).split(",")]


def test_header_binding_and_export_agree():
    name = "fvqa_attn_suffix_mass"
    res, args = _lib.SIGNATURES[name]
    ctype = lambda d: C.c_void_p if "*" in d else {"int": C.c_int, "float": C.c_float}[d.split()[0]]      # noqa: E731
    assert res is C.c_int and args == [ctype(d) for d in _declared_args(name)]
    for which, _ in BUILDS:
        lib = _lib.load(which)
        assert lib.fvqa_version() == _lib.ABI_VERSION == 18       # entries are only added
        assert callable(getattr(lib, name))
    # fvqa_attn_suffix's argument list plus the summary
    old, new = _declared_args("fvqa_attn_suffix"), _declared_args(name)
    assert len(old) == 21 and new[:21] == old and new[21:] == ["float* mass"]
    assert callable(ops.attn_suffix_mass) and 32 <= ops.SUFFIX_MASS_FEATS
    assert f"max_feats <= {ops.SUFFIX_MASS_FEATS}" in open(os.path.join(ROOT, "include", "fvqa.h")).read()


def _suffix_args(dt, n_seq=3, O=5, T=4, S=128, H=2, Dh=128, A_=10, F=10):
    #       suf cache o g1 g2 vstart start len cos sin | ints | stream mass
    return [A, A, A, A, A, A, A, A, A, A, n_seq, O, T, S, H, Dh, A_, F, 1, dt, None, A]


@pytest.mark.parametrize("which,h16", BUILDS)
def test_the_entry_checks_its_operands_on_the_host(which, h16):
    """Every call here must be refused: one that passed validation would launch a kernel on fake addresses."""
    fn = _lib.load(which).fvqa_attn_suffix_mass
    assert len(_suffix_args(h16)) == len(_lib.SIGNATURES[fn.__name__][1])
    shapes = ((10, 0), (10, 65536), (11, 0), (11, 4097), (12, 0), (12, 17), (13, 0), (13, 4097), (14, 0), (14, 65536), (15, 64),
              (16, -1), (16, 17), (17, -1), (17, ops.SUFFIX_MASS_FEATS + 1))
    for dt in (h16, _lib.F32):
        for at in list(range(10)) + [21]:                     # every pointer is required, the summary's too
            a = _suffix_args(dt)
            a[at] = None
            assert fn(*a) == -1, (dt, at)
        for at, v in shapes:
            a = _suffix_args(dt)
            a[at] = v
            assert fn(*a) == -2, (at, v)
        for at in (0, 1, 2):
            a = _suffix_args(dt)
            a[at] = C.c_void_p(264)
            assert fn(*a) == -3, at
        a = _suffix_args(dt)
        a[21] = C.c_void_p(258)
        assert fn(*a) == -3
    other = _lib.F16 if h16 == _lib.BF16 else _lib.BF16
    assert fn(*_suffix_args(other)) == -1 and fn(*_suffix_args(7)) == -1


def test_the_wrapper_refuses_host_tensors_and_score_options_refuses_before_it_reads_the_batch():
    z = torch.zeros
    i32 = z(1, dtype=torch.int32)
    with pytest.raises(ValueError, match="device"):
        ops.attn_suffix_mass(z(8, 384), z(138, 384), z(8, 128), z(8, 1, 12), z(1), z(1), i32, i32, i32, (z(128, 64), z(128, 64)), 1,
                             2, 4, 128, 1, 128, 10, 10, cache_rotated=True)
    with pytest.raises(ValueError, match="frame_attention is not built for contrast"):
        score.score_options(None, {}, contrast="blind", frame_attention=True)          # no engine, no batch: neither is touched
    with pytest.raises(ValueError, match="frame_attention"):
        attribution.summarize_options({"individual_losses": z(1)})


def _plan(start, length, rows):
    return score.OptionPlan(start=torch.tensor(start), length=torch.tensor(length), T=max(length), shared=True, why_dense="",
                            rows=torch.tensor(rows, dtype=torch.int64).view(-1, 3))


def test_summarize_options_on_hand_made_arrays():
    B, O, T, L, H, F = 2, 3, 4, 2, 2, 3
    g = torch.Generator().manual_seed(0)
    fa = torch.rand(B, O, T, L, H, F + 2, generator=g)
    # sample 0 (start 10): option 0 scores rows 10, 11; option 1 row 12; option 2 none. sample 1 (start 20): option 0 row 23
    rows = [(0, 0, 10), (0, 0, 11), (0, 1, 12), (1, 0, 23)]
    s = attribution.summarize_options({"frame_attention": fa, "plan": _plan([10, 20], [3, 4], rows)})
    want = np.zeros((B, O, F))
    a = fa.numpy().astype(np.float64)
    want[0, 0] = a[0, 0, [0, 1], :, :, :F].mean((0, 1, 2))
    want[0, 1] = a[0, 1, 2, :, :, :F].mean((0, 1))
    want[1, 0] = a[1, 0, 3, :, :, :F].mean((0, 1))
    assert tuple(s["frame_share"].shape) == (B, O, F) and tuple(s["video_mass"].shape) == (B, O)
    assert np.allclose(s["frame_share"].numpy(), want, atol=1e-6) and np.allclose(s["video_mass"].numpy(), want.sum(-1), atol=1e-6)
    assert not bool(s["frame_share"][0, 2].any()) and not bool(s["frame_share"][1, 1:].any())      # no scored row: zeros
    with pytest.raises(ValueError, match="plan.T"):
        attribution.summarize_options({"frame_attention": fa[:, :, :3], "plan": _plan([10, 20], [3, 4], rows)})


def test_plan_shaped_rows():
    """The rows a result covers are the plan's: j < length[n] of every option, at sequence n * O + c and position start[n] + j of
    the dense arena, row-major; everything else of (B, O, T) stays zero."""
    plan = _plan([5, 9, 7], [2, 0, 3], [(0, 0, 5)])
    seq, pos, at = score._suffix_rows(plan, 2)
    assert seq.tolist() == [0, 0, 1, 1, 4, 4, 4, 5, 5, 5] and pos.tolist() == [5, 6, 5, 6, 7, 8, 9, 7, 8, 9]
    assert at.tolist() == [0, 1, 3, 4, 12, 13, 14, 15, 16, 17]
    empty = score._suffix_rows(_plan([5], [0], []), 3)
    assert all(t.numel() == 0 for t in empty)


def test_the_parser_refuses_the_flag_where_no_option_is_scored_once():
    import train
    p = train.get_args_parser()
    assert p.parse_args(["--val_frame_attention"]).val_frame_attention and not p.parse_args([]).val_frame_attention
    for extra in (["--is_generation_task"], ["--contrast", "blind"]):
        with pytest.raises(SystemExit):
            p.parse_args(["--val_frame_attention"] + extra)
    assert p.parse_args([]).log_video_mass == 0 and p.parse_args(["--log_video_mass", "50"]).log_video_mass == 50
    with pytest.raises(SystemExit):
        p.parse_args(["--log_video_mass", "-1"])


@pytest.mark.parametrize("name", MU.FIXTURES)
def test_the_fixtures_are_summaries(name):
    fix = MU.load_fixture(name)
    g = dict(np.load(os.path.join(ROOT, "tests", "golden", f"score_{name}.npz")))
    mass, start, length = fix["mass"], fix["start"], fix["length"]
    B, O, T, L, H, F2 = mass.shape
    plan = score.plan_options(torch.from_numpy(g["text_id_vqa"]), torch.from_numpy(g["label_vqa"]), g["prefix_vqa"].tolist(),
                              g["vstart_vqa"].tolist(), F2 - 2)
    assert plan.shared and plan.start.tolist() == start.tolist() and plan.length.tolist() == length.tolist() and plan.T == T
    live = np.arange(T)[None, :] < length[:, None]
    assert mass.dtype == np.float32 and (mass >= 0).all()
    by_row = mass.transpose(0, 2, 1, 3, 4, 5)                                            # (B, T, O, L, H, F + 2)
    assert np.abs(by_row.sum(-1)[live] - 1).max() < 1e-5
    assert not by_row[~live].any()                                                       # zeros behind length
    # the stored separations are the fixture's own, and rows in front of the first differing token are equal across options
    assert np.allclose(np.nan_to_num(fix["sep_row"]), np.nan_to_num(np.abs(np.diff(mass, axis=2)).max(-1)) * ~np.isnan(fix["sep_row"]))
    assert np.array_equal(fix["sep_option"], np.abs(np.diff(mass, axis=1)).max(-1))
    dead = ~fix["sep_option_live"] & live[:, None, :]
    assert not fix["sep_option"][dead[..., None, None].repeat(L, 3).repeat(H, 4)].any()
    assert not fix["sep_option_live"][:, :, :2].any() and fix["sep_option_live"][:, :, 2:].any()


def test_the_helpers_fp64_summary_is_the_oracles():
    """tests/score_mass_util.case_reference restates the summary from the kernel's operands; here it is held to the text weights
    of oracle/ref_cpu.attn_fwd over the whole sequences of the same case (start edges: every start, len 0, no window)."""
    dtype, rot = torch.float32, True
    c = MU.case("start", dtype, rot)
    want = MU.case_reference("start", dtype, rot)
    N, S, H, O, T, F, D = c["N"], c["S"], c["H"], c["O"], c["T"], c["F"], c["D"]
    valid = c["valid"].view(N, O, T)
    assert float((want.sum(-1)[valid] - 1).abs().max()) < 1e-12 and not bool(want[~valid].any())
    assert bool(valid[:8].all(-1).any()) and not bool(valid[8].any())
    # the oracle: build sample 2's (start 31, window [19, 29)) option sequences from the cache and the suffix rows
    from oracle import ref_cpu
    n, st, vs = 2, int(c["start"][2]), int(c["vstart"][2])
    L = int(valid[n, 0].sum())
    _, _, c64, s64 = U.tables(S)
    full = c["cache"][n * S:(n + 1) * S].clone().view(1, S, 3 * D).repeat(O, 1, 1)
    full[:, st:] = 0
    full[:, st:st + L] = c["suf"].view(N, O, T, 3 * D)[n, :, :L]
    f5 = full.view(O, S, 3, H, U.DH)
    qr = U.rotated_rounded(f5[:, :, 0], c64, s64, dtype)
    kr = U.rotated_rounded(f5[:, :, 1], c64, s64, dtype)
    kr[:, :st] = f5[:, :st, 1].double()                                                # (the cache holds rotated keys)
    ak = c["cache"][N * S:, D:2 * D].double().view(c["A"], H, U.DH)
    av = c["cache"][N * S:, 2 * D:].double().view(c["A"], H, U.DH)
    _, (_, pt) = ref_cpu.attn_fwd(qr, kr, f5[:, :, 2].double(), ak, av, c["g1"].double(), c["g2"].double(), [vs] * O, F)
    for o in range(O):
        for j in range(L):
            p = st + j
            assert float((MU.summary(pt[o, :, p, :p + 1], vs, F, p) - want[n, o, j]).abs().max()) < 1e-12
