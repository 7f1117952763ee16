"""Host-side refusals of the row, head and optimizer entry points (csrc/rowops.hip, csrc/heads.hip, csrc/optim.hip), without a
GPU: argument validation comes before any launch, so every call here hands the library fake addresses and is turned away — a
null pointer with FVQA_EINVAL (-1), an unsupported shape with FVQA_ESHAPE (-2), a pointer that is not aligned to the widest
access its kernel makes on it with FVQA_EALIGN (-3). Both builds, the 16-bit type of each and fp32.

Every call of this file must be refused: one that passed validation would launch a kernel on the fake addresses."""
import ctypes as C

import pytest

from fvqa import _lib

A = C.c_void_p(256)             # aligned for every access width
M = C.c_void_p(260)             # 4 bytes past it: off the 8-byte (16-bit Vec4, int64) and 16-byte (fp32 Vec4, 8 x 16-bit) boundaries
H = C.c_void_p(258)             # off the 4-byte boundary of an fp32 element

BUILDS = [("bf16", _lib.BF16), ("f16", _lib.F16)]


def _cases(dt):
    """name -> (arguments that only a launch could follow, positions of the required pointers, positions of the pointers a
    kernel reads or writes with 8- or 16-byte accesses, positions of the fp32 pointers read element by element).
    `dt` is the storage dtype code of the call; the stream is the trailing None."""
    return {
        "fvqa_rmsnorm_fwd": ([A, A, A, A, 6, 4096, 1e-6, dt, None], [0, 1, 2], [0, 1, 2], [3]),
        "fvqa_rmsnorm_bwd": ([A, A, A, A, A, A, 6, 4096, dt, None], [0, 1, 2, 3, 5], [0, 1, 2, 4, 5], [3]),
        "fvqa_rope_qk": ([A, A, A, 2, 5, 4, 128, 0, dt, None], [0, 1, 2], [0, 1, 2], []),
        "fvqa_swiglu_fwd": ([A, A, 3, 64, dt, None], [0, 1], [0, 1], []),
        "fvqa_swiglu_bwd": ([A, A, A, 3, 64, dt, None], [0, 1, 2], [0, 1, 2], []),
        "fvqa_embed_splice": ([A, A, A, A, A, A, 2, 16, 64, 4, 3, 1, dt, None], [0, 1, 2, 5], [0, 1, 2, 3, 4, 5], []),
        "fvqa_splice_bwd": ([A, A, A, 2, 16, 64, 4, 3, 1, dt, None], [0, 2], [0, 1, 2], []),
        "fvqa_cast_rows": ([A, A, 3, 64, dt, None], [0, 1], [0, 1], []),
        "fvqa_visual_proj_fwd": ([A, A, A, A, A, 20, 10, 768, 64, dt, None], [0, 1, 2, 3, 4], [0, 1], [2, 3]),
        "fvqa_visual_proj_bwd": ([A, A, A, A, A, 20, 10, 768, 64, None], [0, 2, 3, 4], [2, 3], [0, 1, 4]),
        "fvqa_ce_fwd": ([A, A, A, A, A, 2, 5, 4096, -100, None], [0, 1, 2, 3, 4], [0, 1], [2, 3, 4]),
        "fvqa_ce_bwd": ([A, A, A, A, A, A, 2, 5, 4096, -100, dt, None], [0, 1, 2, 3, 4, 5], [0, 1, 5], [2, 3, 4]),
        "fvqa_qav_head_fwd": ([A, A, A, A, A, A, 2, 9, 64, 10, 0.5, dt, None], [0, 1, 2, 3, 4, 5], [0, 1, 2], [3, 4, 5]),
        "fvqa_qav_head_bwd": ([A, A, A, A, A, A, A, A, 2, 9, 64, 10, 0.5, dt, None], list(range(8)), [0, 1, 2, 6, 7],
                              [3, 4, 5]),
        "fvqa_grad_unscale_norm": ([A, A, 3, A, 1.0, None, None, A, A, A, A, 1 << 20, None], [0, 1, 3, 7, 8, 9, 10], [0, 1],
                                   [3, 6, 7, 8, 9, 10]),
        "fvqa_adamw_step": ([A, A, A, A, 1000, 1e-3, 0.9, 0.95, 1e-8, 0.1, A, None, None], [0, 1, 2, 3, 10], [],
                            [0, 1, 2, 3, 10, 11]),
    }


def _with(args, pos, value):
    out = list(args)
    out[pos] = value
    return out


@pytest.mark.parametrize("which,h16", BUILDS)
def test_null_and_misaligned_pointers_are_refused_on_the_host(which, h16):
    """-1 for every required pointer left null, -3 for every pointer that is off the boundary of its kernel's widest access: 260
    for the pointers read 8 or 16 bytes at a time (`grad` of fvqa_grad_unscale_norm among them: the kernel aligns its 16-byte
    body by element INDEX), 258 for the fp32 operands read one element at a time (every operand of fvqa_adamw_step, which takes
    any slice of the flat buffer)."""
    lib = _lib.load(which)
    assert lib.fvqa_version() == _lib.ABI_VERSION              # (these checks changed no signature and no version)
    for dt in (h16, _lib.F32):
        for name, (args, required, wide, scalar) in _cases(dt).items():
            fn = getattr(lib, name)
            assert len(args) == len(_lib.SIGNATURES[name][1]), name
            for pos in required:
                assert fn(*_with(args, pos, None)) == -1, (name, pos)
            for pos in wide:
                assert fn(*_with(args, pos, M)) == -3, (name, pos)
            for pos in scalar:
                assert fn(*_with(args, pos, H)) == -3, (name, pos)


@pytest.mark.parametrize("which,h16", BUILDS)
def test_unsupported_shapes_are_refused_on_the_host(which, h16):
    lib = _lib.load(which)
    other = _lib.F16 if h16 == _lib.BF16 else _lib.BF16
    for dt in (h16, _lib.F32):
        c = {k: v[0] for k, v in _cases(dt).items()}
        for name in ("fvqa_rmsnorm_fwd", "fvqa_rmsnorm_bwd"):
            dim_at = c[name].index(4096)
            assert getattr(lib, name)(*_with(c[name], dim_at, 4100)) == -2             # dim % 8
            assert getattr(lib, name)(*_with(c[name], dim_at, 8200)) == -2             # dim > 8192
            assert getattr(lib, name)(*_with(c[name], dim_at - 1, 0)) == -2            # no rows
        assert lib.fvqa_rope_qk(*_with(c["fvqa_rope_qk"], 6, 132)) == -2               # head_dim % 8
        assert lib.fvqa_rope_qk(*_with(c["fvqa_rope_qk"], 6, 4)) == -2
        assert lib.fvqa_swiglu_fwd(*_with(c["fvqa_swiglu_fwd"], 3, 72)) == -2          # hidden % 16
        assert lib.fvqa_swiglu_bwd(*_with(c["fvqa_swiglu_bwd"], 4, 72)) == -2
        assert lib.fvqa_cast_rows(*_with(c["fvqa_cast_rows"], 3, 66)) == -2            # dim % 4
        assert lib.fvqa_embed_splice(*_with(c["fvqa_embed_splice"], 8, 66)) == -2      # dim % 4
        assert lib.fvqa_embed_splice(*_with(_with(c["fvqa_embed_splice"], 11, 0), 10, 13)) == -2    # vstart + F > S in mode 0
        assert lib.fvqa_splice_bwd(*_with(c["fvqa_splice_bwd"], 5, 66)) == -2
        assert lib.fvqa_visual_proj_fwd(*_with(c["fvqa_visual_proj_fwd"], 7, 2052)) == -2    # in_dim > 2048
        assert lib.fvqa_visual_proj_fwd(*_with(c["fvqa_visual_proj_fwd"], 7, 770)) == -2     # in_dim % 4
        assert lib.fvqa_visual_proj_bwd(*_with(c["fvqa_visual_proj_bwd"], 7, 2052)) == -2
        assert lib.fvqa_visual_proj_bwd(*_with(c["fvqa_visual_proj_bwd"], 5, 21)) == -2      # rows % max_feats
        assert lib.fvqa_ce_fwd(*_with(c["fvqa_ce_fwd"], 7, 4098)) == -2                # vocab % 4
        assert lib.fvqa_ce_bwd(*_with(c["fvqa_ce_bwd"], 8, 4098)) == -2
        assert lib.fvqa_ce_fwd(*_with(c["fvqa_ce_fwd"], 6, 1)) == -2                   # a row needs a next token
        assert lib.fvqa_qav_head_fwd(*_with(c["fvqa_qav_head_fwd"], 9, 17)) == -2      # max_feats = 17 (FMAX 16)
        assert lib.fvqa_qav_head_bwd(*_with(c["fvqa_qav_head_bwd"], 11, 17)) == -2
        assert lib.fvqa_qav_head_fwd(*_with(c["fvqa_qav_head_fwd"], 8, 66)) == -2      # dim % 4
        assert lib.fvqa_qav_head_bwd(*_with(c["fvqa_qav_head_bwd"], 10, 66)) == -2
        assert lib.fvqa_grad_unscale_norm(*_with(c["fvqa_grad_unscale_norm"], 2, 0)) == -2
        assert lib.fvqa_grad_unscale_norm(*_with(c["fvqa_grad_unscale_norm"], 11, 16)) == -3       # short workspace
        assert lib.fvqa_adamw_step(*_with(c["fvqa_adamw_step"], 4, 0)) == -2
    # the other build's 16-bit code is not this library's
    c = {k: v[0] for k, v in _cases(other).items()}
    for name in ("fvqa_rmsnorm_fwd", "fvqa_rope_qk", "fvqa_swiglu_fwd", "fvqa_cast_rows", "fvqa_embed_splice", "fvqa_ce_bwd",
                 "fvqa_qav_head_fwd", "fvqa_visual_proj_fwd"):
        assert getattr(lib, name)(*c[name]) == -1, name
