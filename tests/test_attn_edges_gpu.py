"""The full-sequence attention of the training path — fvqa_attn_fwd, fvqa_attn_bwd and fvqa_attn_bwd_rotated (csrc/attn_mfma.hip,
and the vector build csrc/attn.hip) — against the fp64 oracle at every edge of their tiles: one figure per (row, head) vector of
128 for o, dq, dk, dv and the adapter rows' dk and dv, max |got - ref| / max(max |ref vector|, 1e-2 max |ref tensor|), held to
the project's own bounds (o 3e-5 / 1e-2, gradients 5e-5 / 2e-2, gate gradients 1e-4 / 3e-2); lse_a and lse_t against the fp64
logsumexp (1e-4, absolute). Every output buffer starts as NaN with a guard row behind it. Inputs and references come from
tests/attn_edges_util.py (planted keys, half plants, decoys), which tests/test_attn_edges_cpu.py checks on the CPU; the rows
whose bound the rounding model sets are named there (MODEL_CLASSES, judge). Figures of a run: profiles/attn_edges.log.
Run with -m gpu -s."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

from fvqa import ops  # noqa: E402
from tests import attn_edges_util as U  # noqa: E402

DEV = "cuda"
DTYPES = U.DTYPES
H16 = [U.BF16, U.F16]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dev(x):
    return x.to(DEV).contiguous()


def poisoned(rows, cols, dtype):
    """rows x cols of NaN (one row when cols is None) and one guard row behind them, in one allocation."""
    full = torch.full((rows + 1, cols) if cols else (rows + U.DH,), U.NAN, dtype=dtype, device=DEV)
    return full, full[:rows]


def guard_kept(full, rows):
    tail = full[rows:].cpu()
    return torch.equal(U.bits(tail), U.bits(torch.full_like(tail, U.NAN)))


class Run:
    """The device side of one case: operands, poisoned outputs, a zeroed workspace. form: None (q, k arrive rotated, or there is
    no RoPE), "fused" (raw q, k and the tables) or "prerotated" (rotated beforehand, the backward un-rotates at its store)."""

    def __init__(self, c, form=None):
        self.c, self.form = c, form
        N, S, H, A = c["N"], c["S"], c["H"], c["A"]
        self.shape = (N, S, H, U.DH, A, c["F"])
        self.qkv = dev(c["qkv"])
        self.tables = (dev(c["cos"]), dev(c["sin"])) if form else None
        if form == "prerotated":
            ops.rope_qk(self.qkv, *self.tables, N, S, H, U.DH)
        self.gates = (dev(c["g1"]), dev(c["g2"]), dev(c["vstart"]))
        self.d_o = dev(c["d_o"])
        self.ws = torch.zeros(ops.attn_bwd_workspace(N, S, H, U.DH, A), dtype=torch.uint8, device=DEV)

    def forward(self):
        c, (N, S, H, _, A, _) = self.c, self.shape
        self.o_full, self.o = poisoned(N * S, c["D"], c["dtype"])
        self.la_full, self.la = poisoned(N * H * S, None, torch.float32)
        self.lt_full, self.lt = poisoned(N * H * S, None, torch.float32)
        ops.attn_fwd(self.qkv, self.o, self.la, self.lt, *self.gates, *self.shape, rope=self.tables if self.form == "fused" else None)
        return self

    def backward(self):
        c, (N, S, H, _, A, _) = self.c, self.shape
        self.dqkv_full, self.dqkv = poisoned(N * S + A, 3 * c["D"], c["dtype"])
        self.dg1, self.dg2 = torch.zeros(H, device=DEV), torch.zeros(H, device=DEV)
        # the backward consumes the forward's own (storage-rounded) o
        ops.attn_bwd(self.d_o, self.qkv, self.o, self.la, self.lt, *self.gates, self.dqkv, self.dg1, self.dg2, self.ws, *self.shape,
                     rope=self.tables if self.form else None, prerotated=self.form == "prerotated")
        return self

    def outputs(self, backward=True):
        c, D = self.c, self.c["D"]
        got = dict(o=self.o.cpu(), lse_a=self.la.cpu(), lse_t=self.lt.cpu())
        if backward:
            g = self.dqkv.cpu()
            R = c["N"] * c["S"]
            got.update(dq=g[:R, :D], dk=g[:, D:2 * D], dv=g[:, 2 * D:], dq_adapter=g[R:, :D], dg1=self.dg1.cpu(), dg2=self.dg2.cpu())
        return got


def check(what, c, run, backward=True, mfma=True):
    """Everything the contract promises about one forward (and backward) of case c: guards, finiteness, lse, per-row figures."""
    got = run.outputs(backward)
    N, S, H, A = c["N"], c["S"], c["H"], c["A"]
    assert guard_kept(run.o_full, N * S) and guard_kept(run.la_full, N * H * S) and guard_kept(run.lt_full, N * H * S), what
    for name in ("lse_a", "lse_t"):
        assert bool(torch.isfinite(got[name]).all()), f"{what}: {name}"
        off = float((got[name].double() - c[name].reshape(-1)).abs().max())
        print(f"{what}: {name} worst {off:.3e} (bound {U.BOUND_LSE:.1e}, absolute)")
        if off >= U.BOUND_LSE:          # the rule of the unmeasured bound: four times the float32 emulation of the same formula
            emu = U.lse_fp32_emulation(c)
            print(f"{what}: {name} in float32 on the CPU {emu:.3e}: bound {4 * emu:.3e}")
            assert off < 4 * emu, f"{what}: {name}"
    if not backward:
        assert bool(torch.isfinite(got["o"].float()).all()), what
        f = float(U.row_figures(got["o"], c["o"].reshape(N * S, -1)).max())
        print(f"{what}: o worst row {f:.3e} (bound {U.BOUND_O[c['dtype']]:.1e})")
        assert f < U.BOUND_O[c["dtype"]], what
        return got
    assert guard_kept(run.dqkv_full, N * S + A), what
    assert not bool(got["dq_adapter"].float().any()), f"{what}: q columns of the adapter rows"
    U.judge(what, c, got, mfma=mfma)
    if A == 1:        # a one-key softmax is constant: the oracle's adapter dk is exactly 0, the kernel's is rounding noise
        assert float(got["dk"][N * S:].float().abs().max()) < 1e-5 * float(c["dk"].abs().max()), what
    return got


def name(dtype):
    return str(dtype).replace("torch.", "")


# ------------------------------------------------------------------------------------------------ 1. length sweep
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("S", U.SWEEP_S)
def test_length_sweep(S, dtype):
    """Both sides of the 16-query wave, the 32-key group, the 64-row vector tile and the 128-row MFMA tile; S = 129 has a
    one-query last block, S >= 160 reaches the mask-free key groups, S = 385 three full tiles and a one-row tile."""
    c = U.sweep_case(dtype, S)
    check(f"sweep S={S} {name(dtype)}", c, Run(c).forward().backward())


# ------------------------------------------------------------------------------------------------ 2. frame window edges
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("A,F", U.AF_PAIRS)
@pytest.mark.parametrize("S", U.WINDOW_S)
def test_frame_window_edges(S, A, F, dtype):
    """The window at position 0, across a 16- and a 32-boundary, across the 128 tile edge and flush with the end, next to a
    sequence without one; S = 128 takes the fused backward, S = 160 the split one."""
    for vs in U.window_vstarts(S, F):
        c = U.window_case(dtype, S, A, F, vs)
        check(f"window S={S} A={A} F={F} vs={vs} {name(dtype)}", c, Run(c).forward().backward())


# ------------------------------------------------------------------------------------------------ 3. planted keys, decoys
@pytest.mark.parametrize("dtype", DTYPES)
def test_planted_keys_and_decoys_forward(dtype):
    """S = 257: key j carries >= 0.99 of query i's softmax for j on both sides of every block, group and tile edge and i = j,
    j + 1, the first row of the next tile and S - 1; score-30 decoys sit on i + 1, on the first key of the next 16-block,
    32-group and tile, and on row 0 of the next sequence."""
    for k, c in enumerate(U.planted_cases(dtype)):
        for (n, i, j, _) in c["pairs"]:
            assert float(c["Pt"][n, :, i, j].min()) >= 0.99
        check(f"planted S={U.PLANT_S} launch {k} {name(dtype)}", c, Run(c).forward(), backward=False)


# ------------------------------------------------------------------------------------------------ 4. half plants, backward
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("S", U.HALF_S)
def test_half_weight_plants_backward(S, dtype):
    """The same (i, j) grid with pairs of weight about one half: dS of the pair is large, so dq[i], dk[j] and dv[j] hang on it."""
    for k, c in enumerate(U.planted_cases(dtype, S, half=True)):
        check(f"half plants S={S} launch {k} {name(dtype)}", c, Run(c).forward().backward())


# ------------------------------------------------------------------------------------------------ 5. RoPE forms
@pytest.mark.parametrize("dtype", H16)
@pytest.mark.parametrize("form", ["fused", "prerotated"])
@pytest.mark.parametrize("S", U.ROPE_S)
def test_rope_forms(S, form, dtype):
    """Raw q, k and the tables, or q, k rotated beforehand and the backward un-rotating at its store: against the oracle on the
    rotated, storage-rounded operands, gradients rotated back."""
    if not ops.attn_rope_fused(dtype):
        pytest.skip("vector attention build selected (FVQA_ATTN_VALU=1)")
    c = U.sweep_case(dtype, S, rope=True)
    check(f"rope {form} sweep S={S} {name(dtype)}", c, Run(c, form).forward().backward())
    for k, c in enumerate(U.planted_cases(dtype, S, half=True, rope=True)):
        check(f"rope {form} half plants S={S} launch {k} {name(dtype)}", c, Run(c, form).forward().backward())


# ------------------------------------------------------------------------------------------------ 6. workspace reuse
@pytest.mark.parametrize("dtype", H16)
@pytest.mark.parametrize("S", [128, 129])
def test_workspace_reuse_and_repeatability(S, dtype):
    """N = 3: forward and backward twice on ONE workspace that is zeroed once — the fused backward's per-head arrival counters
    must be back at zero — with equal bits and both inside the bounds."""
    c = U.reuse_case(dtype, S)
    run = Run(c)
    first = check(f"reuse S={S} first call {name(dtype)}", c, run.forward().backward())
    second = check(f"reuse S={S} second call {name(dtype)}", c, run.forward().backward())
    for t in first:
        assert torch.equal(U.bits(first[t]), U.bits(second[t])), t


# ------------------------------------------------------------------------------------------------ 7. the other builds
def child_main():
    """Runs in a fresh process (the switches are read once per process): bf16, S = 128 and 129, the same per-row check."""
    # (FVQA_ATTN_BWD_SPLIT leaves nothing to query: at S = 128 the split kernels do the fused kernel's arithmetic in the same
    # order, so equal figures are expected; the switch is read in fvqa_attn_bwd_mfma, csrc/attn_mfma.hip)
    valu = os.environ.get("FVQA_ATTN_VALU") == "1"
    assert bool(ops.attn_rope_fused(U.BF16)) != valu
    for S in (128, 129):
        c = U.sweep_case(U.BF16, S)
        check(f"{'vector build' if valu else 'split backward'} S={S} bfloat16", c, Run(c).forward().backward(), mfma=not valu)
    torch.cuda.synchronize()
    print("ok")


@pytest.mark.parametrize("switch", ["FVQA_ATTN_BWD_SPLIT", "FVQA_ATTN_VALU"])
def test_the_other_builds(switch):
    """FVQA_ATTN_BWD_SPLIT=1: the split MFMA backward with a single query tile. FVQA_ATTN_VALU=1: attn_fwd_k<bf16_t> and its
    backward, which no other test runs."""
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "from tests import test_attn_edges_gpu as T\n"
            "T.child_main()\n") % (os.path.join(ROOT, "flipped-vqa_amd"), ROOT)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=dict(os.environ, **{switch: "1"}))
    print(r.stdout, end="")
    assert r.returncode == 0 and r.stdout.rstrip().endswith("ok"), r.stderr[-2000:]
