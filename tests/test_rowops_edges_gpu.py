"""The row kernels (csrc/rowops.hip), the loss heads and the visual projection (csrc/heads.hip) and the optimizer
(csrc/optim.hip) on every branch they have: grid-stride second trips, ragged segment ends, the one-pass chunks and the two-pass
loop of the cross entropy, partial lane trips, the row-count and K thresholds between kernels, rows a call must leave alone.

Every reference is fp64 on the CPU (oracle/ref_cpu.py or plain torch) from seeded inputs in storage precision. Errors are
normalised PER ROW (`row_err`), not by the global maximum: a row on a small scale cannot hide behind a large one. Bounds:
`tol(dtype)` = 2e-5 (fp32) / 2e-2 (16-bit storage); 2e-6 for the exact-fp32 projections, 1e-5 for rstd, 1e-2 for a 16-bit RoPE
output (one rounding), as in tests/test_kernels_gpu.py. Where the formula cancels by design the error is held against the
magnitude of what cancels (`cancel_bound`). Every check prints its figure before it asserts (run with -s to read them;
profiles/rowops_edges.log keeps one such run and the mutations that each test was seen to catch)."""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from fvqa import ops  # noqa: E402
from oracle import ref_cpu  # noqa: E402

DEV = "cuda"
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
H16 = [torch.bfloat16, torch.float16]


def tol(dtype, f32=2e-5, h16=2e-2):
    return f32 if dtype == torch.float32 else h16


def rnd(*shape, dtype=torch.float32, scale=1.0, seed=0):
    g = torch.Generator().manual_seed(seed + sum(shape))
    x = (torch.rand(*shape, generator=g, dtype=torch.float64) * 2 - 1) * scale
    return x.to(dtype)            # CPU tensor in storage precision


def dev(x):
    return x.to(DEV).contiguous()


def row_err(got, ref, what="", quantum=0.0):
    """Worst row of max|got - ref| / max|ref|, each row (last dimension; a segment for the optimizer) normalised by ITS OWN
    largest reference magnitude. A row whose reference is all zeros must come back exactly zero (asserted here). A NaN in
    `got` makes the result NaN, which fails every `<` that follows. `quantum`: an absolute rounding step of the OUTPUT FORMAT
    that is taken off every element's error first (fp16 below its smallest normal 6.1e-5 is spaced 2^-24 whatever the value)."""
    got = got.detach().double().cpu()
    ref = ref.detach().double().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    got, ref = got.reshape(-1, got.shape[-1]), ref.reshape(-1, ref.shape[-1])
    den = ref.abs().amax(1)
    zero = den == 0
    assert bool((got[zero] == 0).all()), f"{what}: a row whose reference is all zeros is not exactly zero"
    if bool(zero.all()):
        return 0.0
    err = ((got - ref).abs() - quantum).amax(1)              # (a NaN stays a NaN)
    return float((err[~zero] / den[~zero]).max())


def cancel_bound(z_rows, f32=2e-5):
    """Bound for a quantity whose formula cancels by design — rowloss = lse - z[label], and lse = m + log(sum exp(z - m)) itself:
    the result can be far smaller than the logits it is formed from, so the error is held against the INPUTS' magnitude, per
    row: f32 * max(1, max|z_row|), the maximum over the finite logits of the row (a -inf logit is a legal input)."""
    z = z_rows.double()
    z = torch.where(torch.isfinite(z), z.abs(), torch.zeros_like(z))
    return f32 * z.amax(-1).clamp(min=1.0)


class Checks:
    """Prints every figure before it is judged and fails at the end with all misses, so that one run shows every number."""

    def __init__(self, case):
        self.case, self.bad = case, []

    def lt(self, name, value, bound):
        ok = bool(value < bound)                    # NaN: not ok
        print(f"[edges] {self.case} {name}: {value:.3e} (bound {bound:.1e}){'' if ok else '  MISS'}")
        if not ok:
            self.bad.append((name, value, bound))

    def true(self, name, cond):
        if not bool(cond):
            print(f"[edges] {self.case} {name}: MISS")
            self.bad.append(name)

    def done(self):
        assert not self.bad, (self.case, self.bad)


# ------------------------------------------------------------------------------ SwiGLU, cast
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows,hidden", [(400, 11008), (1, 16)])
def test_swiglu_second_trip_and_saturated_gates(dtype, rows, hidden):
    """400 x 11008 is 1 100 800 four-element vectors against a grid capped at 4096 x 256 = 1 048 576 threads: the last 52 224
    vectors are the second trip of the grid-stride loop (generation prefill and fvqa/score.py run this shape). a = 0, +-20,
    +-100 are planted in the first and the last row: exp(-a) overflows fp32 at a = -100 and the outputs must still be finite
    and right."""
    a, b = rnd(rows, hidden, dtype=dtype, scale=3, seed=1), rnd(rows, hidden, dtype=dtype, scale=3, seed=3)
    dz = rnd(rows, hidden, dtype=dtype, seed=2)
    special = torch.tensor([0.0, 20.0, -20.0, 100.0, -100.0], dtype=dtype)
    for r in {0, rows - 1}:
        a[r, 3:8] = special
        a[r, hidden - 5:] = special
    ab = ops.pack_ab16(a, b)
    z = torch.full((rows, hidden), float("nan"), dtype=dtype, device=DEV)
    ops.swiglu_fwd(dev(ab), z, rows, hidden)
    c = Checks(f"swiglu {dtype} {rows}x{hidden}")
    c.true("z finite", torch.isfinite(z).all())
    c.lt("z", row_err(z, ref_cpu.silu(a.double()) * b.double(), "z"), tol(dtype))
    dab = torch.full((rows, 2 * hidden), float("nan"), dtype=dtype, device=DEV)
    ops.swiglu_bwd(dev(dz), dev(ab), dab, rows, hidden)
    da, db = ref_cpu.swiglu_bwd(dz.double(), a.double(), b.double())
    ga, gb = ops.unpack_ab16(dab)
    c.true("dab finite", torch.isfinite(dab).all())
    c.lt("da", row_err(ga, da, "da"), tol(dtype))
    c.lt("db", row_err(gb, db, "db"), tol(dtype))
    c.done()


def _cast_plants(dtype):
    f = torch.finfo(dtype)
    if dtype == torch.bfloat16:
        ties = [1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), 2.0 ** -126 * (1 + 2.0 ** -8)]
        over = [3.4e38, -3.4e38, torch.finfo(torch.float32).max]           # above bf16's largest finite 3.3895e38
    else:
        ties = [1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, -(1 + 2.0 ** -11), 2.0 ** -24 * 1.5, 2.0 ** -25, 65520.0]
        over = [65536.0, -1e5, 3e38]
    return [0.0, -0.0, 1e-39, -1e-39, 2.0 ** -149, 1e-45, f.max, -f.max, f.tiny, float("inf"), float("-inf"),
            float("nan")] + ties + over


@pytest.mark.parametrize("dtype", H16)
@pytest.mark.parametrize("rows,dim", [(1100, 4096), (1, 4)])
def test_cast_rows_is_the_storage_rounding_bit_for_bit(dtype, rows, dim):
    """fvqa_cast_rows against torch's own fp32 -> 16-bit conversion (round to nearest even, overflow to inf), bitwise; NaNs by
    position. 1100 x 4096 is 1 126 400 vectors, past the 4096 x 256 grid: the plants sit in the first vector, in the second
    trip and in the last vector. Plants: +-0, fp32 subnormals, exact ties of the target format (normal and subnormal), values above
    its largest finite one, +-inf, NaN."""
    src = rnd(rows, dim, scale=4, seed=11)
    plants = torch.tensor(_cast_plants(dtype), dtype=torch.float32)
    flat = src.view(-1)
    if flat.numel() >= 3 * plants.numel():
        flat[: plants.numel()] = plants
        second = 4096 * 256 * 4 + 1001
        flat[second: second + plants.numel()] = plants
        flat[-plants.numel():] = plants
        cases = [src]
    else:                                       # (1, 4): the plants four at a time
        pad = (-plants.numel()) % 4
        cases = list(torch.cat([plants, plants[:pad]]).view(-1, 1, 4))
    for s in cases:
        dst = torch.zeros(s.shape, dtype=dtype, device=DEV)
        ops.cast_rows(dev(s), dst)
        want = s.to(dtype)
        got = dst.cpu()
        nan = torch.isnan(want)
        assert torch.equal(torch.isnan(got), nan)
        gi, wi = got.view(torch.int16), want.view(torch.int16)
        bad = (gi != wi) & ~nan
        assert not bool(bad.any()), (dtype, s[bad][:8], got[bad][:8], want[bad][:8])


# ------------------------------------------------------------------------------ optimizer
ADAM_N = 2 * 2048 * 256 + 3


@functools.lru_cache(maxsize=None)
def _adam_inputs():
    g = torch.Generator().manual_seed(5)
    n = ADAM_N
    sign = lambda: torch.randint(0, 2, (n,), generator=g) * 2.0 - 1.0            # noqa: E731
    p0 = (10.0 ** (torch.rand(n, generator=g, dtype=torch.float64) * 5 - 3) * sign()).float()       # 1e-3 .. 1e2
    g0 = (10.0 ** (torch.rand(n, generator=g, dtype=torch.float64) * 23 - 20) * sign()).float()     # 1e-20 .. 1e3
    g0[torch.rand(n, generator=g) < 0.05] = 0.0
    g0[0] = g0[-1] = 0.0
    g0[1], g0[-2] = 1e-20, 1e3
    return p0, g0


@pytest.mark.parametrize("variant", ["decay", "no_decay", "no_found_inf", "step_9999"])
def test_adamw_second_trip_moments_and_unaligned_view(variant):
    """n = 2 * 2048 * 256 + 3 through the view [1 : n + 1] of a larger buffer (fvqa/optim.py passes such slices): the grid is
    capped at 2048 blocks, so every thread makes a second trip and three make a third. Three steps against torch.optim.AdamW in
    fp64; param, exp_avg and exp_avg_sq are each compared element by element:
      param       |p - ref| <= 2e-5 * (|ref| + lr)
      exp_avg     |m - ref| <= 2e-5 * |ref| + 2^-149
      exp_avg_sq  |v - ref| <= 2e-5 * |ref| + 4 * 2^-149
    The absolute terms are the fp32 FORMAT's: gradients of 1e-20 square to 1e-40, below the smallest normal fp32 (1.2e-38), where
    the spacing is 2^-149 whatever the magnitude; three steps of v = b2 * v + (1 - b2) * g^2 round there three times (product, and
    sum), exp_avg stays normal and needs no more than one such quantum."""
    lr, b1, b2, eps = 0.05, 0.9, 0.95, 1e-8
    wd = 0.0 if variant == "no_decay" else 0.14
    step0 = 9999.0 if variant == "step_9999" else 0.0
    p0, g0 = _adam_inputs()
    n = ADAM_N
    grads = [g0, (g0 * -0.5), (g0 * 2.0)]
    guard = lambda fill: torch.cat([torch.tensor([fill]), torch.zeros(n), torch.tensor([-fill])])        # noqa: E731
    bufs = {k: dev(guard(f)) for k, f in (("p", 11.0), ("g", 13.0), ("m", 17.0), ("v", 19.0))}
    view = {k: t[1:n + 1] for k, t in bufs.items()}
    assert view["p"].data_ptr() % 16 == 4
    view["p"].copy_(p0)
    step = torch.tensor([step0], device=DEV)
    found = None if variant == "no_found_inf" else torch.zeros(1, device=DEV)
    ref_p = torch.nn.Parameter(p0.double().clone())
    opt = torch.optim.AdamW([ref_p], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    opt.state[ref_p] = {"step": torch.tensor(step0, dtype=torch.float64), "exp_avg": torch.zeros(n, dtype=torch.float64),
                        "exp_avg_sq": torch.zeros(n, dtype=torch.float64)}
    for gi in grads:
        ref_p.grad = gi.double()
        opt.step()
        view["g"].copy_(gi)
        ops.adamw_step(view["p"], view["g"], view["m"], view["v"], lr, b1, b2, eps, wd, step, found)
        step += 1.0
    st = opt.state[ref_p]
    assert float(st["step"]) == step0 + 3
    c = Checks(f"adamw {variant}")
    q = 2.0 ** -149

    def worst(got, ref, rel_to, absolute):
        got, ref = got.double().cpu(), ref.detach()
        excess = (got - ref).abs() - absolute
        return float((excess / rel_to).max())

    pr = ref_p.detach()
    c.lt("param", worst(view["p"], pr, pr.abs() + lr, 0.0), 2e-5)
    c.lt("exp_avg", worst(view["m"], st["exp_avg"], st["exp_avg"].abs() + 1e-300, q), 2e-5)
    c.lt("exp_avg_sq", worst(view["v"], st["exp_avg_sq"], st["exp_avg_sq"].abs() + 1e-300, 4 * q), 2e-5)
    zero = g0 == 0
    c.true("zero gradients leave zero moments", (view["m"].cpu()[zero] == 0).all() and (view["v"].cpu()[zero] == 0).all())
    for k, f in (("p", 11.0), ("g", 13.0), ("m", 17.0), ("v", 19.0)):
        c.true(f"guards of {k}", bufs[k][0].item() == f and bufs[k][-1].item() == -f)
    c.done()


SEG_SIZES = [0, 1, 2, 3, 5, 7, 64, 4099, 262147, 300001]
SEG_BODY_TRIP = 256 * 256 * 4          # elements one trip of the 16-byte body covers (NB blocks x 256 threads x 4)


@functools.lru_cache(maxsize=None)
def _seg_case():
    g = torch.Generator().manual_seed(3)
    order = torch.randperm(40, generator=g).tolist()
    sizes = [SEG_SIZES[i % 10] for i in order]                 # every size four times, in a seeded order
    off = [3]
    for s in sizes:
        off.append(off[-1] + s)
    total = off[-1] + 5
    g0 = torch.randn(total, generator=g) * 3
    scaled = g0 * 1024.0                                        # exact: the unscaled gradient is g0 again, bit for bit
    per_sq = torch.stack([(g0[a:b].double() ** 2).sum() for a, b in zip(off[:-1], off[1:])])
    return off, sizes, g0, scaled, per_sq


def _unscale(grad, off):
    n_seg = len(off) - 1
    seg = torch.tensor(off, dtype=torch.int64, device=DEV)
    seg_sq = torch.full((n_seg,), float("nan"), device=DEV)
    found, norm = torch.full((1,), 7.0, device=DEV), torch.full((1,), float("nan"), device=DEV)
    ws = torch.empty(ops.grad_norm_workspace(n_seg), dtype=torch.uint8, device=DEV)
    ops.grad_unscale_norm(grad, seg, torch.tensor([1024.0], device=DEV), seg_sq, found, norm, ws)
    return seg_sq, found, norm


def test_grad_unscale_norm_ragged_segments():
    """40 segments from element 3 on, sizes {0, 1, 2, 3, 5, 7, 64, 4099, 262 147, 300 001} four times each in a seeded order: heads
    and tails off the 16-byte grid, segments too short to hold an aligned body (the scalar fallback), an empty one, bodies longer
    than one trip of 256 blocks (262 144 elements), and more segments than the 16 waves of norm_finish_k. Every seg_sq against
    the fp64 sum of squares of its segment, the norm, every unscaled element, the words around the segments, and bitwise
    repeatability."""
    off, sizes, g0, scaled, per_sq = _seg_case()
    assert sorted(set(sizes)) == SEG_SIZES and off[0] == 3
    bodies = [(a, b) for a, b in zip(off[:-1], off[1:]) if ((a + 3) & ~3) < (b & ~3)]
    assert any(a % 4 for a, _ in bodies) and any(b % 4 for _, b in bodies)                    # ragged heads and tails
    assert any((b & ~3) - ((a + 3) & ~3) > SEG_BODY_TRIP for a, b in bodies)                   # a second body trip
    assert any(a < b and ((a + 3) & ~3) >= (b & ~3) for a, b in zip(off[:-1], off[1:]))        # the scalar fallback
    grad = dev(scaled)
    seg_sq, found, norm = _unscale(grad, off)
    c = Checks("grad_unscale_norm")
    c.true("found_inf == 0", found.item() == 0.0)
    sq = seg_sq.double().cpu()
    empty = per_sq == 0
    c.true("empty segments sum to exactly 0", (sq[empty] == 0).all() and int(empty.sum()) == 4)
    c.lt("seg_sq", float(((sq - per_sq).abs()[~empty] / per_sq[~empty]).max()), tol(torch.float32))
    want = per_sq.sum().sqrt().item()
    c.lt("norm", abs(norm.item() - want) / want, 1e-6)
    got = grad.cpu()
    c.true("outside words untouched", torch.equal(got[:3], scaled[:3]) and torch.equal(got[off[-1]:], scaled[off[-1]:]))
    worst = 0.0
    for a, b in zip(off[:-1], off[1:]):
        if b > a:
            worst = max(worst, row_err(got[a:b][None], g0[a:b][None], "unscaled"))
    c.lt("unscaled elements, per segment", worst, tol(torch.float32))
    c.true("unscaled elements exact (power-of-two scale)", torch.equal(got[3:off[-1]], g0[3:off[-1]]))
    seg_sq2, _, norm2 = _unscale(dev(scaled), off)
    c.true("bitwise repeatable", torch.equal(seg_sq, seg_sq2) and torch.equal(norm, norm2))
    c.done()


@pytest.mark.parametrize("where", ["ragged_head", "ragged_tail", "second_body_trip", "one_element_segment"])
@pytest.mark.parametrize("value", [float("inf"), float("nan")])
def test_grad_unscale_norm_sees_a_non_finite_gradient_everywhere(where, value):
    off, sizes, g0, scaled, _ = _seg_case()
    segs = list(zip(off[:-1], off[1:]))
    body = lambda a, b: ((a + 3) & ~3, b & ~3)                 # noqa: E731
    if where == "ragged_head":
        at = next(a for a, b in segs if a % 4 and body(a, b)[0] < body(a, b)[1])
    elif where == "ragged_tail":
        at = next(b - 1 for a, b in segs if b % 4 and body(a, b)[0] < body(a, b)[1])
    elif where == "second_body_trip":
        at = next(body(a, b)[0] + SEG_BODY_TRIP + 1 for a, b in segs if body(a, b)[1] - body(a, b)[0] > SEG_BODY_TRIP + 4)
    else:
        at = next(a for a, b in segs if b - a == 1)
    assert off[0] <= at < off[-1]
    grad = scaled.clone()
    grad[at] = value
    _, found, _ = _unscale(dev(grad), off)
    assert found.item() == 1.0, (where, value, at)


# ------------------------------------------------------------------------------ cross entropy
CE_V = [4, 4096, 4100, 32000, 32768, 32772]          # one chunk; chunk 0 full; a partial chunk 1; 7 chunks + a partial one; all 8; two-pass


@functools.lru_cache(maxsize=None)
def _ce_case(V):
    B, S = 2, 5
    logits = rnd(B * S, V, scale=30, seed=1).double()
    shift = torch.tensor([50.0, -50.0, 12.5, -31.0, 0.0, 44.0, -7.0, 50.0, -50.0, 3.0], dtype=torch.float64)
    logits = logits + shift[:, None]
    g = torch.Generator().manual_seed(V)
    labels = torch.randint(1, V, (B, S), generator=g)
    labels[0] = torch.tensor([1, 0, V - 1, V, -5])      # rows 0..3 are scored by labels[0, 1:]: 0, V - 1, V (out of range), -5
    labels[1, 1] = -100                                  # row 5
    labels[1, 2] = 0                                     # row 6: scored unless ignore_index = 0
    logits[0, 0] = 95.0                                  # the maximum at column 0 (row 0, whose label is 0: rowloss ~ 0)
    logits[6, V - 1] = 99.0                              # ... and at the last column
    logits[1, V - 1] += 20.0                             # row 1, label V - 1, a likely label
    inf_col = 2
    if labels[1, 4] == inf_col:
        labels[1, 4] = inf_col + 1
    logits[8, inf_col] = float("-inf")                   # a masked logit off the label of row 8
    return B, S, logits.float(), labels


def _ce_reference(logits, labels, B, S, V, ignore):
    z = logits.double().view(B, S, V)
    lab = torch.full((B, S), ignore, dtype=torch.int64)
    lab[:, :-1] = labels[:, 1:]
    scored = ((lab != ignore) & (lab >= 0) & (lab < V)).flatten()
    lse = torch.logsumexp(z.view(-1, V), -1)
    picked = z.view(-1, V).gather(1, lab.flatten().clamp(0, V - 1)[:, None])[:, 0]
    return scored, lab.flatten(), torch.where(scored, lse, torch.zeros_like(lse)), \
        torch.where(scored, lse - picked, torch.zeros_like(lse))


@pytest.mark.parametrize("ignore", [-100, 0])
@pytest.mark.parametrize("V", CE_V)
def test_cross_entropy_every_chunk_and_the_two_pass_path(V, ignore):
    """lse and rowloss of every row (fvqa/score.py reads them row by row), the accumulated loss_sum (documented `+=`) and the
    count. Logits are +-30 around a per-row shift of up to +-50 (|z| reaches 100: one fp32 ulp of such a logit is 7.6e-6, so the
    bound for lse and rowloss is the input-relative `cancel_bound`). Labels V and -5 are not classes: the kernel states that it
    leaves such rows unscored, and they must come back as exact zeros like the ignored ones."""
    B, S, logits, labels = _ce_case(V)
    scored, _, lse_r, loss_r = _ce_reference(logits, labels, B, S, V, ignore)
    lse = torch.full((B * S,), float("nan"), device=DEV)
    rowloss = torch.full((B * S,), float("nan"), device=DEV)
    old = (7.5, 3.0)
    loss_sum = torch.tensor(old, device=DEV)
    ops.ce_fwd(dev(logits), dev(labels), lse, rowloss, loss_sum, B, S, V, ignore)
    c = Checks(f"ce_fwd V={V} ignore={ignore}")
    bound = cancel_bound(logits)
    gl, gr = lse.double().cpu(), rowloss.double().cpu()
    c.true("unscored rows are exact zeros", (gl[~scored] == 0).all() and (gr[~scored] == 0).all())
    c.true("scored rows", int(scored.sum()) == (5 if ignore == -100 else 3))
    c.lt("lse / bound", float(((gl - lse_r).abs() / bound)[scored].max()), 1.0)
    c.lt("rowloss / bound", float(((gr - loss_r).abs() / bound)[scored].max()), 1.0)
    n = int(scored.sum())
    c.true("count", loss_sum[1].item() == old[1] + n)
    c.lt("loss_sum[0] = old + new, / bound", abs(loss_sum[0].item() - (old[0] + loss_r.sum().item())) / float(bound[scored].sum()), 1.0)
    mean = (loss_sum[0].item() - old[0]) / (loss_sum[1].item() - old[1])
    c.lt("mean / bound", abs(mean - loss_r.sum().item() / n) / float(bound[scored].max()), 1.0)
    c.done()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("V", CE_V)
def test_cross_entropy_backward_rows(dtype, V):
    """dlogits = (softmax - onehot) * gscale / count per scored row, exact zeros on every other row of a NaN-filled buffer. The
    label column is p - 1, which cancels when the label is likely (row 0 holds nearly all of its mass there): it is held against its inputs, k = gscale
    / count; the other columns per row against the row's own largest entry. Each scored row sums to 0 within the same k-relative
    bound."""
    ignore, gscale = -100, 2.5
    B, S, logits, labels = _ce_case(V)
    scored, lab, _, _ = _ce_reference(logits, labels, B, S, V, ignore)
    lse = torch.empty(B * S, device=DEV)
    rowloss = torch.empty(B * S, device=DEV)
    loss_sum = torch.zeros(2, device=DEV)
    ops.ce_fwd(dev(logits), dev(labels), lse, rowloss, loss_sum, B, S, V, ignore)
    dlog = torch.full((B * S, V), float("nan"), dtype=dtype, device=DEV)
    ops.ce_bwd(dev(logits), dev(labels), lse, loss_sum, torch.tensor([gscale], device=DEV), dlog, B, S, V, ignore)
    k = gscale / int(scored.sum())
    want = torch.softmax(logits.double(), -1)
    rows = torch.arange(B * S)
    onehot = torch.zeros_like(want)
    onehot[rows[scored], lab[scored]] = 1.0
    want = (want - onehot) * k * scored[:, None]
    got = dlog.double().cpu()
    c = Checks(f"ce_bwd {dtype} V={V}")
    c.true("unscored rows are exact zeros", (got[~scored] == 0).all())
    at = (rows[scored], lab[scored])
    c.lt("label column / k", float((got[at] - want[at]).abs().max()) / k, tol(dtype))
    off_g, off_w = got.clone(), want.clone()
    off_g[at] = 0.0
    off_w[at] = 0.0
    # fp16 dlogits: k * p of an unlikely class lies below fp16's smallest normal, where the format rounds to multiples of 2^-24
    # (the fp16 step runs under a loss scale for this reason); the error of one such rounding is at most half a step
    quantum = 2.0 ** -25 if dtype == torch.float16 else 0.0
    c.lt("other columns, per row", row_err(off_g[scored], off_w[scored], "dlogits", quantum), tol(dtype))
    c.lt("row sums / k", float(got[scored].sum(-1).abs().max()) / k, tol(dtype))
    c.done()


# ------------------------------------------------------------------------------ QAV head
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("F,D,tau", [(1, 4, 100.0), (10, 260, 0.05), (16, 4096, 100.0)])
def test_qav_head_frame_counts_and_lane_trips(dtype, F, D, tau):
    """F = 1, 10 and 16 (FMAX); D = 4 (one lane), 260 (a second lane trip of one lane), 4096. probs and rowloss of every scored row,
    dxn per row (exact zeros on unscored rows of a NaN-filled buffer), d_raw on top of a base. A label equal to F is not a frame
    and leaves its row unscored. tau = 0.05 takes the logits into the hundreds: softmax = exp(z - lse) and rowloss = lse - z[label]
    cancel there, so probs, rowloss and what is formed from probs (dxn, d_raw) are held against the logits' magnitude
    (`cancel_bound`, scaled to tol(dtype) for the 16-bit outputs); at the product's tau = 100 |z| stays near 1 and that is the plain
    bound."""
    B, S = 3, 9
    xn = rnd(B * S, D, dtype=dtype, seed=1)
    vf = rnd(B * F, D, scale=3, seed=2)
    if tau < 1:          # frames that differ a little around a common direction per sample: large logits, a softmax that is not one-hot
        vf = (rnd(B, 1, D, seed=4).double() + 0.01 * rnd(B, F, D, seed=2).double()).reshape(B * F, D).float()
    labels = torch.full((B, S), -1, dtype=torch.int64)
    for b in range(B):
        for j, s in enumerate(range(1 + b, 6 + b)):                # five labelled positions per sample
            labels[b, s] = (j * 7 + b) % F
    labels[1, 3] = F                                               # not a frame: unscored
    labels[2, 0] = F - 1                                           # position 0 labels no row
    probs = torch.full((B * S * F,), float("nan"), device=DEV)
    rowloss = torch.full((B * S,), float("nan"), device=DEV)
    loss_sum = torch.zeros(2, device=DEV)
    ops.qav_head_fwd(dev(xn), dev(vf), dev(labels), probs, rowloss, loss_sum, B, S, D, F, tau)
    x64, v64 = xn.double().view(B, S, D), vf.double().view(B, F, D)
    z = torch.einsum("nsd,nfd->nsf", x64, v64).reshape(B * S, F) / tau
    lab = torch.full((B, S), -1, dtype=torch.int64)
    lab[:, :-1] = labels[:, 1:]
    lab = lab.flatten()
    scored = (lab >= 0) & (lab < F)
    assert int(scored.sum()) == 14
    p_ref = torch.softmax(z, -1)
    loss_ref = torch.logsumexp(z, -1) - z.gather(1, lab.clamp(0, F - 1)[:, None])[:, 0]
    scale = cancel_bound(z, 1.0)                                   # max(1, max|z_row|)
    c = Checks(f"qav {dtype} F={F} D={D} tau={tau}")
    print(f"[edges] {c.case} max|z| {float(z.abs().max()):.1f}")
    gp, gr = probs.view(B * S, F).double().cpu(), rowloss.double().cpu()
    c.true("rowloss of unscored rows is 0", (gr[~scored] == 0).all())
    c.true("count", loss_sum[1].item() == 14)
    ftol = tol(torch.float32)
    c.lt("probs per row / max(1,|z|)", max(row_err(gp[i][None], p_ref[i][None], "probs") / float(scale[i])
                                           for i in torch.nonzero(scored).flatten().tolist()), ftol)
    c.lt("rowloss / max(1,|z|)", float(((gr - loss_ref).abs() / scale)[scored].max()), ftol)
    c.lt("mean / max(1,|z|)", abs(loss_sum[0].item() / 14 - float(loss_ref[scored].mean())) / float(scale[scored].max()), ftol)
    gs = 0.5
    dxn = torch.full((B * S, D), float("nan"), dtype=dtype, device=DEV)
    base = rnd(B * F, D, scale=1e-2, seed=8)
    d_raw = dev(base)
    ops.qav_head_bwd(dev(xn), dev(vf), dev(labels), probs, loss_sum, torch.tensor([gs], device=DEV), dxn, d_raw, B, S, D, F, tau)
    onehot = torch.zeros_like(p_ref)
    idx = torch.nonzero(scored).flatten()
    onehot[idx, lab[idx]] = 1.0
    dl = ((p_ref - onehot) * (gs / 14 / tau) * scored[:, None]).view(B, S, F)
    want_x = torch.einsum("nsf,nfd->nsd", dl, v64).reshape(B * S, D)
    want_v = torch.einsum("nsf,nsd->nfd", dl, x64).reshape(B * F, D) + base.double()
    gx = dxn.double().cpu()
    c.true("dxn of unscored rows is exact zeros", (gx[~scored] == 0).all())
    if F == 1:                                # one frame: probs = 1 exactly, dl = 0: every gradient is exactly zero
        c.true("F = 1: dxn == 0 and d_raw == base", (gx == 0).all() and torch.equal(d_raw.cpu(), base))
    else:
        # a row of dxn is sum_f dl[f] * vf[f]: the error of dl (a probability's, times k) against the row's own dl, per row
        zmax = float(scale[scored].max())
        c.lt("dxn per row / max(1,|z|)", row_err(gx[scored], want_x[scored], "dxn") / zmax, tol(dtype, 1e-5, 1e-2))
        c.lt("d_raw per row / max(1,|z|)", row_err(d_raw, want_v, "d_raw") / zmax, 1e-5)
    c.done()


# ------------------------------------------------------------------------------ RMSNorm, RoPE
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dim", [8, 2048, 2056, 8192])
def test_rmsnorm_row_scales_and_rows_argument(dtype, dim):
    """dim = 8 (one thread), 2048 (chunk 0 full), 2056 (one thread in chunk 1), 8192 (all four chunks). Six rows of a nine-row buffer
    through `rows=6`, as every production call passes it: rows 6-8 of y, rstd and dx keep their sentinels. Row scales 1, 1e-4 (eps =
    1e-6 dominates the mean square), 1e3, an all-zero row (rstd = 1 / sqrt(eps), y = 0, dx = rstd * g * w + resid), 1 and 0.03; each
    row is judged against its own magnitude."""
    eps, R, live = 1e-6, 9, 6
    scales = torch.tensor([1.0, 1e-4, 1e3, 0.0, 1.0, 0.03, 1.0, 1.0, 1.0], dtype=torch.float64)
    x = (rnd(R, dim, seed=1).double() * scales[:, None]).to(dtype)
    w = (rnd(dim, scale=0.1, seed=2).float() + 1).to(dtype)
    g, res = rnd(R, dim, dtype=dtype, seed=3), rnd(R, dim, dtype=dtype, seed=4)
    yr, rr = ref_cpu.rmsnorm_fwd(x.double()[:live], w.double(), eps)
    c = Checks(f"rmsnorm {dtype} dim={dim}")
    y = torch.full((R, dim), 7.0, dtype=dtype, device=DEV)
    rstd = torch.full((R,), -3.0, device=DEV)
    ops.rmsnorm_fwd(dev(x), dev(w), y, rstd, eps, rows=live)
    c.true("rows past `rows` untouched (y, rstd)", (y[live:] == 7.0).all() and (rstd[live:] == -3.0).all())
    c.lt("y per row", row_err(y[:live], yr, "y"), tol(dtype))
    c.lt("rstd per element", float(((rstd[:live].double().cpu() - rr[:, 0]).abs() / rr[:, 0]).max()), 1e-5)
    c.lt("rstd of the zero row", abs(rstd[3].item() - 1 / math.sqrt(eps)) * math.sqrt(eps), 1e-5)
    y2 = torch.full((R, dim), 7.0, dtype=dtype, device=DEV)
    ops.rmsnorm_fwd(dev(x), dev(w), y2, None, eps, rows=live)
    c.true("rstd=None gives the same y", torch.equal(y2, y))
    dxr = ref_cpu.rmsnorm_bwd(g.double()[:live], x.double()[:live], w.double(), rr)
    for resid in (res, None):
        dx = torch.full((R, dim), 7.0, dtype=dtype, device=DEV)
        ops.rmsnorm_bwd(dev(g), dev(x), dev(w), rstd, dx, resid=None if resid is None else dev(resid), rows=live)
        want = dxr if resid is None else dxr + resid.double()[:live]
        name = "dx" if resid is None else "dx + resid"
        c.true(f"rows past `rows` untouched ({name})", (dx[live:] == 7.0).all())
        c.lt(f"{name} per row", row_err(dx[:live], want, name), tol(dtype))
    c.done()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("H,Dh", [(9, 128), (2, 64), (1, 8)])
def test_rope_head_dims_second_trip_and_inverse(dtype, inverse, H, Dh):
    """H = 9, Dh = 128: q | k is 2304 columns, past the 2048 a workgroup covers per trip. Dh = 64 and 8 are the other table
    widths. Forward and inverse against ref_cpu.rope_apply per row in all three storage types; v and the appended adapter rows
    must be bitwise untouched."""
    N, S, A = 2, 5, 3
    D = H * Dh
    qkv = rnd(N * S + A, 3 * D, dtype=dtype, seed=9)
    cos, sin = ref_cpu.rope_tables(16, Dh, torch.float32)          # a table longer than S
    buf = dev(qkv)
    ops.rope_qk(buf, dev(cos), dev(sin), N, S, H, Dh, inverse=inverse)
    got = buf.cpu()
    c = Checks(f"rope {dtype} H={H} Dh={Dh} inverse={inverse}")
    for name, lo in (("q", 0), ("k", D)):
        t = qkv[: N * S, lo:lo + D].double().view(N, S, H, Dh)
        want = ref_cpu.rope_apply(t, cos[:S].double(), sin[:S].double(), inverse=inverse).reshape(N * S, D)
        c.lt(f"{name} per row", row_err(got[: N * S, lo:lo + D], want, name), tol(dtype, h16=1e-2))
    as_int = lambda t: t.contiguous().view(torch.int32 if dtype == torch.float32 else torch.int16)       # noqa: E731
    c.true("v untouched", torch.equal(as_int(got[: N * S, 2 * D:]), as_int(qkv[: N * S, 2 * D:])))
    c.true("adapter rows untouched", torch.equal(as_int(got[N * S:]), as_int(qkv[N * S:])))
    c.done()


# ------------------------------------------------------------------------------ embed + splice
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", [4, 260])
def test_embed_splice_edges(dtype, D):
    """123 rows (not a multiple of the 4 rows of a workgroup), D = 4 (one lane) and 260 (a second lane trip). Mode 0 with the frames
    at the very start, at the very end, and with no frames at all; mode 1 with two frames of one sample aimed at one row: the row
    is accumulated frame-ascending in storage precision, rounded after each add (the kernel documents that order)."""
    B, S, F, V = 3, 41, 10, 50
    g = torch.Generator().manual_seed(D)
    ids = torch.randint(0, V, (B, S), generator=g)
    emb, vf = rnd(V, D, dtype=dtype, seed=1), rnd(B * F, D, dtype=dtype, seed=2)
    for vstart in (0, S - F):
        h = torch.full((B * S, D), float("nan"), dtype=dtype, device=DEV)
        ops.embed_splice(dev(ids), dev(emb), dev(vf), h, B, S, F, vstart=vstart, mode=0)
        ref = emb[ids].clone()
        ref[:, vstart:vstart + F] = vf.view(B, F, D)
        assert torch.equal(h.cpu().view(B, S, D), ref), vstart
    h = torch.full((B * S, D), float("nan"), dtype=dtype, device=DEV)
    ops.embed_splice(dev(ids), dev(emb), torch.empty(0, D, dtype=dtype, device=DEV), h, B, S, 0, vstart=7, mode=0)
    assert torch.equal(h.cpu().view(B, S, D), emb[ids])                                        # F = 0
    # mode 1: frames 2 and 7 of sample 1 both go to row 20 (a zero-labelled row), frames 0 and 1 of sample 2 to row 40, which
    # keeps its embedding
    idx = torch.stack([torch.arange(p, p + F) for p in (0, 15, 31)])
    idx[1, 7] = idx[1, 2] = 20
    idx[2, 0] = idx[2, 1] = 40
    lab = torch.full((B, S), -1, dtype=torch.int64)
    lab[0, :F] = torch.arange(F)
    lab[1, 15:25] = torch.arange(F)
    ops.embed_splice(dev(ids), dev(emb), dev(vf), h, B, S, F, zero_labels=dev(lab), index=dev(idx), mode=1)
    ref = (emb[ids].float() * (~(lab >= 0))[..., None]).to(dtype)
    for b in range(B):
        for f in range(F):                                                                     # frame-ascending, rounded each time
            s = int(idx[b, f])
            ref[b, s] = (ref[b, s].float() + vf.view(B, F, D)[b, f].float()).to(dtype)
    assert torch.equal(h.cpu().view(B, S, D), ref)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", [4, 260])
def test_splice_bwd_skips_indices_outside_the_sequence(dtype, D):
    """An index of -1 or S names no row: that d_tok row keeps what it held; every other row is old + dh (one fp32 add: exact)."""
    B, S, F = 3, 41, 10
    dh = rnd(B * S, D, dtype=dtype, seed=5)
    idx = torch.stack([torch.arange(p, p + F) for p in (0, 15, 31)])
    idx[0, 4], idx[2, 9] = -1, S
    old = rnd(B * F, D, seed=6)
    d_tok = dev(old)
    ops.splice_bwd(dev(dh), d_tok, B, S, F, index=dev(idx), mode=1)
    want = old.view(B, F, D).clone()
    for b in range(B):
        for f in range(F):
            s = int(idx[b, f])
            if 0 <= s < S:
                want[b, f] += dh.view(B, S, D)[b, s].float()
    assert torch.equal(d_tok.cpu().view(B, F, D), want)
    d_tok = dev(old)
    ops.splice_bwd(dev(dh), d_tok, B, S, F, vstart=S - F, mode=0)
    assert torch.equal(d_tok.cpu().view(B, F, D), old.view(B, F, D) + dh.view(B, S, D)[:, S - F:].float())


# ------------------------------------------------------------------------------ visual projection
VP_SHAPES = [(128, 8, 64, 520),       # nrb = 8 on the MFMA kernel, D % 16 = 8, one k-step per wave
             (120, 10, 832, 512),     # MFMA kernel, K / 4 = 208: three full trips of four k-steps and a partial one
             (129, 3, 768, 520),      # one row past the MFMA kernel: the wave kernel with K % 64 == 0
             (160, 10, 768, 512),     # batch 16
             (30, 10, 1792, 40),      # K > 1024: the <32, 2, 4> backward; D % 16 = 8
             (30, 10, 100, 24)]       # K % 64 != 0 at few rows: the wave kernel on a ragged K; 6 live rows in the last <16, 4, 8>
                                      # trip; D % 16 = 8 in a grid of two workgroups


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("R,F,K,D", VP_SHAPES)
def test_visual_proj_row_counts_and_k_ranges(dtype, R, F, K, D):
    video, W, temp = rnd(R, K, seed=1), rnd(D, K, scale=1 / math.sqrt(K), seed=2), rnd(F, D, seed=3)
    raw = torch.full((R, D), float("nan"), device=DEV)
    tok = torch.full((R, D), float("nan"), dtype=dtype, device=DEV)
    ops.visual_proj_fwd(dev(video), dev(W), dev(temp), raw, tok)
    ref = video.double() @ W.double().T
    c = Checks(f"visual_proj {dtype} R={R} F={F} K={K} D={D}")
    c.lt("vf_raw per row", row_err(raw, ref, "vf_raw"), 2e-6)
    c.lt("vf_tok per row", row_err(tok, ref + temp.double().repeat(R // F, 1), "vf_tok"), tol(dtype, 2e-6, 5e-3))
    d_tok, d_qav = rnd(R, D, seed=4), rnd(R, D, seed=5)
    bW, bT = rnd(D, K, seed=6), rnd(F, D, seed=7)
    for dq in (d_qav, None):
        dW, dT = dev(bW), dev(bT)
        ops.visual_proj_bwd(dev(d_tok), None if dq is None else dev(dq), dev(video), dW, dT)
        gsum = d_tok.double() if dq is None else (d_tok + dq).double()      # (the kernel adds the two in fp32 as well)
        name = "without d_qav" if dq is None else "with d_qav"
        c.lt(f"dW per row, {name}", row_err(dW, bW.double() + gsum.T @ video.double(), "dW"), 2e-6)
        c.lt(f"dtemporal per row, {name}", row_err(dT, bT.double() + d_tok.double().view(R // F, F, D).sum(0), "dT"), 2e-6)
    c.done()


def test_visual_proj_mfma_and_wave_kernels_agree_on_their_common_rows():
    """R = 128 runs on the matrix cores, R = 129 on the wave-per-feature kernel: the same 128 frame rows through both must agree
    within the fp32 bound of either against fp64."""
    K, D = 768, 520
    video, W = rnd(129, K, seed=1), rnd(D, K, scale=1 / math.sqrt(K), seed=2)
    out = {}
    for R, F in ((128, 8), (129, 3)):
        raw = torch.empty(R, D, device=DEV)
        tok = torch.empty(R, D, device=DEV)
        ops.visual_proj_fwd(dev(video[:R]), dev(W), torch.zeros(F, D, device=DEV), raw, tok)
        assert torch.equal(raw, tok)                     # fp32 token output, zero temporal embedding
        out[R] = raw.cpu()
    e = row_err(out[128], out[129][:128], "mfma against wave")
    print(f"[edges] visual_proj mfma against wave kernel, per row: {e:.3e} (bound 2.0e-06)")
    assert e < 2e-6
