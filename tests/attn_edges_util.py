"""Helpers of the training-attention edge tests (tests/test_attn_edges_gpu.py, checked on the CPU by
tests/test_attn_edges_cpu.py): inputs and fp64 references for fvqa_attn_fwd, fvqa_attn_bwd and fvqa_attn_bwd_rotated, built on
the CPU only.

The reference is oracle/ref_cpu.attn_fwd / attn_bwd in fp64 on the storage-rounded operands; for the RoPE forms on q and k
rotated in fp64 and rounded to storage — the kernels' stated contract — with the gradients rotated back.

The measure is one figure per (row, head) vector of 128: max |got - ref| / max(max |ref vector|, 1e-2 * max |ref tensor|). The
tensor of the floor is the q, k or v column block of dqkv, text rows and adapter rows together (for `o`, the output): dk of
S = 1, the adapter dk of A = 1 and dq of row 0 at A = 1 are exactly zero in the oracle, and the floor keeps them finite.

A PLANTED key (cached_attn_util.planted, score 16) carries >= 0.99 of one query's softmax; a DECOY (score 30) sits on a key that
query must not see; a HALF plant has the score that gives the pair a weight of about one half, so that dS of the pair is large
(a score-16 plant makes dS vanish: P (dP - delta) with delta = dP); the d_o row of its query is twice the others' and
points along v[j], so that the pair outweighs what the other queries add to dk[j] and dv[j]."""
import math

import torch

from oracle import ref_cpu
from tests.cached_attn_util import AF_PAIRS, DECOY, DH, NAN, PLANT, bits, planted, rnd, rot_rows, rotated_rounded, tables  # noqa: F401

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
DTYPES = [F32, BF16, F16]
BOUND_O = {F32: 3e-5, BF16: 1e-2, F16: 1e-2}              # the project's own bounds (tests/test_kernels_gpu.py), per row here
BOUND_G = {F32: 5e-5, BF16: 2e-2, F16: 2e-2}
BOUND_GATE = {F32: 1e-4, BF16: 3e-2, F16: 3e-2}
BOUND_LSE = 1e-4                                          # absolute: fp32 on scores <= 32 (ulp 3.8e-6), 128 products, one log
FLOOR_REL = 1e-2
# Classes of rows whose bound the rounding model (model_fwd_bwd) sets, case by case, by the rule of judge(): rows whose
# softmax has one or two keys. There the oracle's dS cancels (one key: P = 1, dP = delta, dS = 0 exactly) while the kernels take
# delta from the storage-rounded `o`: what is left is dO.(o - round(o)) times a key — noise of the size of these rows' floor.
# dgate2 sums dS over the frame window, where the head with gate2 in [2, 4] keeps most of a row's weight: the same noise of
# delta, times that weight, against a sum of dS that cancels to a few per cent of its terms.
# Rows 2 to 7 are the same in kind: their few keys do not average the leftover out, and one key with a large score (the window
# cases plant one on key 0) carries the row as the only key of row 0 does.
MODEL_CLASSES = ["dq of rows 0 to 7", "dk at S <= 2", "dgate2"]
FEW_KEYS = 8

SWEEP_S = [1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 159, 160, 161, 255, 256, 257, 385]
WINDOW_S = [128, 160]                                     # fused backward, split backward
PLANT_J = [0, 15, 16, 31, 32, 127, 128, 159, 160, 255, 256]
PLANT_S = 257
HALF_S = [128, 257]
ROPE_S = [17, 128, 129, 257]
TIE_STEP = 2.0 ** -14
GROUP = 32                                                # keys per online-softmax step of the MFMA forward
TILE = 128                                                # rows per MFMA tile (csrc/attn_mfma.hip BQ)


def row_figures(got, ref, tensor_max=None):
    """One figure per (row, head) vector of 128. got, ref (R, H * DH); tensor_max: max |ref| of the tensor the rows belong to
    (default: of `ref` itself)."""
    got = got.detach().double().cpu().reshape(-1, DH)
    ref = ref.detach().double().cpu().reshape(-1, DH)
    tmax = float(ref.abs().max()) if tensor_max is None else float(tensor_max)
    den = ref.abs().amax(-1).clamp(min=FLOOR_REL * tmax)
    return (got - ref).abs().amax(-1) / den


def gates(H, seed):
    """gate1 in [-1, 1]; gate2: even heads in [-4, -2] (the trained sign), odd heads in [2, 4] — there the frame window carries
    most of a biased row's weight."""
    g2 = rnd(H, seed=seed + 2).float() + torch.tensor([-3.0, 3.0] * H)[:H]
    return rnd(H, seed=seed + 1).float(), g2


def sweep_vstart(S, F):
    return [-1, max(0, min(19, S - F))]


def window_vstarts(S, F):
    return list(dict.fromkeys([0, 6, 22, 27, 118, S - F]))               # (S - F is 118 at S = 128, F = 10: once)


def window_target(S, F, vs):
    """The query of the window case that carries a half plant on the first frame key vs: the last row, when it is biased."""
    return S - 1 if F > 0 and vs + F <= S - 1 else None


# ------------------------------------------------------------------------------------------------ the formulas, with hooks
def scores(q, k, ak, g2, vstart, F):
    """s_a (N, H, S, A) and s_t (N, H, S, S) of ref_cpu.attn_fwd: scaled, causal -inf and the gate2 window added."""
    N, S, H, _ = q.shape
    sc = 1.0 / math.sqrt(DH)
    s_a = torch.einsum("nshd,ahd->nhsa", q, ak) * sc
    s_t = torch.einsum("nshd,nthd->nhst", q, k) * sc
    bias = torch.stack([ref_cpu._text_bias(S, F, int(vs), g2, q.dtype) for vs in vstart])
    return s_a, s_t + bias


def fwd_from_scores(s_a, s_t, v, av, g1):
    """o, Pa, Pt of ref_cpu.attn_fwd from (possibly corrupted) scores."""
    Pa, Pt = torch.softmax(s_a, -1), torch.softmax(s_t, -1)
    o = torch.tanh(g1)[None, :, None, None] * torch.einsum("nhsa,ahd->nhsd", Pa, av) + torch.einsum("nhst,nthd->nhsd", Pt, v)
    return o.transpose(1, 2).contiguous(), Pa, Pt


def model_fwd_bwd(c, dtype, mfma=True, compute=torch.float64):
    """The fp64 formulas with three quantities rounded to the storage type where csrc/attn_mfma.hip rounds them: P before P.V
    (the forward: exp(s - running maximum over the groups of 32 keys so far), normalised by the unrounded sum afterwards; the
    backward: P itself; the adapter's tanh(gate1) P likewise), dS before the dQ / dK
    products, and the `o` that feeds the row deltas (delta_t = dO.o - delta_a). mfma=False: the vector build (csrc/attn.hip),
    which rounds `o` only. compute=torch.float32: every operation in float32 on the CPU — the emulation of the fp32 build.
    Returns the tensors of reference(), dq and dk in the frame of the rotated operands, and dg1, dg2 (summed from the
    unrounded dS, as the kernels do)."""
    ro = lambda t: t.to(dtype).to(compute)      # noqa: E731
    r = ro if mfma else (lambda t: t)
    q, k, v, ak, av, do = (c[t].to(compute) for t in ("q", "k", "v", "ak", "av", "do"))
    g1 = torch.tanh(c["g1"].to(compute))
    sc = 1.0 / math.sqrt(DH)
    s_a, s_t = scores(q, k, ak, c["g2"].to(compute), c["vstart_list"], c["F"])
    e_t = torch.exp(s_t - s_t.amax(-1, keepdim=True))
    Pt = e_t / e_t.sum(-1, keepdim=True)
    Pa = torch.softmax(s_a, -1)
    g1b = g1[None, :, None, None]
    # the forward rounds exp(s - running maximum) of each group of 32 keys and rescales the sums when the maximum moves
    N, H, S = s_t.shape[:3]
    gm = torch.nn.functional.pad(s_t, (0, (-S) % GROUP), value=float("-inf")).view(N, H, S, -1, GROUP).amax(-1)
    run = torch.cummax(gm, -1).values.repeat_interleave(GROUP, -1)[..., :S]
    p_fwd = r(torch.exp(s_t - run)) * torch.exp(run - s_t.amax(-1, keepdim=True)) if mfma else e_t
    o = torch.einsum("nhst,nthd->nhsd", p_fwd, v) / e_t.sum(-1, keepdim=True) + torch.einsum("nhsa,ahd->nhsd", r(Pa * g1b), av)
    o = o.transpose(1, 2)
    dov = torch.einsum("nshd,ahd->nhsa", do, av)
    dpt = torch.einsum("nshd,nthd->nhst", do, v)
    da = (Pa * g1b * dov).sum(-1, keepdim=True)
    dt = (do * ro(o)).sum(-1).transpose(1, 2)[..., None] - da
    dSa, dSt = Pa * (g1b * dov - da), Pt * (dpt - dt)
    dg1 = (dov * Pa).sum((0, 2, 3)) * (1.0 - g1 * g1)
    dg2 = torch.zeros_like(g1)
    for n, vs in enumerate(c["vstart_list"]):
        if vs >= 0:
            dg2 += dSt[n, :, vs + c["F"]:, vs:vs + c["F"]].sum((1, 2))
    dSa, dSt = r(dSa), r(dSt)
    dq = (torch.einsum("nhsa,ahd->nshd", dSa, ak) + torch.einsum("nhst,nthd->nshd", dSt, k)) * sc
    dk = torch.einsum("nhst,nshd->nthd", dSt, q) * sc
    dv = torch.einsum("nhst,nshd->nthd", r(Pt), do)
    dak = torch.einsum("nhsa,nshd->ahd", dSa, q) * sc
    dav = torch.einsum("nhsa,nshd->ahd", r(Pa * g1b), do)
    return {t: x.double() for t, x in dict(o=o, dq=dq, dk=dk, dv=dv, dak=dak, dav=dav, dg1=dg1, dg2=dg2).items()}


def near_ties(t, c64, s64, dtype, rel=2.0 ** -20):
    """Mask (..., DH / 2) of the rotation pairs of t (N, S, H, DH, storage type) one of whose ROTATED values lies within
    rel * (the larger element of the pair) of a rounding tie of the storage type whose two sides are more than TIE_STEP apart;
    a rotation in fp32 is off by a quarter of that distance at most. (A tiny value next to a large one rounds either way
    whatever is done: a step of TIE_STEP moves a score by 5e-6.)"""
    x = ref_cpu.rope_apply(t.double(), c64[: t.shape[1]], s64[: t.shape[1]])
    big = torch.maximum(t[..., 0::2].double().abs(), t[..., 1::2].double().abs())
    eps = rel * torch.stack([big, big], -1).reshape(t.shape)
    tie = ((x + eps).to(dtype).double() - (x - eps).to(dtype).double()).abs() > TIE_STEP
    return tie[..., 0::2] | tie[..., 1::2]


def untie(t, c64, s64, dtype):
    """Moves one element of each pair of near_ties() by a few storage ulps (in place) until no rotated value is near a tie: the
    kernels rotate in fp32, the reference in fp64, and both then round to the same storage values. The first and the second
    element take turns: at a small angle a whole number of ulps on one of them keeps its rotated value on the tie."""
    for it in range(12):
        m = near_ties(t, c64, s64, dtype)
        if not bool(m.any()):
            return t
        half = t[..., it % 2::2]                                             # a view of every pair's first / second element
        half[m] = (half[m].double() * (1 + 2.0 ** -7)).to(dtype)
    raise AssertionError("rotation ties did not go away")


# ------------------------------------------------------------------------------------------------ cases
def make_case(dtype, N, S, A, F, vstart, seed, H=2, rope=False, plants=(), backward=True):
    """qkv (N * S + A, 3 * H * DH) and d_o in the storage type, gates, and the fp64 references. rope: qkv holds RAW q, k and the
    reference sees them rotated in fp64 and rounded to storage (no rotated value near a rounding tie: untie). plants: (nq, i, nk, j, score) in order — key j of sequence nk
    is replaced by the key that scores `score` (a float, or "half") against query i of sequence nq, on every head."""
    D = H * DH
    qkv = rnd(N * S + A, 3 * D, dtype=dtype, seed=seed)
    d_o = rnd(N * S, D, dtype=dtype, seed=seed + 5)
    g1, g2 = gates(H, seed)
    cos, sin, c64, s64 = tables(S)
    seqs = qkv[: N * S].view(N, S, 3, H, DH)
    q, k, v = seqs[:, :, 0], seqs[:, :, 1], seqs[:, :, 2]                    # views: a planted key lands in qkv
    rot = (lambda x, pos, inv=False: rot_rows(x, pos, c64, s64, inverse=inv).to(dtype).double()) if rope else \
          (lambda x, pos, inv=False: x.to(dtype).double())
    ak = qkv[N * S:, D:2 * D].double().view(A, H, DH)
    av = qkv[N * S:, 2 * D:].double().view(A, H, DH)
    half_scores = {}
    if rope:
        untie(q, c64, s64, dtype), untie(k, c64, s64, dtype)
    for (nq, i, nk, j, score) in plants:
        qhat = rot(q[nq, i].double(), i)                                    # (H, DH) as the kernel sees it
        if score == "half":                                                  # weight 1/2: the score equals the logsumexp of
            assert nq == nk and j <= i and i > 0                             # the row's other visible keys
            kr_n = rot(k[nq, : i + 1].double(), torch.arange(i + 1)[:, None])
            s = torch.einsum("hd,thd->ht", qhat, kr_n) / math.sqrt(DH)
            s = s + ref_cpu._text_bias(S, F, int(vstart[nq]), g2.double(), torch.float64)[:, i, : i + 1]
            own = s[:, j].clone()
            s[:, j] = float("-inf")
            raw_bias = own - torch.einsum("hd,hd->h", qhat, kr_n[j]) / math.sqrt(DH)      # gate2 on the pair, or 0
            score = (torch.logsumexp(s, -1) - raw_bias)[:, None]
            half_scores[(nq, i, j)] = score[:, 0]
            # this one pair must carry dk[j] and dv[j]: the query's d_o row is twice as large and points along v[j], so dP
            # of the pair is about 64 against +-8 for its other keys, and dS of the pair a quarter of that
            d_o[nq * S + i] = 2 * d_o[nq * S + i].abs() * torch.sign(v[nk, j].reshape(-1).float()).to(dtype)
        k[nk, j] = rot(planted(qhat, score), j, True).to(dtype)
    if rope:
        untie(k, c64, s64, dtype)                                           # the planted keys: a few ulps, 1e-3 of a score
        qr, kr = rotated_rounded(q, c64, s64, dtype), rotated_rounded(k, c64, s64, dtype)
    else:
        qr, kr = q.double(), k.double()
    c = dict(qkv=qkv, d_o=d_o, g1=g1, g2=g2, cos=cos, sin=sin, c64=c64, s64=s64, vstart=torch.tensor(vstart, dtype=torch.int32),
             vstart_list=list(vstart), N=N, S=S, H=H, A=A, F=F, D=D, rope=rope, dtype=dtype, plants=list(plants),
             half_scores=half_scores, q=qr, k=kr, v=v.double(), ak=ak, av=av, do=d_o.double().view(N, S, H, DH))
    c.update(reference(c, backward))
    return c


def reference(c, backward=True):
    """The oracle's o, lse_a, lse_t (N, H, S), the text weights Pt and — backward — dq, dk, dv (N, S, H, DH; rotated back for the
    RoPE forms), dak, dav (A, H, DH), dg1, dg2 (H,)."""
    g1, g2 = c["g1"].double(), c["g2"].double()
    o, cache = ref_cpu.attn_fwd(c["q"], c["k"], c["v"], c["ak"], c["av"], g1, g2, c["vstart_list"], c["F"])
    s_a, s_t = scores(c["q"], c["k"], c["ak"], g2, c["vstart_list"], c["F"])
    out = dict(o=o, Pt=cache[1], lse_a=torch.logsumexp(s_a, -1), lse_t=torch.logsumexp(s_t, -1))
    if backward:
        dq, dk, dv, dak, dav, dg1, dg2 = ref_cpu.attn_bwd(c["do"], c["q"], c["k"], c["v"], c["ak"], c["av"], g1, g2,
                                                           c["vstart_list"], c["F"], cache)
        out.update(dq_rot=dq, dk_rot=dk)                     # in the frame of the rotated operands
        if c["rope"]:
            S = c["S"]
            dq = ref_cpu.rope_apply(dq, c["c64"][:S], c["s64"][:S], inverse=True)
            dk = ref_cpu.rope_apply(dk, c["c64"][:S], c["s64"][:S], inverse=True)
        out.update(dq=dq, dk=dk, dv=dv, dak=dak, dav=dav, dg1=dg1, dg2=dg2)
    return out


def blocks(c, r=None):
    """The reference as the column blocks of dqkv: k and v blocks (N * S + A, D), text rows then adapter rows."""
    r = c if r is None else r
    N, S, A, D = c["N"], c["S"], c["A"], c["D"]
    return dict(o=r["o"].reshape(N * S, D), dq=r["dq"].reshape(N * S, D),
                dk=torch.cat([r["dk"].reshape(N * S, D), r["dak"].reshape(A, D)]),
                dv=torch.cat([r["dv"].reshape(N * S, D), r["dav"].reshape(A, D)]))


def model_figures(c):
    """Worst per-row figure of the rounding model against the exact reference, per tensor (RoPE forms: in the rotated frame)."""
    m, ref = model_fwd_bwd(c, c["dtype"]), dict(c, dq=c["dq_rot"], dk=c["dk_rot"])
    bm, br = blocks(c, m), blocks(c, ref)
    return {t: float(row_figures(bm[t], br[t]).max()) for t in ("o", "dq", "dk", "dv")}


def class_masks(c):
    """{tensor: bool mask over the rows of its block (row, head)} of MODEL_CLASSES in this case."""
    N, S, A, H = c["N"], c["S"], c["A"], c["H"]
    first = torch.zeros(N, S, H, dtype=torch.bool)
    first[:, :FEW_KEYS] = True
    text_k = torch.zeros(N * S + A, H, dtype=torch.bool)
    text_k[: N * S] = S <= 2
    return dict(dq=first.view(N * S, H), dk=text_k)


def whole(got, ref):
    return float((got.double() - ref).abs().max() / (ref.abs().max() + 1e-30))


def judge(what, c, got, mfma=True, log=print):
    """got: o, dq (N * S, D), dk, dv (N * S + A, D), dg1, dg2 (H,) as the kernels left them. Prints the worst per-row figure of
    each tensor and asserts the bounds: the project's, per row (the gate gradients: per vector, as tests/test_kernels_gpu.py
    does). Only where the kernel is OVER the project's bound on the rows of one of MODEL_CLASSES (or on dgate2) is the rounding
    model consulted: if the model itself is off by more than half the project's bound there, the bound of that class in this
    case is twice the model's figure, and the kernel's deviation must be the model's: kernel against model, in the same
    measure, within the project's bound. Otherwise the excess stands as a failure.
    fp32 has one such case, dk at S = 1: storage rounding explains a fifth of what fp32 arithmetic leaves of the exact zero, so
    there the model is the same formulas evaluated in float32 on the CPU, times four, with no common realisation to compare."""
    dtype, ref = c["dtype"], blocks(c)
    masks, cache = class_masks(c), {}

    def model(compute=torch.float64):
        if compute not in cache:
            m = model_fwd_bwd(c, dtype, mfma, compute=compute)
            if c["rope"]:
                S = c["S"]
                m["dq"] = ref_cpu.rope_apply(m["dq"], c["c64"][:S], c["s64"][:S], inverse=True)
                m["dk"] = ref_cpu.rope_apply(m["dk"], c["c64"][:S], c["s64"][:S], inverse=True)
            cache[compute] = (m, blocks(c, m))
        return cache[compute]

    worst, fails = {}, []
    for t in ("o", "dq", "dk", "dv"):
        assert bool(torch.isfinite(got[t].float()).all()), f"{what}: {t} is not finite"
        f = row_figures(got[t], ref[t]).view(-1, c["H"])
        bound = (BOUND_O if t == "o" else BOUND_G)[dtype]
        limit, note = torch.full_like(f, bound), ""
        mask = masks.get(t)
        if mask is not None and bool(mask.any()) and float(f[mask].max()) >= bound:
            kf = float(f[mask].max())
            bm = model()[1]
            mf = float(row_figures(bm[t], ref[t]).view(-1, c["H"])[mask].max())
            if mf > bound / 2:
                agree = float(row_figures(got[t].double() - bm[t] + ref[t], ref[t]).view(-1, c["H"])[mask].max())
                note = f" [class rows: kernel {kf:.3e}, model {mf:.3e}, bound {2 * mf:.3e}; kernel against model {agree:.3e}]"
                if agree < bound:
                    limit[mask] = 2 * mf
            elif dtype == F32 and t == "dk":
                ef = float(row_figures(model(torch.float32)[1][t], ref[t]).view(-1, c["H"])[mask].max())
                note = f" [class rows: kernel {kf:.3e}, storage model {mf:.3e}, float32 emulation {ef:.3e}, bound {4 * ef:.3e}]"
                if ef > bound / 2:
                    limit[mask] = 4 * ef
            else:
                note = f" [class rows: kernel {kf:.3e}, model {mf:.3e}: not explained]"
            rest = f[~mask]
            worst[t] = float(rest.max()) if rest.numel() else 0.0
        worst.setdefault(t, float(f.max()))
        log(f"{what}: {t} worst row {worst[t]:.3e} (bound {bound:.1e}){note}")
        if bool((f >= limit).any()):
            fails.append(t)
    for t in ("dg1", "dg2"):
        assert bool(torch.isfinite(got[t]).all()), f"{what}: {t} is not finite"
        f, bound, note = whole(got[t], c[t]), BOUND_GATE[dtype], ""
        limit = bound
        if t == "dg2" and f >= bound and dtype != F32:
            m = model()[0]
            mf = whole(m[t], c[t])
            agree = whole(got[t].double() - m[t] + c[t], c[t])
            note = f" [model {mf:.3e}, bound {2 * mf:.3e}; kernel against model {agree:.3e}]"
            if mf > bound / 2 and agree < bound:
                limit = 2 * mf
        worst[t] = f
        log(f"{what}: {t} {f:.3e} (bound {bound:.1e}){note}")
        if f >= limit:
            fails.append(t)
    assert not fails, f"{what}: {fails} over their bound"
    return worst


def sweep_case(dtype, S, rope=False):
    """Case 1: N = 2, H = 2, A = F = 10, vstart = [-1, min(19, S - F)] clamped at 0."""
    return make_case(dtype, 2, S, 10, 10, sweep_vstart(S, 10), seed=100 + S, rope=rope)


def window_case(dtype, S, A, F, vs):
    """Case 2: one sequence with the frame window at vs, one without a window. When the last row is biased, the first frame key
    vs is a half plant for it, on both heads: half of that row hangs on one key whose score holds gate2, so a window that
    starts one key late, or a bias left out, moves the row by about half of v[vs] — whatever the sign of gate2."""
    i = window_target(S, F, vs)
    return make_case(dtype, 2, S, A, F, [vs, -1], seed=300 + S + 7 * A + F + vs, plants=[(0, i, 0, vs, "half")] if i else [])


def plant_grid(S):
    """(i, j) of cases 3 and 4: key j of PLANT_J for the queries j, j + 1, the first row of the next tile and S - 1."""
    out = []
    for j in PLANT_J:
        for i in (j, j + 1, (j // TILE + 1) * TILE, S - 1):
            if j < S and i < S and (i, j) not in out:
                out.append((i, j))
    return out


def decoys_of(i, S):
    """Keys query i must not see: i + 1, the first key of the next 16-block, 32-group and tile (inside the sequence)."""
    return sorted({p for p in (i + 1, (i // 16 + 1) * 16, (i // 32 + 1) * 32, (i // TILE + 1) * TILE) if p < S})


def pack_pairs(S, half):
    """The (i, j) grid spread over sequences so that no key (planted, or a decoy) and no query is used twice in one. Returns a
    list of sequences, each a list of (i, j, decoy positions). Half plants carry no decoys and leave out i = 0, whose softmax
    has one key: its weight is 1 whatever the score."""
    seqs = []
    for (i, j) in plant_grid(S):
        if half and i == 0:
            continue
        dec = [] if half else decoys_of(i, S)
        touched = {j, *dec}
        for s in seqs:
            if not (touched & s["keys"]) and i not in s["queries"] and not ({i} & s["keys"] - {j}):
                break
        else:
            s = dict(keys=set(), queries=set(), pairs=[])
            seqs.append(s)
        s["keys"] |= touched
        s["queries"].add(i)
        s["pairs"].append((i, j, dec))
    return [s["pairs"] for s in seqs]


def planted_cases(dtype, S=PLANT_S, half=False, rope=False, vstart=(19, -1)):
    """Cases 3 and 4, two sequences per launch (N = 2, H = 2, A = F = 10). Each case carries `pairs`: (n, i, j, decoys) with
    decoys a list of (nk, position). Forward cases (half=False): the last query of sequence 0, when it is planted for, also gets
    a decoy on row 0 of sequence 1 — tile-local index S of sequence 0."""
    packed = pack_pairs(S, half)
    if not half:                        # the last launch: a sequence with planted last queries in front of a plain sequence
        last = max(a for a, seq in enumerate(packed) if any(i == S - 1 for (i, _, _) in seq))
        rest = packed[:last] + packed[last + 1:]
        packed = rest + [[]] * (len(rest) % 2) + [packed[last], []]
    cases = []
    for a in range(0, len(packed), 2):
        plants, pairs = [], []
        two = packed[a:a + 2]
        cross = not half and a + 2 == len(packed)
        for n, seq in enumerate(two):
            for (i, j, dec) in seq:
                where = [(n, p) for p in dec]
                if cross and n == 0 and i == S - 1:
                    where.append((1, 0))
                plants.append((n, i, n, j, "half" if half else PLANT))
                plants += [(n, i, nk, p, DECOY) for (nk, p) in where]
                pairs.append((n, i, j, where))
        c = make_case(dtype, 2, S, 10, 10, list(vstart), seed=500 + S + a + (7 if half else 0), rope=rope, plants=plants,
                      backward=half)
        c["pairs"] = pairs
        cases.append(c)
    return cases


def reuse_case(dtype, S):
    """Case 6: N = 3, H = 2, A = F = 10."""
    return make_case(dtype, 3, S, 10, 10, [19, -1, min(100, S - 10)], seed=700 + S)


def lse_fp32_emulation(c):
    """The logsumexp of the same scores evaluated in torch float32 on the CPU, against fp64: worst absolute figure."""
    f = torch.float32
    s_a, s_t = scores(c["q"].to(f), c["k"].to(f), c["ak"].to(f), c["g2"].to(f), c["vstart_list"], c["F"])
    return max(float((torch.logsumexp(s_a, -1).double() - c["lse_a"]).abs().max()),
               float((torch.logsumexp(s_t, -1).double() - c["lse_t"]).abs().max()))
