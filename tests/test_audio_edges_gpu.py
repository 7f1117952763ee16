"""The audio front end (csrc/heads.hip: proj_fwd_mfma_k, proj_fwd_k, proj_bwd_k, temporal_bwd_k, av_proj_dx_k,
av_cross_attn_fwd_k / _bwd_k) against fp64 PER ROW on every branch the kernels have: partial trips of the unrolled k-loops,
feature / row / column clamps, row counts around the row blocks, ragged K, the thresholds between the kernel forms, pitched
operands, the second chunk of queries and the second column tile of the cross-attention backward. Cases, routes, inputs and
references: tests/audio_edges_util.py (checked without a GPU by tests/test_audio_edges_cpu.py).

Every call goes through fvqa.ops. Pitched operands are column ranges of buffers whose other columns are NaN; written outputs are
prefilled with NaN, accumulated ones with a random base, and every bit outside the result must come back unchanged. Bounds: 2e-6
per row for the exact-fp32 projections and 5e-3 for a cast token row of a 16-bit build (tests/test_rowops_edges_gpu.py,
tests/test_audio_gpu.py); for the cross-attention max(2e-6, 4 x the figure of an fp32 restatement of the same formula on the same
inputs against fp64) — x and dv per row, dq and dk against the magnitude of what cancels in dS (audio_edges_util.ca_dens). Every
check prints its figure before it asserts (-s; profiles/audio_edges.log keeps one such run and the mutations each test caught)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from fvqa import ops  # noqa: E402
from tests import audio_edges_util as U  # noqa: E402
from tests.test_rowops_edges_gpu import DEV, DTYPES, Checks, row_err  # noqa: E402

NAN = float("nan")


def dev(x):
    return x.to(DEV).contiguous()


def view(buf_d, c0, cols, rows=None):
    return buf_d[:rows if rows is not None else buf_d.shape[0], c0:c0 + cols]


def nan_out(rows, cols, dtype=torch.float32, extra=2):
    """A written output with `extra` rows behind it, all NaN -> (buffer, the (rows, cols) result in it, a host copy of before)."""
    buf = torch.full((rows + extra, cols), NAN, dtype=dtype, device=DEV)
    return buf, buf[:rows], buf.cpu()


def rows_mask(buf, rows):
    return U.mask2d(tuple(buf.shape), rows, 0, buf.shape[1])


def fwd_sources(case, p):
    """Device sources of a forward case: `concat` weights as two column ranges of ONE NaN-padded matrix, pitched x likewise."""
    xs = []
    for x in p["xs"]:
        if case.xpitch:
            b, c0 = U.pitched(x)
            xs.append(view(dev(b), c0, x.shape[1]))
        else:
            xs.append(dev(x))
    if case.layout == "concat":
        offs, width = U.two_ranges(*case.Ks)
        W = torch.full((case.D, width), NAN)
        for o, w in zip(offs, p["ws"]):
            W[:, o:o + w.shape[1]] = w
        Wd = dev(W)
        ws = [view(Wd, o, k) for o, k in zip(offs, case.Ks)]
    elif case.xpitch:
        ws = []
        for w in p["ws"]:
            b, c0 = U.pitched(w)
            ws.append(view(dev(b), c0, w.shape[1]))
    else:
        ws = [dev(w) for w in p["ws"]]
    return list(zip(xs, ws))


def run_fwd(case, p, srcs, bias, F, dtype, c, tag=""):
    """One launch of one mode, twice; -> the raw result (host)."""
    R, D = case.R, case.D
    raw_ref, tok_ref = U.fwd_refs(case, p, bias, F)
    Fn = None if F is None else (R if F == "R" else F)
    what = f"{tag}bias={int(bias)} F={Fn}"
    outs = []
    for _ in range(2):
        rawb, raw, raw0 = nan_out(R, D)
        tokb = tok = tok0 = None
        if Fn is not None:
            tokb, tok, tok0 = nan_out(R, D, dtype)
        ops.av_proj_fwd(srcs, raw, bias=dev(p["bias"]) if bias else None,
                        temporal=dev(p["temporal"][:Fn]) if Fn is not None else None, out_tok=tok)
        outs.append((rawb.cpu(), None if tokb is None else tokb.cpu()))
    (rawh, tokh), (rawh2, tokh2) = outs
    c.true(f"{what} two launches bitwise equal", U.outside_unchanged(rawh, rawh2, torch.zeros(rawh.shape, dtype=torch.bool))
           and (tokh is None or U.outside_unchanged(tokh, tokh2, torch.zeros(tokh.shape, dtype=torch.bool))))
    c.true(f"{what} rows behind raw untouched", U.outside_unchanged(rawh, raw0, rows_mask(rawh, R)))
    c.lt(f"{what} raw per row", row_err(rawh[:R], raw_ref, what), U.PROJ)
    if Fn is not None:
        c.true(f"{what} rows behind tok untouched", U.outside_unchanged(tokh, tok0, rows_mask(tokh, R)))
        c.lt(f"{what} tok per row", row_err(tokh[:R], tok_ref, what), U.PROJ if dtype == torch.float32 else U.PROJ_H16)
    return rawh[:R]


# ------------------------------------------------------------------------------ forward projections
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", U.FWD_CASES, ids=lambda c: c.name)
def test_av_proj_fwd_edges(case, dtype):
    p = U.fwd_problem(case)
    c = Checks(f"av_proj_fwd {dtype} {case.name}")
    c.true("route", not U.holds(U.route_fwd(case.R, case.Ks, case.D, False, True), case.expect))
    srcs = fwd_sources(case, p)
    for bias, F in (U.FWD_MODES if dtype == torch.float32 else U.H16_MODES):
        run_fwd(case, p, srcs, bias, F, dtype, c)
    c.done()


def test_av_proj_fwd_mfma_and_wave_forms_agree_on_their_common_rows():
    """128 rows run the MFMA form, 129 the streamed wave form: two sources, the same first 128 rows and the same weights — each
    against fp64 and against the other, per row (the two-source twin of
    test_visual_proj_mfma_and_wave_kernels_agree_on_their_common_rows)."""
    Ks, D = U.AGREE["Ks"], U.AGREE["D"]
    big = U.Fwd("agree-R129", Ks, "concat", 129, D, False, {}, "")
    assert U.route_fwd(128, Ks, D, True, True)["form"] == "mfma" and U.route_fwd(129, Ks, D, True, True)["form"] == "stream"
    p = U.fwd_problem(big)
    small = big._replace(name="agree-R128", R=128)
    p128 = {"xs": [x[:128] for x in p["xs"]], "ws": p["ws"], "bias": p["bias"], "temporal": p["temporal"][:128],
            "ref": p["ref"][:128]}
    c = Checks("av_proj_fwd mfma against wave, two sources")
    a = run_fwd(small, p128, fwd_sources(small, p128), True, 1, torch.float32, c, "R=128 ")
    b = run_fwd(big, p, fwd_sources(big, p), True, 1, torch.float32, c, "R=129 ")
    ref = p["ref"][:128] + p["bias"].double()[None, :]
    den = ref.abs().amax(1)
    c.lt("mfma against wave, per row", float(((a.double() - b[:128].double()).abs().amax(1) / den).max()), U.PROJ)
    c.done()


# ------------------------------------------------------------------------------ backward projections
def run_bwd(case, p, c):
    R, D = case.R, case.D
    base = p["dW_base"]
    dWd = dev(base)
    srcs = [(dev(x), view(dWd, o, k)) for o, k, x in zip(p["dW_offs"], case.Ks, p["xs"])]
    inside = torch.zeros(base.shape, dtype=torch.bool)
    for o, k in zip(p["dW_offs"], case.Ks):
        inside[:, o:o + k] = True
    extra = {}
    if case.entry == "linear":
        if case.gpitch:
            gb, c0 = U.pitched(p["g0"])
            g = view(dev(gb), c0, D)
        else:
            g = dev(p["g0"])
        dbias = dev(p["dbias_base"]) if case.bias else None
        ops.av_linear_bwd(g, srcs, dbias[:D] if case.bias else None)
        if case.bias:
            extra["dbias"] = dbias.cpu()
    else:
        dtemp = dev(p["dtemp_base"])
        ops.av_proj_bwd(dev(p["g0"]), dev(p["g1"]), srcs, dtemp[:case.F])
        extra["dtemp"] = dtemp.cpu()
    got = dWd.cpu()
    if c is None:                                             # the second launch: compared bit for bit by the caller
        return got, extra
    c.true("dW columns between and beside the ranges untouched", U.outside_unchanged(got, base, inside))
    for s, (o, k, ref) in enumerate(zip(p["dW_offs"], case.Ks, p["dW_ref"])):
        c.lt(f"dW{s} per row", row_err(got[:, o:o + k], ref, case.name), U.PROJ)
    if "dbias" in extra:
        b = extra["dbias"]
        c.true("dbias tail untouched", torch.equal(b[D:], p["dbias_base"][D:]))
        c.lt("dbias (added once)", row_err(b[None, :D], p["dbias_ref"][None, :], case.name), U.PROJ)
        # twice would be off by |sum g|: far above the bound whenever it is resolved at all
        c.lt("dbias - base against sum g, per element scale",
             float((b[:D].double() - p["dbias_ref"]).abs().max() / p["g0"].double().sum(0).abs().max()), 1e-5)
    if "dtemp" in extra:
        t = extra["dtemp"]
        c.true("dtemporal row behind untouched", torch.equal(t[case.F:], p["dtemp_base"][case.F:]))
        c.lt("dtemporal per row", row_err(t[:case.F], p["dtemp_ref"], case.name), U.PROJ)
    return got, extra


def _bwd_groups():
    groups = {}
    for case in U.BWD_CASES:
        groups.setdefault(case.name.rsplit("-R", 1)[0].split("-D")[0], []).append(case)
    return groups


BWD_GROUPS = _bwd_groups()


@pytest.mark.parametrize("group", sorted(BWD_GROUPS))
def test_av_proj_and_linear_bwd_edges(group):
    bad = []
    for case in BWD_GROUPS[group]:
        p = U.bwd_problem(case)
        c = Checks(f"{case.entry}_bwd {case.name}")
        c.true("route", not U.holds(U.route_bwd(case.R, case.Ks, case.D, case.bias), case.expect))
        a, ea = run_bwd(case, p, c)
        b, eb = run_bwd(case, p, None)
        c.true("two launches bitwise equal", torch.equal(a, b) and all(torch.equal(ea[k], eb[k]) for k in ea))
        bad += c.bad and [(case.name, c.bad)]
    assert not bad, bad


def test_av_bwd_refusals_touch_nothing():
    """K = 2052 is beyond the 2048 columns a wave keeps in registers: FVQA_ESHAPE from both entries. A source pitch that is no
    multiple of 4 floats breaks the 16-byte loads: FVQA_EALIGN. No output is touched."""
    inp = U.Inputs("refusals")
    R, D = 4, 8
    g, g1 = dev(inp.t("g", R, D)), dev(inp.t("g1", R, D))
    x = dev(inp.t("x", R, 2052))
    dW0, db0, dt0 = inp.t("dW", D, 2052), inp.t("db", D), inp.t("dt", R, D)
    dW, db, dt = dev(dW0), dev(db0), dev(dt0)
    with pytest.raises(RuntimeError, match="ESHAPE"):
        ops.av_linear_bwd(g, [(x, dW)], db)
    with pytest.raises(RuntimeError, match="ESHAPE"):
        ops.av_proj_bwd(g, g1, [(x, dW)], dt)
    xp = dev(inp.t("xp", R, 102))[:, :100]                    # pitch 102: rows 2 and 3 start off a 16-byte boundary
    with pytest.raises(RuntimeError, match="EALIGN"):
        ops.av_linear_bwd(g, [(xp, dW[:, :100])], db)
    with pytest.raises(RuntimeError, match="EALIGN"):
        ops.av_proj_bwd(g, g1, [(xp, dW[:, :100])], dt)
    raw = torch.full((R, D), NAN, device=DEV)
    with pytest.raises(RuntimeError, match="EALIGN"):
        ops.av_proj_fwd([(xp, dW[:, :100])], raw)
    torch.cuda.synchronize()
    assert torch.equal(dW.cpu(), dW0) and torch.equal(db.cpu(), db0) and torch.equal(dt.cpu(), dt0)
    assert bool(torch.isnan(raw).all())


# ------------------------------------------------------------------------------ av_proj_dx
@pytest.mark.parametrize("dim", [64, 320, 576])
def test_av_proj_dx_edges(dim):
    bad = []
    for case in [x for x in U.DX_CASES if x.dim == dim]:
        p = U.dx_problem(case)
        c = Checks(f"av_proj_dx {case.name}")
        c.true("route", not U.holds(U.route_dx(case.rows, case.dim, case.k), case.expect))
        outs = []
        for _ in range(2):
            gb, gc = U.pitched(p["g0"])
            g0 = view(dev(gb), gc, dim)
            g1 = view(dev(U.pitched(p["g1"])[0]), gc, dim) if case.g1 else None
            wb, wc = U.pitched(p["w"])
            dxb = torch.full((case.rows + 2, case.k + 2 * U.PAD), NAN, device=DEV)
            before = dxb.cpu()
            ops.av_proj_dx(g0, g1, view(dev(wb), wc, case.k), view(dxb, U.PAD, case.k, case.rows))
            outs.append(dxb.cpu())
        c.true("two launches bitwise equal", U.outside_unchanged(outs[0], outs[1], torch.zeros(before.shape, dtype=torch.bool)))
        c.true("dx outside columns and rows untouched",
               U.outside_unchanged(outs[0], before, U.mask2d(tuple(before.shape), case.rows, U.PAD, case.k)))
        c.lt("dx per row", row_err(outs[0][:case.rows, U.PAD:U.PAD + case.k], p["ref"], case.name), U.PROJ)
        bad += c.bad and [(case.name, c.bad)]
    assert not bad, bad


# ------------------------------------------------------------------------------ cross-attention
def ca_operands(case, p):
    """q pitched in a NaN-padded buffer; k | v as two column ranges of one NaN-padded buffer."""
    dim = case.dim
    qb, qc = U.pitched(p["q"])
    offs, width = U.two_ranges(dim, dim)
    kv = torch.full((U.CA_B * case.T, width), NAN)
    kv[:, offs[0]:offs[0] + dim], kv[:, offs[1]:offs[1] + dim] = p["k"], p["v"]
    kvd = dev(kv)
    return view(dev(qb), qc, dim), view(kvd, offs[0], dim), view(kvd, offs[1], dim), offs, width


def run_ca_fwd(case, p, c):
    B, nq, T, dim = U.CA_B, case.nq, case.T, case.dim
    q, k, v, _, _ = ca_operands(case, p)
    outs = []
    for _ in range(2):
        xb, x, x0 = nan_out(B * nq, dim)
        ops.av_cross_attn_fwd(q, k, v, x, B, nq, T)
        outs.append(xb.cpu())
    c.true("x two launches bitwise equal", U.outside_unchanged(outs[0], outs[1], torch.zeros(x0.shape, dtype=torch.bool)))
    c.true("rows behind x untouched", U.outside_unchanged(outs[0], x0, rows_mask(x0, B * nq)))
    got = outs[0][:B * nq]
    print(f"[edges] {c.case} fp32 restatement x per row: {p['own']['x']:.3e}")
    c.lt("x per row", row_err(got, p["f64"]["x"], case.name), p["bound"]["x"])
    if T == 1:
        c.true("one key: x is v bit for bit", torch.equal(got.view(B, nq, dim), p["v"].view(B, 1, dim).expand(B, nq, dim)))


def run_ca_bwd(case, p, c):
    B, nq, T, dim = U.CA_B, case.nq, case.T, case.dim
    q, k, v, offs, width = ca_operands(case, p)
    dx = dev(p["dx"])
    outs = []
    for _ in range(2):
        dqb = torch.full((B * nq + 2, dim + 2 * U.PAD), NAN, device=DEV)
        dkv = torch.full((B * T + 2, width), NAN, device=DEV)
        before = (dqb.cpu(), dkv.cpu())
        ops.av_cross_attn_bwd(q, k, v, dx, view(dqb, U.PAD, dim, B * nq), view(dkv, offs[0], dim, B * T),
                              view(dkv, offs[1], dim, B * T), B, nq, T)
        outs.append((dqb.cpu(), dkv.cpu()))
    (dqh, dkvh), (dqh2, dkvh2) = outs
    none = lambda t: torch.zeros(t.shape, dtype=torch.bool)  # noqa: E731
    c.true("dq, dk | dv two launches bitwise equal", U.outside_unchanged(dqh, dqh2, none(dqh)) and
           U.outside_unchanged(dkvh, dkvh2, none(dkvh)))
    c.true("dq outside columns and rows untouched",
           U.outside_unchanged(dqh, before[0], U.mask2d(tuple(dqh.shape), B * nq, U.PAD, dim)))
    inside = U.mask2d(tuple(dkvh.shape), B * T, offs[0], dim) | U.mask2d(tuple(dkvh.shape), B * T, offs[1], dim)
    c.true("dk | dv outside columns and rows untouched", U.outside_unchanged(dkvh, before[1], inside))
    dq = dqh[:B * nq, U.PAD:U.PAD + dim]
    dk, dv = dkvh[:B * T, offs[0]:offs[0] + dim], dkvh[:B * T, offs[1]:offs[1] + dim]
    for name in ("dv", "dq", "dk"):
        print(f"[edges] {c.case} fp32 restatement {name}: {p['own'][name]:.3e}")
    c.lt("dv per row", row_err(dv, p["f64"]["dv"], case.name), p["bound"]["dv"])
    c.lt("dq / den_q", U.den_err(dq, p["f64"]["dq"], p["den_q"], case.name), p["bound"]["dq"])
    c.lt("dk / den_k", U.den_err(dk, p["f64"]["dk"], p["den_k"], case.name), p["bound"]["dk"])
    if T == 1:
        c.true("one key: dq and dk exactly zero", bool((dq == 0).all()) and bool((dk == 0).all()))


@pytest.mark.parametrize("nq,T", U.CA_SHAPES)
@pytest.mark.parametrize("mode", U.CA_MODES)
def test_av_cross_attn_edges(mode, nq, T):
    bad = []
    for case in [x for x in U.CA_CASES if (x.mode, x.nq, x.T) == (mode, nq, T)]:
        p = U.ca_problem(case)
        c = Checks(f"av_cross_attn {case.name}")
        c.true("route", not U.holds(U.route_ca(case.nq, case.T, case.dim), case.expect))
        c.true("condition (b)", max(p["own"].values()) < U.COND_B)
        if mode == "planted":
            c.true("planted key holds >= 0.99 of every row",
                   all(float(p["f64"]["P"][n, :, t].min()) >= 0.99 for n, t in enumerate(p["planted"])))
        run_ca_fwd(case, p, c)
        run_ca_bwd(case, p, c)
        bad += c.bad and [(case.name, c.bad)]
    assert not bad, bad


@pytest.mark.parametrize("case", U.CA_BIG_CASES, ids=lambda c: c.name)
def test_av_cross_attn_fwd_scores_beyond_100(case):
    """Every row's largest score is above 100 (up to thousands): exp() of it overflows fp32 unless the maximum is subtracted."""
    p = U.ca_problem(case)
    c = Checks(f"av_cross_attn_fwd {case.name}")
    c.true("every row's top score > 100", float(p["f64"]["S"].amax(-1).min()) > 100.0)
    run_ca_fwd(case, p, c)
    c.done()


def test_av_cross_attn_fwd_refuses_17_keys():
    inp = U.Inputs("ca-refusal")
    q, kv = dev(inp.t("q", 2, 8)), dev(inp.t("kv", 34, 16))
    x = torch.full((2, 8), NAN, device=DEV)
    with pytest.raises(RuntimeError, match="ESHAPE"):
        ops.av_cross_attn_fwd(q, kv[:, :8], kv[:, 8:], x, 2, 1, 17)
    torch.cuda.synchronize()
    assert bool(torch.isnan(x).all())
