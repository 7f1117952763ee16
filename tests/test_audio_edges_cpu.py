"""tests/audio_edges_util.py without a GPU: its fp64 references against independent ones (autograd, the torch.cat forms), its
restatement of heads.hip's routing for every case, the coverage of the kernel branches by the case tables, and the two
preconditions on the inputs that the bounds of tests/test_audio_edges_gpu.py rest on:
  (a) an fp32 product stays under 1e-6 per row against fp64 for every projection case (half of the 2e-6 bound);
  (b) the fp32 restatement of the cross-attention stays under 5e-6 against fp64 in its figures (so no bound exceeds 2e-5).
A case that violates one is changed (other inputs, other shape), never the bound. Both are evaluated in a summation order that
is fixed by the code (audio_edges_util.tree_sum), so that they are properties of the inputs and not of the host's BLAS; the
figure of torch's own fp32 matmul is printed beside (a) for the record."""
import math

import pytest
import torch

from tests import audio_edges_util as U


# ------------------------------------------------------------------------------ routes and coverage
def test_every_case_takes_the_route_it_was_written_for():
    bad = []
    for c in U.FWD_CASES:
        bad += [(c.name, U.holds(U.route_fwd(c.R, c.Ks, c.D, False, True), c.expect))]
    for c in U.BWD_CASES:
        bad += [(c.name, U.holds(U.route_bwd(c.R, c.Ks, c.D, c.bias), c.expect))]
    for c in U.DX_CASES:
        bad += [(c.name, U.holds(U.route_dx(c.rows, c.dim, c.k), c.expect))]
    for c in U.CA_CASES:
        bad += [(c.name, U.holds(U.route_ca(c.nq, c.T, c.dim), c.expect))]
    bad = [b for b in bad if b[1]]
    assert not bad, bad


def test_route_restates_the_thresholds_of_heads_hip():
    f = U.route_fwd
    assert f(128, (768, 1024), 4096, False, True)["form"] == "mfma" and f(129, (768, 1024), 4096, False, True)["form"] == "stream"
    assert f(8, (100,), 16, False, True)["form"] == "held" and f(8, (2048 + 4,), 16, False, True)["form"] == "stream"
    assert f(129, (2048,), 16, False, True)["form"] == "held" and f(8, (100, 64), 16, False, True)["form"] == "stream"
    assert not f(8, (64,), 16, False, True)["opt"] and f(8, (64,), 16, True, True)["opt"] and f(8, (64,), 16, False, False)["opt"]
    # the step's own shapes: 768 = 12 k-steps of 16 per wave = 3 whole trips, 1024 = 4 whole trips
    assert f(80, (768, 1024), 4096, False, True)["partial"] == [0, 0]
    assert f(17, (64, 320), 24, False, True)["partial"] == [1, 1] and f(17, (64, 320), 24, False, True)["trips"] == [1, 2]
    b = U.route_bwd
    assert b(8, (768, 1024), 16, False)["form"] == "narrow" and b(8, (768, 1028), 16, False)["form"] == "wide"
    assert b(8, (768, 1028), 16, False)["launches"] == 2 and b(33, (768,), 21, True)["row_rem"] == 1
    assert not b(80, (768, 1024), 4096, False)["d_partial"]
    assert U.route_dx(80, 4096, 768) == {"steps": 64, "trips": 8, "partial": 0, "col_tiles": 48, "k_clamp": False,
                                         "row_tiles": 5, "row_rem": 0}
    assert U.route_ca(10, 10, 768)["chunks"] == 1 and U.route_ca(17, 16, 1028) == {"chunks": 2, "last_chunk": 1, "col_tiles": 2,
                                                                                   "col_rem": 4, "T": 16}


def test_the_case_tables_hit_every_cell_of_the_gap_table():
    hit = U.coverage()
    for cell, names in sorted(hit.items()):
        print(f"[audio edges] {cell}: {len(names)} cases, e.g. {names[0] if names else '-'}")
    assert not [cell for cell, names in hit.items() if not names]
    # the shapes the issue lists are all there
    fw = {(c.Ks, c.layout, c.R, c.D) for c in U.FWD_CASES}
    for ks in U.MFMA2_KS:
        for layout in ("concat", "sum"):
            for R in (1, 16, 17, 127, 128):
                for D in (24, 520):
                    assert (ks, layout, R, D) in fw
    assert {(c.nq, c.T, c.dim, c.mode) for c in U.CA_CASES} == {(nq, T, dim, m) for nq, T in [(1, 1), (16, 2), (17, 16), (33, 3)]
                                                                for dim in (4, 68, 1028, 2052) for m in U.CA_MODES}
    assert {(c.dim, c.k, c.rows, c.g1) for c in U.DX_CASES} == {(d, k, r, g) for d in (64, 320, 576) for k in (20, 772)
                                                                for r in (1, 15, 17, 33) for g in (False, True)}
    names = [c.name for t in (U.FWD_CASES, U.BWD_CASES, U.DX_CASES, U.CA_CASES) for c in t]
    assert len(names) == len(set(names))


def test_operands_of_a_case_never_share_a_generator_seed():
    inp = U.Inputs("x")
    inp.t("a", 3, 17, 1028)
    inp.t("b", 3, 16, 1029)
    with pytest.raises(AssertionError):
        inp.t("a", 2, 2)
    for prob in [U.fwd_problem(U.FWD_CASES[0]), U.bwd_problem(U.BWD_CASES[0]), U.dx_problem(U.DX_CASES[0]),
                 U.ca_problem(U.CA_CASES[0])]:
        seeds = list(prob["seeds"].values())
        assert len(seeds) == len(set(seeds)) and len(seeds) >= 2
    # what the shape-summed seeds did: q (3, 17, 1028) and k (3, 16, 1028) came out correlated. Here they do not.
    p = U.ca_problem([c for c in U.CA_CASES if (c.nq, c.T, c.dim, c.mode) == (17, 16, 1028, "broad")][0])
    a, b = p["q"][:48].double().flatten(), p["k"][:48].double().flatten()
    n = min(a.numel(), b.numel())
    assert abs(float(torch.corrcoef(torch.stack([a[:n].sign(), b[:n].sign()]))[0, 1])) < 0.05


# ------------------------------------------------------------------------------ projections
@pytest.mark.parametrize("case", U.FWD_CASES, ids=lambda c: c.name)
def test_forward_reference_and_condition_a(case):
    p = U.fwd_problem(case)
    cat = torch.cat([x.double() for x in p["xs"]], 1) @ torch.cat([w.double() for w in p["ws"]], 1).T
    assert torch.allclose(p["ref"], cat, rtol=0, atol=1e-13)
    raw, tok = U.fwd_refs(case, p, True, 3)
    r = 4 % case.R
    assert torch.allclose(tok[r] - raw[r], p["temporal"][r % 3].double(), rtol=0, atol=1e-14)
    assert float(U.row_scales(case.R).min()) == 2.0 ** -min(case.R - 1, 6)
    for bias in (False, True):
        ref = U.fwd_refs(case, p, bias, None)[0]
        e, own = U.row_err(U.fwd_fp32(p, bias), ref, case.name), U.row_err(U.fwd_fp32(p, bias, torch_own=True), ref, case.name)
        print(f"[audio edges] {case.name} bias={bias} fp32 per row: {e:.3e} (condition {U.COND_A:.0e}); torch's matmul {own:.3e}")
        assert e < U.COND_A


@pytest.mark.parametrize("case", U.BWD_CASES, ids=lambda c: c.name)
def test_backward_reference_and_condition_a(case):
    p = U.bwd_problem(case)
    xs = [x.double() for x in p["xs"]]
    ws = [torch.zeros(case.D, k, dtype=torch.float64, requires_grad=True) for k in case.Ks]
    b = torch.zeros(case.D, dtype=torch.float64, requires_grad=True)
    g = p["g0"].double() + (p["g1"].double() if p["g1"] is not None else 0.0)
    (sum(x @ w.T for x, w in zip(xs, ws)) + b).backward(g)
    for o, k, w, ref, f32 in zip(p["dW_offs"], case.Ks, ws, p["dW_ref"], p["dW_fp32"]):
        assert torch.allclose(ref - p["dW_base"][:, o:o + k].double(), w.grad, rtol=0, atol=1e-13)
        e = U.row_err(f32, ref, case.name)
        assert e < U.COND_A, (case.name, e)
    if case.bias:
        assert torch.allclose(p["dbias_ref"] - p["dbias_base"][:case.D].double(), b.grad, rtol=0, atol=1e-13)
    if case.entry == "proj":
        t = torch.zeros(case.F, case.D, dtype=torch.float64, requires_grad=True)
        (t[torch.arange(case.R) % case.F]).backward(p["g0"].double())
        assert torch.allclose(p["dtemp_ref"] - p["dtemp_base"][:case.F].double(), t.grad, rtol=0, atol=1e-13)


@pytest.mark.parametrize("case", U.DX_CASES, ids=lambda c: c.name)
def test_dx_reference_and_condition_a(case):
    p = U.dx_problem(case)
    x = torch.zeros(case.rows, case.k, dtype=torch.float64, requires_grad=True)
    (x @ p["w"].double().T).backward(p["g0"].double() + (p["g1"].double() if case.g1 else 0.0))
    assert torch.allclose(p["ref"], x.grad, rtol=0, atol=1e-13)
    e = U.row_err(p["fp32"], p["ref"], case.name)
    assert e < U.COND_A, (case.name, e)


# ------------------------------------------------------------------------------ cross-attention
@pytest.mark.parametrize("case", U.CA_CASES + U.CA_BIG_CASES, ids=lambda c: c.name)
def test_cross_attention_restatement_and_condition_b(case):
    B, nq, T, dim = U.CA_B, case.nq, case.T, case.dim
    p = U.ca_problem(case)
    q, k, v = (p[n].double().requires_grad_() for n in ("q", "k", "v"))
    att = torch.softmax(q.view(B, nq, dim) @ k.view(B, T, dim).transpose(1, 2) / math.sqrt(dim), -1)
    x = (att @ v.view(B, T, dim)).reshape(B * nq, dim)
    x.backward(p["dx"].double())
    f = p["f64"]
    assert U.row_err(f["x"], x.detach()) < 1e-13
    if case.mode == "big":
        assert float(f["S"].amax(-1).min()) > 100.0               # without the maximum subtracted exp() overflows fp32 here
        assert float(f["P"].amax(-1).min()) >= 0.99 and p["own"]["x"] < U.COND_B
        return                                                    # forward only
    assert U.row_err(f["dv"], v.grad) < 1e-13
    assert U.den_err(f["dq"], q.grad, p["den_q"]) < 1e-13 and U.den_err(f["dk"], k.grad, p["den_k"]) < 1e-13
    assert bool((p["den_q"] > 0).all()) and bool((p["den_k"] > 0).all())
    if T == 1:                                                    # P = 1 and dS = 1 * (dP - dP): exact zeros in any precision
        assert bool((f["dq"] == 0).all()) and bool((f["dk"] == 0).all()) and torch.equal(f["x"], p["v"].double())
    if case.mode == "planted":
        for n, t in enumerate(p["planted"]):
            assert float(f["P"][n, :, t].min()) >= 0.99, (case.name, n, float(f["P"][n, :, t].min()))
    for name, e in p["own"].items():
        print(f"[audio edges] {case.name} fp32 restatement {name}: {e:.3e} -> bound {p['bound'][name]:.1e}")
        assert e < U.COND_B, (case.name, name, e)
        assert p["bound"][name] <= 4 * U.COND_B


def test_peaked_and_broad_cases_are_what_they_say():
    """broad: no key of a 16-key row above 0.5; peaked (q x 30): some row gives one key more than 0.9 — at dim 1028, where the
    scores are sums of many terms."""
    by = {(c.mode, c.nq, c.T, c.dim): c for c in U.CA_CASES}
    broad, peaked = U.ca_problem(by["broad", 17, 16, 1028]), U.ca_problem(by["peaked", 17, 16, 1028])
    assert float(broad["f64"]["P"].max()) < 0.5
    assert float(peaked["f64"]["P"].max()) > 0.9


def test_linear_bwd_takes_any_gradient_pitch():
    """fvqa_av_linear_bwd refused a gradient whose row pitch is no multiple of 4 floats (a contiguous g at dim = 21) although its
    kernel reads g element by element — fvqa_av_proj_bwd runs the same kernel at ldg = dim for any dim. Seen here without a
    launch: with a source of 4096 columns the call must get as far as that source's FVQA_ESHAPE, not stop at FVQA_EALIGN."""
    import ctypes as C

    from fvqa import _lib
    one, odd = C.c_void_p(256), C.c_void_p(260)
    src = (_lib.ProjSrc * 1)()
    src[0].x, src[0].w, src[0].ldx, src[0].ldw, src[0].k = 256, 256, 4096, 4096, 4096
    for which in ("bf16", "f16"):
        lib = _lib.load(which)
        assert lib.fvqa_av_linear_bwd(one, 21, C.addressof(src), 1, None, 80, 21, None) == -2
        assert lib.fvqa_av_linear_bwd(one, 29, C.addressof(src), 1, one, 80, 21, None) == -2
        assert lib.fvqa_av_linear_bwd(one, 20, C.addressof(src), 1, None, 80, 21, None) == -2     # ldg < dim
        assert lib.fvqa_av_linear_bwd(odd, 24, C.addressof(src), 1, None, 80, 21, None) == -3     # the pointers still 16 bytes
        assert lib.fvqa_av_linear_bwd(one, 24, C.addressof(src), 1, odd, 80, 21, None) == -3
