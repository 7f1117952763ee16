"""Frame attention on the GPU: the two summary kernels — fvqa_attn_decode_mass, fvqa_attn_row_mass (csrc/attn_decode.hip,
attn_decode_body.h) — against the fp64 text weights of tests/cached_attn_util.py at every edge its decode cases build, and
`generate(frame_attention=True)` end to end against the reference's own probabilities (tests/golden/attn_mass_tiny_peakedperm.npz,
tools/gen_golden_attention.py) and against a host-side fp64 summary of a teacher-forced dense forward, which runs neither kernel.

Kernel bound: every entry within 3e-5 absolute of the fp64 summary, in every storage type (q and k are rounded to the storage
type on both sides; what remains is fp32 arithmetic, BOUND[float32] of the util). End-to-end bound b, per build: 4 x the distance
of the host summary of the EXISTING prefill arena, teacher-forced on the fixture's ids, from the fixture, and not below 3e-5 —
measured before the feature was written (profiles/frame_attention.log), see E2E_FIGURE. Run with -m gpu -s for the figures."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from fvqa import attribution, generate, ops  # noqa: E402
from tests import cached_attn_util as U  # noqa: E402
from tests.test_eval import GOLDS, golden_batch  # noqa: E402
from tests.test_generate_gpu import GEN_EOS, model_of  # noqa: E402

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
MODES = [(d, r) for d in DTYPES for r in (False, True)]
BOUND = 3e-5
FIX = dict(np.load(os.path.join(ROOT, "tests", "golden", "attn_mass_tiny_peakedperm.npz")))
# max |host fp64 summary of the prefill arena, teacher-forced on the fixture's ids - fixture|, per build, as measured on the
# tree BEFORE the kernels existed (profiles/frame_attention.log); b = max(4 x figure, 3e-5)
E2E_FIGURE = {torch.float32: 1.444e-07, torch.bfloat16: 5.128e-04, torch.float16: 7.877e-05}      # b: 3e-5, 2.051e-3, 3.151e-4


def e2e_bound(dtype):
    return max(4 * E2E_FIGURE[dtype], BOUND)


def dev(x):
    return x.to(DEV).contiguous()


# ------------------------------------------------------------------------------------------------ the summary, on the host
def summary(pt, vs, F, p):
    """pt (H, p + 1) text weights of the row at position p -> (H, F + 2): the issue's definition, term by term."""
    H = pt.shape[0]
    out = torch.zeros(H, F + 2, dtype=pt.dtype)
    if vs < 0:
        out[:, F + 1] = pt.sum(-1)
        return out
    for f in range(F):
        if vs + f <= p:
            out[:, f] = pt[:, vs + f]
    out[:, F] = pt[:, :min(vs, p + 1)].sum(-1)
    out[:, F + 1] = pt[:, vs + F:p + 1].sum(-1)
    return out


def case_reference(c, rot):
    """The fp64 summary (N, H, F + 2) of a decode case of the util, through its one_row_ref: the rotated, rounded query and keys
    are rebuilt from what the case holds (`full`: the sequences as a prefill would leave them, k in the cache's convention)."""
    N, S, H, A, F, D = c["N"], c["S"], c["H"], c["A"], c["F"], c["D"]
    dtype = c["full"].dtype
    _, _, c64, s64 = U.tables(S)
    seqs = c["full"][: N * S].view(N, S, 3, H, U.DH)
    ak = c["full"][N * S:, D:2 * D].double().view(A, H, U.DH)
    av = c["full"][N * S:, 2 * D:].double().view(A, H, U.DH)
    want = torch.empty(N, H, F + 2, dtype=torch.float64)
    qhats = []
    for n in range(N):
        p, vs = int(c["pos"][n]), int(c["vstart"][n])
        qhat = U.rot_rows(seqs[n, p, 0].double(), p, c64, s64).to(dtype).double()
        kr = seqs[n, :, 1].double() if rot else U.rotated_rounded(seqs[n:n + 1, :, 1], c64, s64, dtype)[0]
        _, pt = U.one_row_ref(qhat, kr, seqs[n, :, 2].double(), ak, av, c["g1"].double(), c["g2"].double(), vs, F, p)
        want[n] = summary(pt, vs, F, p)
        qhats.append(qhat)
    return want, torch.stack(qhats)


def launch_decode(c, rot, mass=None):
    N, S, H, D = c["N"], c["S"], c["H"], c["D"]
    dtype = c["cache"].dtype
    cache = dev(c["cache"])
    o = torch.full((N, D), U.NAN, dtype=dtype, device=DEV)
    args = (dev(c["g1"]), dev(c["g2"]), dev(c["vstart"]), dev(c["pos"]), (dev(c["cos"]), dev(c["sin"])), N, S, H, U.DH, c["A"],
            c["F"])
    if mass is None:
        ops.attn_decode(dev(c["qkv_row"]), cache, o, *args, cache_rotated=rot)
    else:
        ops.attn_decode_mass(dev(c["qkv_row"]), cache, o, mass, *args, cache_rotated=rot)
    return o.cpu(), cache.cpu()


def check_case(what, c, rot):
    """Both kernels on one case of the util -> (decode's mass, the fp64 summary), after every check that holds for all cases."""
    N, S, H, F, D = c["N"], c["S"], c["H"], c["F"], c["D"]
    dtype = c["cache"].dtype
    want, qhat = case_reference(c, rot)
    assert float((want.sum(-1) - 1).abs().max()) < 1e-12
    new = lambda: torch.full((N, H, F + 2), U.NAN, dtype=torch.float32, device=DEV)      # noqa: E731
    m1, m2 = new(), new()
    o0, cache0 = launch_decode(c, rot)
    o1, cache1 = launch_decode(c, rot, m1)
    launch_decode(c, rot, m2)
    assert torch.equal(U.bits(o0), U.bits(o1)) and torch.equal(U.bits(cache0), U.bits(cache1)), what      # fvqa_attn_decode's bits
    assert torch.equal(U.bits(m1.cpu()), U.bits(m2.cpu())), what                                          # two launches, one result
    # the rows as an arena holds them: the query row in the cache's convention at pos, NaN behind it
    arena = c["cache"].clone()
    arena[c["rows"]] = c["full"][c["rows"]]
    if rot:
        arena[c["rows"], :D] = qhat.reshape(N, D).to(dtype)
    m3, m4 = torch.full_like(m1, U.NAN), torch.full_like(m1, U.NAN)
    arena_d = dev(arena)
    for m in (m3, m4):
        ops.attn_row_mass(arena_d, torch.arange(N, dtype=torch.int32, device=DEV), dev(c["pos"].to(torch.int32)), m, dev(c["g2"]),
                          dev(c["vstart"]), (dev(c["cos"]), dev(c["sin"])), N, S, H, U.DH, c["A"], F, cache_rotated=rot)
    assert torch.equal(U.bits(arena_d.cpu()), U.bits(arena))                                              # nothing stored
    assert torch.equal(U.bits(m3.cpu()), U.bits(m4.cpu())), what
    got, got_row = m1.cpu().double(), m3.cpu().double()
    assert bool(torch.isfinite(got).all()) and bool(torch.isfinite(got_row).all()), what
    e1, e2, e3 = (float((a - b).abs().max()) for a, b in ((got, want), (got_row, want), (got, got_row)))
    print(f"{what}: decode_mass {e1:.2e}, row_mass {e2:.2e}, one against the other {e3:.2e}, sums off 1 by "
          f"{float((got.sum(-1) - 1).abs().max()):.1e} (bound {BOUND:.0e})")
    assert e1 <= BOUND and e2 <= BOUND and e3 <= BOUND, what
    for n in range(N):                                       # exact zeros: beyond p, and every frame entry without a window
        p, vs = int(c["pos"][n]), int(c["vstart"][n])
        dead = [f for f in range(F) if vs < 0 or vs + f > p]
        assert not bool(m1[n, :, dead].any()) and not bool(m3[n, :, dead].any()), (what, n)
        if vs < 0:
            assert not bool(m1[n, :, F].any()) and not bool(m3[n, :, F].any()), (what, n)
    return got, want


# ------------------------------------------------------------------------------------------------ the kernels
@pytest.mark.parametrize("dtype,rot", MODES)
def test_position_sweep(dtype, rot):
    """S = 320: p = 0, 1, 15 ... 319 — both sides of the 128 unrolled keys and of every trip of the score loop —, video_start
    absent, 0, 19 and a window that holds p (some of its keys beyond p: exact zeros)."""
    check_case(f"mass sweep {dtype} rot={rot}", U.sweep_case(dtype, rot), rot)


@pytest.mark.parametrize("dtype,rot", MODES)
@pytest.mark.parametrize("A,F", U.AF_PAIRS)
def test_bias_edge_and_window_shapes(A, F, dtype, rot):
    """S = 64: p = vs + F - 1 (unbiased) next to vs + F (biased), p = vs, p = S - 1, a window that runs over the end of the row,
    no window; F = 0 (a summary of two entries), F = 16, A = 1 .. 16."""
    check_case(f"mass bias edge A={A} F={F} {dtype} rot={rot}", U.bias_edge_case(dtype, rot, A, F), rot)


@pytest.mark.parametrize("dtype,rot", MODES)
def test_planted_keys_show_where_they_are(dtype, rot):
    """One key per row carries >= 0.99 of the text softmax: a frame key of a biased row (window [10, 20), p = 319) and of an
    unbiased one ((128, 127), window [120, 130)) in its own entry, every other one in front of or behind the window."""
    c = U.planted_decode_case(dtype, rot)
    got, _ = check_case(f"mass planted keys {dtype} rot={rot}", c, rot)
    pairs, _ = U.plant_pairs()
    F, seen = c["F"], set()
    assert all(float(w.min()) >= 0.99 for w in c["weight"].values())
    for n, (p, j) in enumerate(pairs):
        vs = int(c["vstart"][n])
        at = F + 1 if vs < 0 or j >= vs + F else F if j < vs else j - vs
        seen.add("frame" if at < F else "front" if at == F else "behind")
        assert float(got[n, :, at].min()) >= 0.99, (n, p, j, vs, at)
        if at < F:
            assert (p >= vs + F) == (p == 319)
    assert seen == {"frame", "front", "behind"}
    assert int(c["vstart"][pairs.index((128, 127))]) == 120 and int(c["vstart"][pairs.index((319, 15))]) == 10


@pytest.mark.parametrize("dtype,rot", [m for m in MODES if m[0] != torch.float16])
def test_at_the_lds_limit(dtype, rot):
    """S = 4096 = SMAX: p = 4095 with a planted frame key behind key 2047 (window [2040, 2050)), and p = 2079 with the window
    [2075, 2085) half visible."""
    c = U.decode_case(dtype, rot, 4096, 1, 10, 10, [4095, 2079], [2040, 2075], 53, plants=[(0, 2048)], oracle=False)
    got, want = check_case(f"mass S=4096 {dtype} rot={rot}", c, rot)
    assert float(want[0, :, 8].min()) > 0.5 and float(got[0, :, 8].min()) > 0.5          # the planted key is frame 8
    assert float(want[1, :, :5].min()) > 0 and not bool(got[1, :, 5:10].any())


def test_operands_are_checked_on_the_host():
    S, A, H, F, D = 64, 10, 1, 10, U.DH
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=DEV)      # noqa: E731
    cache, row, o, g = z(S + A, 3 * D), z(1, 3 * D), z(1, D), z(H)
    vs, pos, rope = z(1, dt=torch.int32), z(1, dt=torch.int64), (z(S, D // 2), z(S, D // 2))
    for mass in (z(1, H, F + 1), z(1, H, F + 2, dt=torch.float64), z(2, H, F + 2)):
        with pytest.raises(ValueError, match="mass"):
            ops.attn_decode_mass(row, cache, o, mass, g, g, vs, pos, rope, 1, S, H, D, A, F, cache_rotated=True)
    with pytest.raises(ValueError, match="device"):
        ops.attn_decode_mass(row, cache, o, torch.zeros(1, H, F + 2), g, g, vs, pos, rope, 1, S, H, D, A, F, cache_rotated=True)
    i32 = z(3, dt=torch.int32)
    for seq, p, mass in ((i32, i32[:2], z(3, H, F + 2)), (i32.long(), i32, z(3, H, F + 2)), (i32, i32, z(3, H, F + 1)),
                         (i32[:0], i32[:0], z(0, H, F + 2))):
        with pytest.raises(ValueError, match="attn_row_mass"):
            ops.attn_row_mass(cache, seq, p, mass, g, vs, rope, 1, S, H, D, A, F, cache_rotated=True)
    with pytest.raises(ValueError, match="attention"):
        ops.attn_row_mass(cache[:-1], i32, i32, z(3, H, F + 2), g, vs, rope, 1, S, H, D, A, F, cache_rotated=True)
    big = 4097
    with pytest.raises(RuntimeError, match="FVQA_ESHAPE"):
        ops.attn_row_mass(z(big + A, 3 * D), i32, i32, z(3, H, F + 2), g, vs, (z(big, D // 2), z(big, D // 2)), 1, big, H, D, A, F,
                          cache_rotated=True)


# ------------------------------------------------------------------------------------------------ end to end
def host_mass(eng, p, rows):
    """The summary in torch fp64 on the host from the arena a dense forward left (p: generate._prefill's result): rows
    [(b, position)] -> (len(rows), L, H, F + 2). Neither summary kernel runs: q and k are read from the arena (rotated here in
    fp64 and rounded to the storage type where the arena holds them raw), scored, biased, soft-maxed and summed here."""
    S, H, F, D = p.S, eng.H, eng.F, eng.D
    qkv = p.ar.qkv.cpu()
    vstart = p.vstart.cpu().tolist()
    c64, s64 = eng.cos.cpu().double(), eng.sin.cpu().double()
    out = torch.zeros(len(rows), eng.L, H, F + 2, dtype=torch.float64)
    for i in range(eng.L):
        g2 = eng.model.gate_views(i)[1].detach().cpu().double()
        for r, (b, pos) in enumerate(rows):
            seq = qkv[i, b * S:(b + 1) * S].view(S, 3, H, U.DH)
            q, k = seq[pos, 0].double(), seq[: pos + 1, 1].double()
            if not p.rotated:
                q = U.rot_rows(q, pos, c64, s64).to(qkv.dtype).double()
                k = U.rot_rows(k, torch.arange(pos + 1)[:, None], c64, s64).to(qkv.dtype).double()
            s = torch.einsum("hd,thd->ht", q, k) / math.sqrt(U.DH)
            vs = vstart[b]
            if vs >= 0 and pos >= vs + F:
                s[:, vs:vs + F] += g2[:, None]
            out[r, i] = summary(torch.softmax(s, -1), vs, F, pos)
    return out


def teacher_forced(eng, batch, ids):
    """One dense forward of the existing route on the given id rows -> generate._prefill's result (the arena, vstart, rotated)."""
    data = dict(batch, text_id={"vqa": ids.cpu().unsqueeze(1)}, label={"vqa": batch["label"]["vqa"][:, 0:1]})
    return generate._prefill(eng, data)


PREMISE_MARGIN = {torch.float32: 4, torch.float16: 4, torch.bfloat16: 1}      # tools/gen_golden_attention.py BOUNDS


def misplaced_is_seen(got, ref, b):
    """got, ref (B, T, L, H, F + 2): the share of the ordered pairs of neighbouring (step, layer, head) entries (e, e') in which
    got[e] differs from ref[e'] by more than b in some component — a summary delivered one step, layer or head off its place
    is refused by the bound."""
    miss = []
    for ax in (1, 2, 3):
        n = got.shape[ax]
        lo, hi = torch.arange(n - 1), torch.arange(1, n)
        for a, c in ((lo, hi), (hi, lo)):
            d = (got.index_select(ax, a) - ref.index_select(ax, c)).abs().amax(-1)
            miss.append((d > b).reshape(-1))
    return float(torch.cat(miss).double().mean())


def answer_rows(prefix, n_new=31):
    return [(b, int(p) - 1 + t) for b, p in enumerate(prefix) for t in range(n_new)]


@pytest.mark.parametrize("dtype", DTYPES)
def test_generate_against_the_reference_fixture(dtype):
    """tiny_peakedperm: generate's summary of each of the 31 answer rows per sample against the reference's own text softmax
    (fixture) and against the host summary of a teacher-forced dense forward on the returned ids, which is itself held to the
    fixture — three sources, two of them without the new kernels.
    Measured (profiles/frame_attention.log): generate - fixture 1.79e-07 fp32, 5.58e-04 bf16, 7.87e-05 fp16 against b = 3.0e-05,
    2.05e-03, 3.15e-04.
    What makes the bound see a summary read at the wrong step, layer or head is asserted twice, for every build. The premise:
    neighbouring (step, layer, head) entries of the fixture lie more than PREMISE_MARGIN x b apart in at least 90 % of the pairs —
    4 b for fp32 (100 %) and fp16 (97.6 %); for the bf16 build's b no committed eval configuration reaches 90 % at 4 b (this one
    79.5 %, the best 82.3 %; tools/gen_golden_attention.py lists all six), so 1 b is held there (95.2 %): the neighbour's own
    reference summary misses the bound. And the consequence itself (`misplaced_is_seen`): generate's summary of an entry, held
    against the fixture's NEIGHBOURING entry, misses b in at least 90 % of the pairs."""
    m = model_of("tiny_peakedperm", dtype)
    eng = m.ensure_engine()
    G = GOLDS["tiny_peakedperm"]
    assert np.array_equal(G["text_id_vqa"], FIX["text_id_vqa"]) and np.array_equal(G["prefix_vqa"], FIX["prefix_vqa"])
    batch = golden_batch(G)
    out = generate.generate(eng, batch, frame_attention=True, stop_at_eos=False, max_new_tokens=31)
    fa = out["frame_attention"]
    B, L, H, F = 4, eng.L, eng.H, eng.F
    assert tuple(fa.shape) == (B, 31, L, H, F + 2) and fa.dtype == torch.float32 and out["steps"] == 31
    assert np.array_equal(out["ids"].cpu().numpy(), FIX["ids_after"])
    p = teacher_forced(eng, batch, out["ids"])
    host = host_mass(eng, p, answer_rows(G["prefix_vqa"])).view(B, 31, L, H, F + 2)
    fix, got = torch.from_numpy(FIX["mass"]).double(), fa.cpu().double()
    b = e2e_bound(dtype)
    e_host, e_fix, e_gh = (float((x - y).abs().max()) for x, y in ((host, fix), (got, fix), (got, host)))
    sep = np.concatenate([FIX[k].reshape(-1) for k in ("sep_step", "sep_layer", "sep_head")])
    print(f"frame attention tiny_peakedperm {dtype}: host - fixture {e_host:.2e}, generate - fixture {e_fix:.2e}, generate - host "
          f"{e_gh:.2e} (b = {b:.1e}); neighbouring fixture entries more than 4 b apart: {float((sep > 4 * b).mean()):.3f}")
    assert float((got.sum(-1) - 1).abs().max()) < 1e-5
    assert e_host <= b and e_fix <= b and e_gh <= b
    seen = misplaced_is_seen(got, fix, b)
    print(f"    more than {PREMISE_MARGIN[dtype]} b apart: {float((sep > PREMISE_MARGIN[dtype] * b).mean()):.3f}; a neighbour's "
          f"entry misses b: {seen:.3f}")
    assert float((sep > PREMISE_MARGIN[dtype] * b).mean()) >= 0.9
    assert seen >= 0.9


@pytest.mark.parametrize("dtype", DTYPES)
def test_generate_against_a_teacher_forced_forward_at_7b_width(dtype):
    """7b_l2_peakedperm (32 heads, D = 4096), no fixture: generate's summary of all 31 answer rows per sample against the host
    summary of a dense forward, and a neighbour's host entry must miss the bound as above."""
    m = model_of("7b_l2_peakedperm", dtype)
    eng = m.ensure_engine()
    G = GOLDS["7b_l2_peakedperm"]
    batch = golden_batch(G)
    out = generate.generate(eng, batch, frame_attention=True, stop_at_eos=False, max_new_tokens=31)
    assert np.array_equal(out["ids"].cpu().numpy(), G["ids_after"])
    p = teacher_forced(eng, batch, out["ids"])
    host = host_mass(eng, p, answer_rows(G["prefix_vqa"])).view(4, 31, eng.L, eng.H, eng.F + 2)
    got = out["frame_attention"].cpu().double()
    err, b = float((got - host).abs().max()), e2e_bound(dtype)
    seen = misplaced_is_seen(got, host, b)
    print(f"frame attention 7b_l2_peakedperm {dtype}: generate - host {err:.2e} (b = {b:.1e}); a neighbour's entry misses b: "
          f"{seen:.3f}")
    assert float((out["frame_attention"].sum(-1) - 1).abs().max()) < 1e-5
    assert err <= b and seen >= 0.9


def same_but_for_the_keyword(eng, batch, **kw):
    off = generate.generate(eng, batch, **kw)
    on = generate.generate(eng, batch, frame_attention=True, **kw)
    assert set(on) == set(off) | {"frame_attention"} and on["steps"] == off["steps"]
    for k in ("ids", "tokens", "logprobs", "n_generated", "choice"):
        if k in off:
            assert torch.equal(on[k], off[k]), k
    fa, tok = on["frame_attention"], on["tokens"]
    assert tuple(fa.shape) == tuple(tok.shape) + (eng.L, eng.H, eng.F + 2) and fa.dtype == torch.float32
    assert not bool(fa[tok == -1].any())
    live = fa[tok != -1]
    assert live.numel() and float((live.sum(-1) - 1).abs().max()) < 1e-5
    return on


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_the_keyword_changes_no_token(dtype):
    """EOS stops, constraints, and sampling with top_k and three samples per prompt: ids, tokens and log-probabilities are those
    of the call without the keyword, bit for bit; the summary has the tokens' shape and is zero where there is no token."""
    m = model_of("tiny_peakedperm", dtype)
    eng = m.ensure_engine()
    G = GEN_EOS["tiny"]
    batch = golden_batch(G)
    on = same_but_for_the_keyword(eng, batch, temperature=0.0, stop_at_eos=True, max_new_tokens=31, return_logprobs=True)
    assert on["n_generated"].tolist() == G["eos_k"].tolist() and bool((on["tokens"] == -1).any())
    first = attribution.arena_mass(eng, 4, 128, torch.arange(4), torch.from_numpy(G["prefix_vqa"]) - 1)     # (the last prefill's)
    assert tuple(first.shape) == (eng.L, 4, eng.H, eng.F + 2)
    cons = [[5, 6, 7], [5, 9], [11, 12, 13, 14]]
    on = same_but_for_the_keyword(eng, batch, temperature=0.0, max_new_tokens=8, constraints=cons, return_logprobs=True)
    assert all(0 <= c < 3 for c in on["choice"].tolist())
    on = same_but_for_the_keyword(eng, batch, temperature=0.9, top_k=50, top_p=0.95, seed=5, num_return_sequences=3,
                                  repetition_penalty=1.2, max_new_tokens=6, return_logprobs=True)
    fa = on["frame_attention"]
    assert tuple(fa.shape[:3]) == (4, 3, on["steps"])
    assert torch.equal(fa[:, 0, 0], fa[:, 1, 0]) and torch.equal(fa[:, 0, 0], fa[:, 2, 0])      # index 0: the prefill row, repeated
    s = attribution.summarize(on)
    assert tuple(s["frame_share"].shape) == (4, 3, eng.F) and tuple(s["video_mass"].shape) == (4, 3)
    assert float(s["video_mass"].min()) > 0 and float(s["video_mass"].max()) < 1


def test_refusals():
    m = model_of("tiny_peakedperm", torch.float32)
    eng = m.ensure_engine()
    batch = golden_batch(GOLDS["tiny_peakedperm"])
    for kw, word in ((dict(num_beams=2), "num_beams"), (dict(contrast="blind"), "contrast"), (dict(lookahead=4), "lookahead"),
                     (dict(constraints=[[5, 6]], jump_forward=4), "jump_forward")):
        with pytest.raises(ValueError, match="frame_attention is not built for " + word):
            generate.generate(eng, batch, frame_attention=True, **kw)
    import inspect
    from fvqa import stream
    assert "frame_attention" not in inspect.signature(stream.generate_stream).parameters
    with pytest.raises(ValueError, match="frame_attention"):
        attribution.summarize({"tokens": torch.zeros(1, 1)})


def test_the_model_and_validation_report_it(tmp_path):
    import engine
    import types
    m = model_of("tiny_peakedperm", torch.float32)
    G = GEN_EOS["tiny"]
    batch = golden_batch(G)
    m.generate(batch, max_new_tokens=5, frame_attention=True)
    g = m.last_generation
    assert tuple(g["frame_attention"].shape)[:2] == (4, g["steps"]) and "tokens" in g
    m.generate(batch, max_new_tokens=5)
    assert "frame_attention" not in m.last_generation and "tokens" not in m.last_generation
    opt = types.SimpleNamespace(param_groups=[{"lr": 0.25}])
    args = types.SimpleNamespace(is_generation_task=True, dataset="nextqa", debug=False, output_dir=str(tmp_path),
                                 gen_frame_attention=True)
    m.args.gen_stop_eos, m.args.gen_frame_attention = True, True
    try:
        stats = engine.val_one_epoch(m, [golden_batch(G)], opt, epoch=1, args=args)
        share = m.last_generation["frame_share"]
    finally:
        m.args.gen_stop_eos, m.args.gen_frame_attention = False, False
    rows = json.load(open(tmp_path / "extracted_answers" / "extracted_answers_epoch1.json"))
    assert len(rows) == 4 and all(len(r["frame_share"]) == 10 for r in rows)
    assert np.allclose([r["frame_share"] for r in rows], share.cpu().numpy(), atol=1e-7)
    assert stats["video_mass"] == pytest.approx(float(share.sum(-1).mean()), abs=1e-6) and 0 < stats["video_mass"] < 1


def test_answer_py_prints_the_frame_shares(tmp_path):
    clip = tmp_path / "clip.npy"
    np.save(clip, np.random.default_rng(0).standard_normal((14, 768)).astype(np.float32))
    r = subprocess.run([sys.executable, "answer.py", "--random_init", "--synthetic", "--question", "what is the man doing",
                        "--features", str(clip), "--max_new_tokens", "4", "--frame_attention", "--json", str(tmp_path / "a.json")],
                       cwd=os.path.join(ROOT, "flipped-vqa_amd"), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("frame shares ")]
    assert len(line) == 1
    left, right = line[0][len("frame shares "):].split(" | video mass ")
    shares = [float(x) for x in left.split()]
    assert len(shares) == 10 and all(0 <= x <= 1 for x in shares) and abs(sum(shares) - float(right)) < 1e-3
    rec = json.load(open(tmp_path / "a.json"))
    assert len(rec) == 1 and len(rec[0]["frame_share"]) == 10 and abs(rec[0]["video_mass"] - float(right)) < 1e-4
