"""The three KV-cache attention kernels of the inference side — fvqa_attn_decode (csrc/attn_decode.hip, attn_decode_body.h),
fvqa_attn_suffix and fvqa_attn_suffix_append (csrc/score.hip) — against the fp64 oracle at every edge of their loops: one figure
per (row, head) vector of 128, max |got - ref| / max |ref| of that vector, held to the decode / suffix tests' own bounds
(3e-5 fp32, 1e-2 16-bit). Inputs and references come from tests/cached_attn_util.py (planted keys, decoys, NaN on every row a
kernel must not read); tests/test_cached_attn_edges_cpu.py checks those on the CPU. Figures of a run:
profiles/cached_attn_edges.log. Run with -m gpu -s."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from fvqa import ops  # noqa: E402
from tests import cached_attn_util as U  # noqa: E402

DEV = "cuda"
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
MODES = [(d, r) for d in DTYPES for r in (False, True)]
KEY_TOL = {torch.float32: 1e-6, torch.bfloat16: 8e-3, torch.float16: 8e-3}    # a stored key, tests/test_kernels_gpu.py's figure


def dev(x):
    return x.to(DEV).contiguous()


def held(what, got, want, dtype):
    """Per-row figure of `got` against the fp64 rows `want`, printed, then held to the bound of the storage type."""
    assert U.ref_floor(want) >= U.FLOOR, what
    assert bool(torch.isfinite(got.float()).all()), what
    worst = float(U.row_figures(got, want).max())
    print(f"{what}: worst row {worst:.3e} (bound {U.BOUND[dtype]:.1e})")
    assert worst < U.BOUND[dtype], what
    return worst


# ------------------------------------------------------------------------------------------------ fvqa_attn_decode
def decode_args(c):
    return (dev(c["g1"]), dev(c["g2"]), dev(c["vstart"]))


def run_decode(c, rot):
    """One launch; the output rows, and the cache checked: k (in the cache's convention) and v of the new tokens in rows
    n * S + pos[n], every other row and the q third of every row with the bits they had."""
    N, S, H, D = c["N"], c["S"], c["H"], c["D"]
    dtype = c["cache"].dtype
    cache_d = dev(c["cache"])
    o = torch.full((N, D), U.NAN, dtype=dtype, device=DEV)
    ops.attn_decode(dev(c["qkv_row"]), cache_d, o, *decode_args(c), dev(c["pos"]), (dev(c["cos"]), dev(c["sin"])),
                    N, S, H, U.DH, c["A"], c["F"], cache_rotated=rot)
    back, rows = cache_d.cpu(), c["rows"]
    keep = torch.ones(N * S + c["A"], dtype=torch.bool)
    keep[rows] = False
    assert torch.equal(U.bits(back[keep]), U.bits(c["cache"][keep]))
    assert torch.equal(U.bits(back[rows][:, :D]), U.bits(c["cache"][rows][:, :D]))
    assert torch.equal(U.bits(back[rows][:, 2 * D:]), U.bits(c["qkv_row"][:, 2 * D:]))
    k_got, k_want = back[rows][:, D:2 * D], c["full"][rows][:, D:2 * D]
    assert float(U.row_figures(k_got, k_want).max()) < KEY_TOL[dtype]
    if not rot:
        assert torch.equal(U.bits(k_got), U.bits(k_want))                  # raw keys: the token's own bits
    return o.cpu()


@pytest.mark.parametrize("dtype,rot", MODES)
def test_decode_position_sweep(dtype, rot):
    """S = 320, one launch, sixteen sequences: p = 0, both sides of the unrolled 128 keys, and both sides of every trip of the
    score loop (stride 64) and the value loop (stride 32) behind them; video_start absent, 0, 19 and around p."""
    c = U.sweep_case(dtype, rot)
    held(f"decode sweep {dtype} rot={rot}", run_decode(c, rot), c["want"], dtype)


@pytest.mark.parametrize("dtype,rot", MODES)
@pytest.mark.parametrize("A,F", U.AF_PAIRS)
def test_decode_bias_edge_and_adapter_lengths(A, F, dtype, rot):
    """S = 64: p = vs + F - 1 (unbiased) next to p = vs + F (biased), p = vs, p = S - 1, a window that runs over the end of the
    sequence and no window, at adapter lengths 1, 3, 10, 16 and frame counts 0, 6, 10, 16."""
    c = U.bias_edge_case(dtype, rot, A, F)
    held(f"decode bias edge A={A} F={F} {dtype} rot={rot}", run_decode(c, rot), c["want"], dtype)


@pytest.mark.parametrize("dtype,rot", MODES)
def test_decode_planted_keys(dtype, rot):
    """S = 320, one sequence per (p, j): key j carries >= 0.99 of the row's softmax — a kernel that skips j is wrong by the row.
    j = p is the token's own key (qkv_row); j = 15, 16 of p = 319 are frame keys of a biased row."""
    c = U.planted_decode_case(dtype, rot)
    assert len(c["weight"]) == c["N"] and all(float(w.min()) >= 0.99 for w in c["weight"].values())
    held(f"decode planted keys {dtype} rot={rot}", run_decode(c, rot), c["want"], dtype)


@pytest.mark.parametrize("j", U.LDS_J)
@pytest.mark.parametrize("dtype,rot", [m for m in MODES if m[0] != torch.float16])
def test_decode_at_the_lds_limit(dtype, rot, j):
    """S = 4096 = SMAX, the size of the score array in LDS: p = 4095 and 2079 against the one-row reference, key j planted."""
    c = U.lds_case(dtype, rot, j)
    assert c["weight"] and all(float(w.min()) >= 0.99 for w in c["weight"].values())
    held(f"decode S=4096 planted j={j} {dtype} rot={rot}", run_decode(c, rot), c["want"], dtype)


def test_decode_refuses_a_sequence_longer_than_the_lds_array():
    S, A, D = 4097, 10, U.DH
    cache = torch.zeros(S + A, 3 * D, device=DEV)
    row, o = torch.zeros(1, 3 * D, device=DEV), torch.zeros(1, D, device=DEV)
    g, vs, pos = torch.zeros(1, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int64, device=DEV)
    rope = (torch.zeros(S, U.DH // 2, device=DEV), torch.zeros(S, U.DH // 2, device=DEV))
    with pytest.raises(RuntimeError, match="FVQA_ESHAPE"):
        ops.attn_decode(row, cache, o, g, g, vs, pos, rope, 1, S, 1, U.DH, A, 10, cache_rotated=True)
    torch.cuda.synchronize()
    assert not bool(o.any()) and not bool(cache.any())


@pytest.mark.parametrize("dtype,rot", MODES)
def test_decode_reads_the_keys_it_stored(dtype, rot):
    """S = 160, prompts of 120, 127 and 144 tokens, sixteen calls on ONE cache, each at the next position: every call after the
    first reads keys that earlier calls stored. Output rows against the oracle over the whole sequences; the stored rows
    against the fp64-rotated keys rounded to storage; everything behind them still NaN."""
    L, steps = [120, 127, 144], 16
    c = U.store_read_case(dtype, rot, 160, 2, 10, 10, L, steps, seed=59)
    N, S, H, D = c["N"], c["S"], c["H"], c["D"]
    cache_d, rope, args = dev(c["cache"]), (dev(c["cos"]), dev(c["sin"])), decode_args(c)
    base_d = dev(c["base"])
    worst = 0.0
    for t in range(steps):
        pos = torch.tensor([ln + t for ln in L], dtype=torch.int64)
        o = torch.full((N, D), U.NAN, dtype=dtype, device=DEV)
        ops.attn_decode(base_d[torch.arange(N) * S + pos].contiguous(), cache_d, o, *args, dev(pos), rope, N, S, H, U.DH,
                        c["A"], c["F"], cache_rotated=rot)
        o = o.cpu()
        assert U.ref_floor(c["want"][t]) >= U.FLOOR and bool(torch.isfinite(o.float()).all())
        worst = max(worst, float(U.row_figures(o, c["want"][t]).max()))
    print(f"decode store-then-read {dtype} rot={rot}: worst row {worst:.3e} (bound {U.BOUND[dtype]:.1e})")
    assert worst < U.BOUND[dtype]
    back = cache_d.cpu()
    new = torch.zeros(N * S + c["A"], dtype=torch.bool)
    for n in range(N):
        new[n * S + L[n]:n * S + L[n] + steps] = True
    assert torch.equal(U.bits(back[~new]), U.bits(c["cache"][~new]))
    assert torch.equal(U.bits(back[new][:, :D]), U.bits(c["cache"][new][:, :D]))
    assert torch.equal(U.bits(back[new][:, 2 * D:]), U.bits(c["base"][new][:, 2 * D:]))
    assert float(U.row_figures(back[new][:, D:2 * D], c["k_want"][new[: N * S]]).max()) < KEY_TOL[dtype]
    if not rot:
        assert torch.equal(U.bits(back[new][:, D:2 * D]), U.bits(c["base"][new][:, D:2 * D]))      # raw keys: the tokens' own bits


# ------------------------------------------------------------------------------------------------ fvqa_attn_suffix
def suffix_args(c):
    return (dev(c["g1"]), dev(c["g2"]), dev(c["vstart"]), dev(c["start"]), dev(c["length"]), (dev(c["cos"]), dev(c["sin"])))


def run_suffix(what, c, rot):
    """Two launches with equal bits; the valid rows held to fp64 per row, the padding rows zeros, the cache untouched."""
    dtype = c["cache"].dtype
    cache_d, suf_d, args = dev(c["cache"]), dev(c["suf"]), suffix_args(c)
    outs = []
    for _ in range(2):
        o = torch.full((c["N"] * c["O"] * c["T"], c["D"]), U.NAN, dtype=dtype, device=DEV)
        ops.attn_suffix(suf_d, cache_d, o, *args, c["N"], c["O"], c["T"], c["S"], c["H"], U.DH, c["A"], c["F"], cache_rotated=rot)
        outs.append(o.cpu())
    got = outs[0]
    assert torch.equal(U.bits(outs[0]), U.bits(outs[1]))
    assert torch.equal(U.bits(cache_d.cpu()), U.bits(c["cache"]))
    assert not bool(got[~c["valid"]].float().any())
    held(what, got[c["valid"]], c["want"][c["valid"]], dtype)
    return got


@pytest.mark.parametrize("dtype,rot", MODES)
@pytest.mark.parametrize("i", range(len(U.T_CASES)))
def test_suffix_rows_that_do_not_fill_the_tiles(i, dtype, rot):
    """T = 7, 12, 5, 15 (and 16 and 1): tiles of 32 queries that see two chunks of suffix keys, start in the middle of an option
    or span three options — fvqa/score.py sets T to the longest answer of the batch, whatever it is."""
    c = U.t_case(dtype, rot, i)
    run_suffix(f"suffix T case {U.T_CASES[i][:5]} {dtype} rot={rot}", c, rot)


@pytest.mark.parametrize("dtype,rot", MODES)
def test_suffix_start_edges(dtype, rot):
    """T = 4, O = 5, S = 128: an empty prompt, a prompt of one key, prompts that end on and around a chunk of 32 keys, a suffix
    that the end of the sequence cuts to one row, and a sample with no suffix rows (zeros)."""
    c = U.start_edge_case(dtype, rot)
    got = run_suffix(f"suffix start edges {dtype} rot={rot}", c, rot).view(c["N"], -1)
    assert not bool(got[8].float().any())


@pytest.mark.parametrize("dtype,rot", MODES)
@pytest.mark.parametrize("A,F", U.AF_PAIRS)
def test_suffix_frame_window_against_the_suffix(A, F, dtype, rot):
    """T = 16, O = 2: the frame window ends inside the suffix (rows behind it are biased, on prompt keys and on suffix keys),
    straddles the start of the suffix, lies inside the suffix, or is absent."""
    c = U.frame_window_case(dtype, rot, A, F)
    run_suffix(f"suffix frame window A={A} F={F} {dtype} rot={rot}", c, rot)


@pytest.mark.parametrize("dtype,rot", MODES)
@pytest.mark.parametrize("kind", U.PLANT_KINDS)
@pytest.mark.parametrize("i,tile", [(i, t) for i, ts in U.PLANT_TILES.items() for t in ts])
def test_suffix_planted_keys_and_decoys(i, tile, kind, dtype, rot):
    """One query of the first or the last tile — or, T = 15, query 63, whose own rows lie in its tile's second chunk of suffix
    keys — gets a planted key: prompt row 31, 32 or start - 1, its own option's row 0, its own row or the row in front of it;
    and decoys everywhere it must not look: the same row of the neighbouring options, the next row of its own
    option, and cache row `start`."""
    c = U.t_case(dtype, rot, i, plant=(kind, tile))
    assert float(c["plant"]["weight"].min()) >= 0.99
    run_suffix(f"suffix planted {kind} {tile} tile, T case {U.T_CASES[i][:5]} {dtype} rot={rot}", c, rot)


# ------------------------------------------------------------------------------------------------ fvqa_attn_suffix_append
@pytest.mark.parametrize("dtype,rot", MODES)
@pytest.mark.parametrize("start", U.APPEND_STARTS)
@pytest.mark.parametrize("T", [1, 7, 16])
def test_append_three_ways_and_against_fp64(T, start, dtype, rot):
    """S = 160, prompts that end on both sides of the 128 unrolled keys of the decode kernel and of a chunk of the suffix
    kernel, an empty one and one with a single free row: the cache holds the bits fvqa_attn_decode stores, the output the bits
    of fvqa_attn_suffix with one option, nothing else moved — and the output rows are the oracle's."""
    c = U.append_case(dtype, rot, T, start)
    N, S, H, D = c["N"], c["S"], c["H"], c["D"]
    L = U.eff_len(S, start, c["length"].tolist())
    suf_d, args = dev(c["suf"]), suffix_args(c)
    shape = (N, T, S, H, U.DH, c["A"], c["F"])
    cache_d = dev(c["cache"])
    o = torch.full((N * T, D), U.NAN, dtype=dtype, device=DEV)
    ops.attn_suffix_append(suf_d, cache_d, o, *args, *shape, cache_rotated=rot)
    # the same raw rows one by one through attn_decode, each on a cache of its own
    want = c["cache"].clone()
    for j in range(T):
        scratch = dev(c["cache"])
        pos = torch.tensor([min(s + j, S - 1) for s in start], dtype=torch.int64, device=DEV)
        ops.attn_decode(suf_d.view(N, T, 3 * D)[:, j].contiguous(), scratch, torch.empty(N, D, dtype=dtype, device=DEV), *args[:3],
                        pos, args[5], N, S, H, U.DH, c["A"], c["F"], cache_rotated=rot)
        scratch = scratch.cpu()
        for n in range(N):
            if j < L[n]:
                want[n * S + start[n] + j, D:] = scratch[n * S + start[n] + j, D:]
    o_one = torch.full((N * T, D), U.NAN, dtype=dtype, device=DEV)
    ops.attn_suffix(suf_d, dev(c["cache"]), o_one, *args, N, 1, T, S, H, U.DH, c["A"], c["F"], cache_rotated=rot)
    back, got = cache_d.cpu(), o.cpu()
    assert torch.equal(U.bits(back), U.bits(want))
    assert int((U.bits(back) != U.bits(c["cache"])).any(1).sum()) == sum(L)
    assert torch.equal(U.bits(back[:, :D]), U.bits(c["cache"][:, :D]))
    assert torch.equal(U.bits(got), U.bits(o_one.cpu()))
    assert not bool(got[~c["valid"]].float().any())
    held(f"append T={T} start={start} {dtype} rot={rot}", got[c["valid"]], c["want"][c["valid"]], dtype)
