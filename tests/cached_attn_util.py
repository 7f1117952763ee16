"""Helpers of the KV-cache attention edge tests (tests/test_cached_attn_edges_gpu.py, checked on the CPU by
tests/test_cached_attn_edges_cpu.py): inputs and fp64 references for fvqa_attn_decode, fvqa_attn_suffix and
fvqa_attn_suffix_append, built on the CPU only.

The reference is oracle/ref_cpu.attn_fwd on rotated operands whose q and k are rounded to the storage type first — the kernels'
stated contract — or, where the whole (S, S) oracle is too large, `one_row_ref`, the same formula at one query row.

A PLANTED key is a key whose rotated value is 16 * sqrt(128) / (q.q) * q for a chosen query q (rotated, rounded): its score is
16 against about +-1 for every other key, so it carries >= 0.99 of the softmax and a kernel that drops it is off by the whole
row, whatever the storage type. A DECOY is the same with score 30 on a key the query must NOT see: the reference never
reads it, a kernel that leaks it is off by about 100 %."""
import math

import torch

from oracle import ref_cpu

DH = 128
PLANT, DECOY = 16.0, 30.0
FLOOR = 1e-2                          # no reference vector may be smaller than this: the per-row figure divides by it
BOUND = {torch.float32: 3e-5, torch.bfloat16: 1e-2, torch.float16: 1e-2}      # the decode / suffix tests' own bounds, per row here
NAN = float("nan")


def rnd(*shape, dtype=torch.float32, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(*shape, generator=g, dtype=torch.float64) * 2 - 1).to(dtype)


def bits(t):
    return t.contiguous().view(torch.uint8)


def tables(S):
    """cos, sin (S, 64) fp32 — what the kernels are handed — and their fp64 widenings for the reference."""
    cos, sin = ref_cpu.rope_tables(S, DH, torch.float32)
    return cos, sin, cos.double(), sin.double()


def rot_rows(x, pos, c64, s64, inverse=False):
    """x (..., DH) fp64, rotated at position pos (an int, or a tensor broadcastable to x's leading dims)."""
    c, s = c64[pos], s64[pos]
    if inverse:
        s = -s
    e, o = x[..., 0::2], x[..., 1::2]
    out = torch.empty_like(x)
    out[..., 0::2] = e * c - o * s
    out[..., 1::2] = e * s + o * c
    return out


def rotated_rounded(t, c64, s64, dtype):
    """t (N, S, H, DH) in the storage type -> RoPE in fp64, rounded to the storage type, as fp64."""
    return ref_cpu.rope_apply(t.double(), c64[: t.shape[1]], s64[: t.shape[1]]).to(dtype).double()


def planted(qhat, score):
    """The rotated key that scores `score` against the rotated, rounded query qhat (..., DH) and about +-1 against others."""
    return score * math.sqrt(DH) / (qhat * qhat).sum(-1, keepdim=True) * qhat


def row_figures(got, ref):
    """One figure per (row, head) vector of 128: max |got - ref| / max |ref| of that vector. got, ref (R, H * DH)."""
    got = got.detach().double().cpu().reshape(-1, DH)
    ref = ref.detach().double().cpu().reshape(-1, DH)
    return (got - ref).abs().amax(-1) / ref.abs().amax(-1)


def ref_floor(ref):
    """Smallest max |ref| over the (row, head) vectors."""
    return float(ref.detach().double().reshape(-1, DH).abs().amax(-1).min())


def one_row_ref(qhat, kr, v, ak, av, g1, g2, vs, F, p):
    """Row p of ref_cpu.attn_fwd without the (S, S) matrix: qhat (H, DH) the rotated query of position p; kr, v (>= p + 1, H,
    DH) rotated keys and values of positions 0..p (later rows are not looked at); ak, av (A, H, DH); g1, g2 (H,) fp64.
    Adapter softmax x tanh(gate1), causal softmax over keys 0..p, gate2 on [vs, vs + F) when p >= vs + F.
    Returns o (H, DH) and the text weights (H, p + 1)."""
    sc = 1.0 / math.sqrt(DH)
    s_a = torch.einsum("hd,ahd->ha", qhat, ak) * sc
    s_t = torch.einsum("hd,thd->ht", qhat, kr[: p + 1]) * sc
    if vs >= 0 and p >= vs + F:
        s_t[:, vs:vs + F] += g2[:, None]
    pa, pt = torch.softmax(s_a, -1), torch.softmax(s_t, -1)
    o = torch.tanh(g1)[:, None] * torch.einsum("ha,ahd->hd", pa, av) + torch.einsum("ht,thd->hd", pt, v[: p + 1])
    return o, pt


def gates(H, seed):
    return rnd(H, seed=seed + 1).float(), rnd(H, seed=seed + 2).float() - 3.0       # gate2 in [-4, -2]


# ------------------------------------------------------------------------------------------------ fvqa_attn_decode
SWEEP_POS = [0, 1, 15, 16, 63, 64, 127, 128, 129, 159, 160, 191, 192, 255, 256, 319]
PLANT_J = [0, 15, 16, 63, 64, 127, 128, 159, 160, 191, 192]
AF_PAIRS = [(10, 10), (1, 10), (16, 6), (3, 16), (10, 0)]


def sweep_vstart(pos):
    """-1, 0, 19 and a window that holds p, in turn."""
    return [[-1, 0, 19, max(p - 3, 0)][i % 4] for i, p in enumerate(pos)]


def bias_edge_rows(S, F):
    """(p, vs) of point 2: p = vs+F-1, vs+F, vs and S-1 for vs in {0, 7, -1} and a vs whose window runs over the end."""
    rows = []
    for vs in (0, 7, -1, S - F + 3 if F else S - 4):
        for p in (vs + F - 1, vs + F, vs, S - 1):
            if 0 <= p < S and (p, vs) not in rows:
                rows.append((p, vs))
    return rows


def plant_pairs():
    """(p, j) of point 3, and the video_start of each sequence: the j = 15 and 16 keys of the p = 319 rows are frame keys of a
    biased row (window [10, 20)), the j = 127 key of p = 128 is a frame key of an UNbiased row (window [120, 130))."""
    pairs, vstart = [], []
    for p in (127, 128, 319):
        for j in sorted(set(PLANT_J + [p - 1, p])):
            if j <= p:
                pairs.append((p, j))
                vstart.append(10 if p == 319 and j in (15, 16) else 120 if (p, j) == (128, 127) else -1 if j % 2 else 40)
    return pairs, vstart


def decode_case(dtype, cache_rotated, S, H, A, F, pos, vstart, seed, plants=(), oracle=True):
    """N = len(pos) sequences of length S; sequence n decodes the token at position pos[n]. plants: (n, j) — key j of
    sequence n is planted for the query of sequence n (every head). oracle=False: one_row_ref per sequence instead of the
    whole-sequence oracle. Every cache row from pos[n] on is NaN."""
    N, D = len(pos), H * DH
    base = rnd(N * S + A, 3 * D, dtype=dtype, seed=seed)
    g1, g2 = gates(H, seed)
    cos, sin, c64, s64 = tables(S)
    seqs = base[: N * S].view(N, S, 3, H, DH)
    q, k, v = seqs[:, :, 0], seqs[:, :, 1].clone(), seqs[:, :, 2]
    ar = torch.arange(N)
    p_t = torch.tensor(pos)
    qhat = rot_rows(q[ar, p_t].double(), p_t[:, None], c64, s64).to(dtype).double()                   # (N, H, DH)
    over = {}
    for (n, j) in plants:
        kh = planted(qhat[n], PLANT)
        if j == pos[n] or not cache_rotated:               # the key is held raw: un-rotated at its position, rounded
            k[n, j] = rot_rows(kh, j, c64, s64, inverse=True).to(dtype)
        else:
            over[(n, j)] = kh.to(dtype).double()
    kr = rotated_rounded(k, c64, s64, dtype)
    for (n, j), kh in over.items():
        kr[n, j] = kh
    ak = base[N * S:, D:2 * D].double().view(A, H, DH)
    av = base[N * S:, 2 * D:].double().view(A, H, DH)
    if oracle:
        qr = rotated_rounded(q, c64, s64, dtype)
        o_ref, (_, pt) = ref_cpu.attn_fwd(qr, kr, v.double(), ak, av, g1.double(), g2.double(), vstart, F)
        want = o_ref[ar, p_t].reshape(N, D)
        weight = {(n, j): pt[n, :, pos[n], j] for (n, j) in plants}
    else:
        want, weight = torch.empty(N, D, dtype=torch.float64), {}
        for n in range(N):
            o, pt = one_row_ref(qhat[n], kr[n], v[n].double(), ak, av, g1.double(), g2.double(), vstart[n], F, pos[n])
            want[n] = o.reshape(D)
            weight.update({(m, j): pt[:, j] for (m, j) in plants if m == n})
    full = base.clone()                                    # the whole sequences as a prefill would hold them
    full[: N * S].view(N, S, 3, H, DH)[:, :, 1] = kr.to(dtype) if cache_rotated else k
    rows = ar * S + p_t
    qkv_row = base[rows].clone()
    qkv_row.view(N, 3, H, DH)[:, 1] = k[ar, p_t]
    cache = full.clone()
    for n in range(N):
        cache[n * S + pos[n]:(n + 1) * S] = NAN
    return dict(qkv_row=qkv_row, cache=cache, full=full, rows=rows, want=want, weight=weight, g1=g1, g2=g2, cos=cos, sin=sin,
                vstart=torch.tensor(vstart, dtype=torch.int32), pos=p_t.to(torch.int64), N=N, S=S, H=H, A=A, F=F, D=D)


def sweep_case(dtype, cache_rotated):
    """Point 1: S = 320, H = 2, A = F = 10, one sequence per position of SWEEP_POS."""
    return decode_case(dtype, cache_rotated, 320, 2, 10, 10, SWEEP_POS, sweep_vstart(SWEEP_POS), seed=41)


def bias_edge_case(dtype, cache_rotated, A, F):
    """Point 2: S = 64, one sequence per (p, vs) of bias_edge_rows."""
    rows = bias_edge_rows(64, F)
    return decode_case(dtype, cache_rotated, 64, 2, A, F, [p for p, _ in rows], [vs for _, vs in rows], seed=43 + A + F)


def planted_decode_case(dtype, cache_rotated):
    """Point 3: S = 320, one sequence per (p, j) of plant_pairs, key j planted for the query at p."""
    pairs, vstart = plant_pairs()
    return decode_case(dtype, cache_rotated, 320, 2, 10, 10, [p for p, _ in pairs], vstart, seed=47,
                       plants=[(n, j) for n, (_, j) in enumerate(pairs)])


LDS_POS = [4095, 2079]
LDS_J = [4094, 2048, 128]


def lds_case(dtype, cache_rotated, j):
    """Point 4: S = 4096 = SMAX, N = 2, H = 1; key j planted in every sequence that can see it. One-row reference."""
    return decode_case(dtype, cache_rotated, 4096, 1, 10, 10, LDS_POS, [19, -1], seed=53,
                       plants=[(n, j) for n, p in enumerate(LDS_POS) if j <= p], oracle=False)


def store_read_case(dtype, cache_rotated, S, H, A, F, lengths, steps, seed):
    """Point 5: sequences with prompts of `lengths` tokens in the cache (NaN behind them) that are decoded `steps` tokens
    further, one call per token. want[t] (N, D): the oracle's rows lengths[n] + t over the whole sequences."""
    N, D = len(lengths), H * DH
    base = rnd(N * S + A, 3 * D, dtype=dtype, seed=seed)
    g1, g2 = gates(H, seed)
    cos, sin, c64, s64 = tables(S)
    seqs = base[: N * S].view(N, S, 3, H, DH)
    q, k, v = seqs[:, :, 0], seqs[:, :, 1], seqs[:, :, 2]
    qr, kr = rotated_rounded(q, c64, s64, dtype), rotated_rounded(k, c64, s64, dtype)
    vstart = [19, -1, 125][:N]
    ak = base[N * S:, D:2 * D].double().view(A, H, DH)
    av = base[N * S:, 2 * D:].double().view(A, H, DH)
    o_ref, _ = ref_cpu.attn_fwd(qr, kr, v.double(), ak, av, g1.double(), g2.double(), vstart, F)
    full = base.clone()
    if cache_rotated:
        full[: N * S].view(N, S, 3, H, DH)[:, :, 1] = kr.to(dtype)
    cache = full.clone()
    for n in range(N):
        cache[n * S + lengths[n]:(n + 1) * S] = NAN
    ar, L = torch.arange(N), torch.tensor(lengths)
    return dict(base=base, cache=cache, full=full, g1=g1, g2=g2, cos=cos, sin=sin, vstart=torch.tensor(vstart, dtype=torch.int32),
                want=[o_ref[ar, L + t].reshape(N, D) for t in range(steps)],
                k_want=(kr if cache_rotated else k.double()).reshape(N * S, D), N=N, S=S, H=H, A=A, F=F, D=D)


# ------------------------------------------------------------------------------------------------ fvqa_attn_suffix
T_CASES = [
    # N, S, H, O, T, start, len
    (2, 128, 2, 5, 7, [40, 96], [7, 3]),          # tile 0 spans 35 suffix rows: a second chunk, all of it hidden; tile 1 starts
                                                  # inside option 4
    (2, 128, 1, 3, 12, [33, 64], [12, 5]),        # 36 suffix rows in one tile: a second chunk that holds hidden keys only
    (1, 128, 2, 7, 5, [100], [5]),
    (2, 160, 1, 9, 15, [130, 32], [15, 1]),       # 135 queries in five tiles that span three options; in tile 1 (q0 = 32, suffix
                                                  # rows 30..74) queries 62 and 63 NEED the second chunk: their own rows 62, 63
    (1, 64, 1, 2, 16, [48], [16]),                # exactly one tile
    (1, 64, 1, 1, 1, [63], [1]),
]
T_VSTART = [[19, 90], [30, -1], [-1], [125, 28], [41], [5]]          # windows in front of, across and inside the suffix
START_EDGES = [0, 1, 31, 32, 33, 64, 124, 127]
PLANT_KINDS = ["prompt31", "prompt32", "prompt_last", "own0", "own_qj", "own_qj_m1"]


def eff_len(S, start, length):
    return [max(0, min(ln, S - st)) for st, ln in zip(start, length)]


PLANT_TILES = {0: ["first", "last"], 3: ["first", "chunk2", "last"]}       # T case -> where the planted query sits


def plant_target(O, T, length, tile):
    """(option, row) of the query that gets the planted key: in the first tile of 32 queries, in the last, or ("chunk2", T = 15
    only) query 63 = row 3 of option 4 in tile 1, whose suffix keys start at row 30: its own rows 2 and 3 (and the decoy on its
    row 4) are keys 62..64, in the tile's SECOND chunk of suffix keys."""
    c, qj = {"first": (1, 3), "last": (O - 1, length - 2), "chunk2": (4, 3)}[tile]
    qi = c * T + qj
    assert qi // 32 == {"first": 0, "last": (O * T - 1) // 32, "chunk2": 1}[tile] and qj + 1 < length
    if tile == "chunk2":
        assert qi - 1 >= (32 // T) * T + 32 and c + 1 < O
    return c, qj


def suffix_case(dtype, cache_rotated, N, S, H, O, T, vstart, start, length, A, F, seed, plant=None, decoys=True):
    """The N * O full sequences (option c of sample n: the sample's rows in front of start[n], rows of its own from there on),
    the oracle over each of them, and what the kernel is handed: the raw suffix rows (padding rows NaN), and the cache with
    every row from start[n] on NaN. plant = (kind, tile): sample 0 gets one planted key for one query (PLANT_KINDS,
    plant_target) and every decoy of point 9 for that query; the cache row start[0] then holds a decoy instead of NaN."""
    D = H * DH
    base = rnd(N * S + A, 3 * D, dtype=dtype, seed=seed)
    g1, g2 = gates(H, seed)
    cos, sin, c64, s64 = tables(S)
    full = base[: N * S].view(N, 1, S, 3 * D).repeat(1, O, 1, 1)
    own = rnd(N * O * S, 3 * D, dtype=dtype, seed=seed + 3).view(N, O, S, 3 * D)
    for n in range(N):
        full[n, :, start[n]:] = own[n, :, start[n]:]
    f5 = full.view(N, O, S, 3, H, DH)
    q, k, v = f5[:, :, :, 0], f5[:, :, :, 1], f5[:, :, :, 2]                 # views: a planted raw key lands in `full`
    L = eff_len(S, start, length)
    over, info, decoy_row = {}, None, None
    if plant is not None:
        kind, tile = plant
        st = start[0]
        c, qj = plant_target(O, T, L[0], tile)
        qhat = rot_rows(q[0, c, st + qj].double(), st + qj, c64, s64).to(dtype).double()                    # (H, DH)
        raw_at = lambda pos, score: rot_rows(planted(qhat, score), pos, c64, s64, inverse=True).to(dtype)   # noqa: E731
        if kind.startswith("prompt"):
            r = {"prompt31": 31, "prompt32": 32, "prompt_last": st - 1}[kind]
            assert 0 <= r < st
            if cache_rotated:
                over[r] = planted(qhat, PLANT).to(dtype).double()
            else:
                k[0, :, r] = raw_at(r, PLANT)
            kj, key_pos = None, r
        else:
            kj = {"own0": 0, "own_qj": qj, "own_qj_m1": qj - 1}[kind]
            k[0, c, st + kj] = raw_at(st + kj, PLANT)
            key_pos = st + kj
        where = [(c, qj + 1)]                                                # own option, the next row: causally hidden
        for cn in (c - 1, c + 1):                                            # the neighbouring options, the same row
            if 0 <= cn < O:
                where.append((cn, qj if kj is None else kj))
        for (cd, kd) in where if decoys else []:
            assert kd < L[0]
            k[0, cd, st + kd] = raw_at(st + kd, DECOY)
        decoy_row = planted(qhat, DECOY).to(dtype) if cache_rotated else raw_at(st, DECOY)                  # cache row start[0]
        info = dict(c=c, qj=qj, key_pos=key_pos, decoys=where)
    qr = rotated_rounded(q.reshape(N * O, S, H, DH), c64, s64, dtype)
    kr = rotated_rounded(k.reshape(N * O, S, H, DH), c64, s64, dtype)
    for r, kh in over.items():
        kr.view(N, O, S, H, DH)[0, :, r] = kh
    ak = base[N * S:, D:2 * D].double().view(A, H, DH)
    av = base[N * S:, 2 * D:].double().view(A, H, DH)
    vs_all = [vstart[n] for n in range(N) for _ in range(O)]
    o_ref, (_, pt) = ref_cpu.attn_fwd(qr, kr, v.reshape(N * O, S, H, DH).double(), ak, av, g1.double(), g2.double(), vs_all, F)
    o_ref = o_ref.reshape(N, O, S, D)
    if info is not None:
        info["weight"] = pt[info["c"], :, start[0] + info["qj"], info["key_pos"]]                           # sample 0: rows 0..O-1
        info["row"] = info["c"] * T + info["qj"]
    cache = base.clone()
    cache[: N * S].view(N, S, 3, H, DH)[:, :, 1] = (kr.view(N, O, S, H, DH)[:, 0].to(dtype) if cache_rotated else k[:, 0])
    for n in range(N):
        cache[n * S + start[n]:(n + 1) * S] = NAN
    if decoy_row is not None and decoys:
        cache[start[0]] = own[0, 0, 0]                                       # finite q and v; the decoy as its key
        cache[start[0]].view(3, H, DH)[1] = decoy_row
    suf = torch.full((N, O, T, 3 * D), NAN, dtype=dtype)
    want = torch.zeros(N, O, T, D, dtype=torch.float64)
    valid = torch.zeros(N, O, T, dtype=torch.bool)
    for n in range(N):
        suf[n, :, :L[n]] = full[n, :, start[n]:start[n] + L[n]]
        want[n, :, :L[n]] = o_ref[n, :, start[n]:start[n] + L[n]]
        valid[n, :, :L[n]] = True
    return dict(suf=suf.reshape(N * O * T, 3 * D), cache=cache, g1=g1, g2=g2, cos=cos, sin=sin, want=want.reshape(-1, D),
                valid=valid.reshape(-1), plant=info, vstart=torch.tensor(vstart, dtype=torch.int32),
                start=torch.tensor(start, dtype=torch.int32), length=torch.tensor(length, dtype=torch.int32),
                N=N, S=S, H=H, O=O, T=T, A=A, F=F, D=D)


def t_case(dtype, cache_rotated, i, plant=None, decoys=True):
    """Point 6 (and 9 with `plant`): case i of T_CASES, A = F = 10."""
    N, S, H, O, T, start, length = T_CASES[i]
    return suffix_case(dtype, cache_rotated, N, S, H, O, T, T_VSTART[i], start, length, 10, 10, seed=61 + i, plant=plant,
                       decoys=decoys)


def start_edge_case(dtype, cache_rotated, seed=21):
    """Point 7: one sample per start in START_EDGES (len 4; at 127 the end of the sequence cuts it to 1) and one with len 0."""
    start = START_EDGES + [50]
    length = [4] * len(START_EDGES) + [0]
    vstart = [-1, 0, 19, 30, 25, -1, 60, 120, 3]
    return suffix_case(dtype, cache_rotated, len(start), 128, 2, 5, 4, vstart, start, length, 10, 10, seed)


def frame_window_case(dtype, cache_rotated, A, F, seed=31):
    """Point 8: T = 16, O = 2, S = 64, start = 30; the window ends inside the suffix (at its row 5), straddles its start, lies
    wholly inside it, and is absent. Inside: rows 2 .. 2 + F, biased rows behind it — except F = 16 = T, where the only window
    inside the suffix IS the suffix (vs = start) and no row can lie behind it. With F = 0 the window is empty wherever it is:
    the four placements then differ only in which rows count as biased, on no key."""
    S, st = 64, 30
    vstart = [st + 5 - F, st - F // 2, st + 2 if F + 2 < 16 else st, -1]
    return suffix_case(dtype, cache_rotated, 4, S, 2, 2, 16, vstart, [st] * 4, [16] * 4, A, F, seed)


def append_case(dtype, cache_rotated, T, start):
    """Points 11 and 12: N = 3, S = 160, H = 2, one continuation per sequence (O = 1)."""
    return suffix_case(dtype, cache_rotated, 3, APPEND_S, 2, 1, T, [19, -1, 125], start, append_lengths(T, start), 10, 10,
                       seed=71 + T + start[0])


APPEND_S = 160
APPEND_STARTS = [[120, 127, 144], [0, 32, 159]]


def append_lengths(T, start):
    """Mixed lengths: a full one, an empty one, and one that the end of the sequence cuts (start 159 with T > 1)."""
    return [T, 0, T] if start[0] else [max(1, T // 2), T, T]


# ------------------------------------------------------------------------------------------------ fp32 in the kernel's order
def decode_row_fp32(qhat, kr, v, ak, av, g1, g2, vs, F, p):
    """one_row_ref's formula in fp32 on the CPU with the VALUE sum in fvqa_attn_decode's order (csrc/attn_decode_body.h: four
    partial sums over keys w, w + 4, ..., then the adapter's, added pairwise); exp of score - max and probabilities scaled by
    1 / sum as there. The 128-term dot products and the softmax sums use torch's fp32 sums, not the kernel's quad / wave order.
    For the rule that a per-row bound which the GPU misses is re-derived from this figure (x 4) and not from the GPU's."""
    f = torch.float32
    qhat, kr, v, ak, av = qhat.to(f), kr[: p + 1].to(f), v[: p + 1].to(f), ak.to(f), av.to(f)
    sc = torch.tensor(1.0 / math.sqrt(DH), dtype=f)
    s_t = (qhat[None] * kr).sum(-1).T * sc                                   # (H, p + 1)
    if vs >= 0 and p >= vs + F:
        s_t[:, vs:vs + F] += g2.to(f)[:, None]
    e = torch.exp(s_t - s_t.amax(-1, keepdim=True))
    pt = e * (1.0 / e.sum(-1, keepdim=True))
    s_a = (qhat[None] * ak).sum(-1).T * sc
    ea = torch.exp(s_a - s_a.amax(-1, keepdim=True))
    pa = ea / ea.sum(-1, keepdim=True) * torch.tanh(g1.to(f))[:, None]
    parts = []
    for w in range(4):
        o = torch.zeros(qhat.shape, dtype=f)
        for j in range(w, p + 1, 4):
            o += pt[:, j, None] * v[j]
        for a in range(w, ak.shape[0], 4):
            o += pa[:, a, None] * av[a]
        parts.append(o)
    return (parts[0] + parts[1]) + (parts[2] + parts[3])
