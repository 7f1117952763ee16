"""Helpers of the option-scoring frame-attention tests (tests/test_score_mass_cpu.py, tests/test_score_mass_gpu.py), host code only:
an fp64 restatement of the summary fvqa_attn_suffix_mass writes, straight from the operands a suffix case of
tests/cached_attn_util.py hands the kernel; the same rows laid out as a dense arena for fvqa_attn_row_mass; the neighbour swaps
that show a misplaced summary; and, for the end-to-end tests, the dense scoring arena of the existing route with its host fp64
summary, and the reference's fixtures (tools/gen_golden_score_attention.py)."""
import functools
import math
import os

import numpy as np
import torch

from tests import cached_attn_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND = 3e-5                          # the project's bound for the decode summary (tests/test_frame_attention_gpu.py: BOUND)
FIXTURES = ("tiny", "7b_l2_peakedperm")
AXES = {"option": 1, "row": 2, "layer": 3, "head": 4}


def summary(pt, vs, F, p):
    """pt (H, p + 1) text weights of the query at position p -> (H, F + 2): include/fvqa.h's definition, key by key."""
    at = [kpos - vs if (vs >= 0 and vs <= kpos < vs + F) else F if kpos < vs else F + 1 for kpos in range(p + 1)]
    return torch.zeros(pt.shape[0], F + 2, dtype=pt.dtype).index_add_(1, torch.tensor(at), pt)


# ------------------------------------------------------------------------------------------------ the kernel's cases
@functools.lru_cache(maxsize=None)
def case(kind, dtype, rot, arg=None):
    """The suffix cases of the util, built once per (kind, storage type, cache convention) and shared by the tests."""
    if kind == "t":
        return U.t_case(dtype, rot, arg)
    if kind == "start":
        return U.start_edge_case(dtype, rot)
    return U.frame_window_case(dtype, rot, *arg)


@functools.lru_cache(maxsize=None)
def case_reference(kind, dtype, rot, arg=None):
    """The fp64 summary (N, O, T, H, F + 2) of a case: every valid query row's softmax over the cached prompt keys [0, start[n])
    and rows 0..j of its own option, q and k rotated in fp64 and rounded to the storage type as the kernel's contract states
    (a rotated cache is taken as it is), gate2 on the window when the row lies behind it; zeros at the padding rows."""
    c = case(kind, dtype, rot, arg)
    N, S, H, O, T, F = c["N"], c["S"], c["H"], c["O"], c["T"], c["F"]
    _, _, c64, s64 = U.tables(S)
    suf = c["suf"].view(N, O, T, 3, H, U.DH)
    cache = c["cache"][: N * S].view(N, S, 3, H, U.DH)
    g2 = c["g2"].double()
    L = U.eff_len(S, c["start"].tolist(), c["length"].tolist())
    want = torch.zeros(N, O, T, H, F + 2, dtype=torch.float64)
    rr = lambda x, pos: U.rot_rows(x.double(), pos[:, None], c64, s64).to(dtype).double()      # noqa: E731
    for n in range(N):
        st, vs = int(c["start"][n]), int(c["vstart"][n])
        kp = cache[n, :st, 1].double() if rot else rr(cache[n, :st, 1], torch.arange(st))
        own = st + torch.arange(L[n])
        for o in range(O):
            qs, ks = rr(suf[n, o, :L[n], 0], own), rr(suf[n, o, :L[n], 1], own)
            for j in range(L[n]):
                p = st + j
                s = torch.einsum("hd,thd->ht", qs[j], torch.cat([kp, ks[: j + 1]])) / math.sqrt(U.DH)
                if vs >= 0 and p >= vs + F:
                    s[:, vs:vs + F] += g2[:, None]
                want[n, o, j] = summary(torch.softmax(s, -1), vs, F, p)
    return want


def dense_arena(c, rot):
    """The case's N * O sequences as ONE layer's arena buffer (N * O * S + A, 3 * D) for fvqa_attn_row_mass — prompt rows from the
    cache, suffix rows behind them, q and k of the suffix rows in the cache's convention (rotated and rounded when it holds rotated
    keys), everything behind a sequence's last valid row NaN — with seq, pos (int32) of every valid row, its index in (N, O, T), every sequence's video_start and the arena's adapter rows."""
    N, S, H, O, T, A, D = c["N"], c["S"], c["H"], c["O"], c["T"], c["A"], c["D"]
    dtype = c["cache"].dtype
    _, _, c64, s64 = U.tables(S)
    A_arena = max(A, 1)                  # (the summary does not read the adapter rows; its wrapper asks for one)
    arena = torch.full((N * O * S + A_arena, 3 * D), U.NAN, dtype=dtype)
    arena[N * O * S:N * O * S + A] = c["cache"][N * S:]
    suf = c["suf"].view(N, O, T, 3 * D)
    L = U.eff_len(S, c["start"].tolist(), c["length"].tolist())
    seq, pos, at = [], [], []
    for n in range(N):
        st = int(c["start"][n])
        for o in range(O):
            m = n * O + o
            arena[m * S:m * S + st] = c["cache"][n * S:n * S + st]
            rows = suf[n, o, :L[n]].clone()
            if rot and L[n]:
                qk = rows.view(L[n], 3, H, U.DH)[:, :2].double()
                own = (st + torch.arange(L[n]))[:, None, None]
                rows.view(L[n], 3, H, U.DH)[:, :2] = U.rot_rows(qk, own, c64, s64).to(dtype)
            arena[m * S + st:m * S + st + L[n]] = rows
            for j in range(L[n]):
                seq.append(m), pos.append(st + j), at.append((n * O + o) * T + j)
    i32 = lambda x: torch.tensor(x, dtype=torch.int32)      # noqa: E731
    return arena, i32(seq), i32(pos), torch.tensor(at), c["vstart"].repeat_interleave(O), A_arena


def one_hot_rows(want):
    """Rows whose reference summary puts all weight on ONE entry — no window, or a window that starts behind the row — are equal
    to each other by definition, wherever they sit; so are padding rows (zeros). (N, O, T, H) bool."""
    return (want.amax(-1) == want.sum(-1))


def swapped_pairs_missing(got, want, axis, bound=BOUND):
    """got, want (N, O, T, H, F + 2): entry e of got against the NEIGHBOURING entry e' of want along `axis` (1 option, 2 row,
    3 head), both directions -> (pairs that miss the bound, pairs), over the pairs in which not both references are one-hot."""
    n = got.shape[axis]
    lo, hi = torch.arange(n - 1), torch.arange(1, n)
    hot = one_hot_rows(want)
    miss = total = 0
    for a, b in ((lo, hi), (hi, lo)):
        d = (got.index_select(axis, a) - want.index_select(axis, b)).abs().amax(-1)
        keep = ~(hot.index_select(axis, a) & hot.index_select(axis, b))
        miss += int((d[keep] > bound).sum())
        total += int(keep.sum())
    return miss, total


# ------------------------------------------------------------------------------------------------ end to end
def load_fixture(name):
    return dict(np.load(os.path.join(ROOT, "tests", "golden", f"score_mass_{name}.npz")))


def dense_scoring_arena(eng, batch):
    """The arena of the EXISTING dense scoring route (fvqa/score.py _dense: the options flattened to (B * O, 1, S), the training
    forward with tail rows) -> (qkv (L, B * O * S + A, 3 D), vstart (B * O,), whether k is rotated), on the host."""
    from fvqa import rowpass, score
    from fvqa.generate import vqa_stream_only
    ids, lab = batch["text_id"]["vqa"].cpu(), batch["label"]["vqa"].cpu()
    B, O, S = ids.shape
    vs = [int(v) for v in batch["video_start"]["vqa"]]
    sub = score._front_inputs(batch, O)
    sub.update({"text_id": {"vqa": ids.reshape(B * O, 1, S)}, "label": {"vqa": lab.reshape(B * O, 1, S)},
                "video_start": {"vqa": [vs[0]] * (B * O), "vaq": [vs[0]] * (B * O)}})
    with torch.no_grad(), vqa_stream_only(eng, "_score_arena", "scored"):
        eng.forward(sub)
        qkv, vstart = eng.saved["ar"].qkv.cpu(), eng.saved["vstart"].cpu()
        eng.saved = None
    return qkv, vstart, rowpass.cache_rotated(eng)


def host_rows_mass(eng, qkv, vstart, rotated, seq, pos, S):
    """The summary in torch fp64 on the host of the rows (seq[r], pos[r]) of an arena (L, n_seq * S + A, 3 D) -> (R, L, H, F + 2).
    No summary kernel runs: q and k are read from the arena (rotated here in fp64 and rounded to the storage type where the arena
    holds them raw), scored, biased, soft-maxed and binned here."""
    H, F, L = eng.H, eng.F, eng.L
    c64, s64 = eng.cos.cpu().double(), eng.sin.cpu().double()
    out = torch.zeros(len(seq), L, H, F + 2, dtype=torch.float64)
    for i in range(L):
        g2 = eng.model.gate_views(i)[1].detach().cpu().double()
        for r, (m, p) in enumerate(zip(seq, pos)):
            rows = qkv[i, m * S:(m + 1) * S].view(S, 3, H, U.DH)
            vs = int(vstart[m])
            q, k = rows[p, 0].double(), rows[: p + 1, 1].double()
            if not rotated:
                q = U.rot_rows(q, p, c64, s64).to(qkv.dtype).double()
                k = U.rot_rows(k, torch.arange(p + 1)[:, None], c64, s64).to(qkv.dtype).double()
            s = torch.einsum("hd,thd->ht", q, k) / math.sqrt(U.DH)
            if vs >= 0 and p >= vs + F:
                s[:, vs:vs + F] += g2[:, None]
            out[r, i] = summary(torch.softmax(s, -1), vs, F, p)
    return out


def host_option_mass(eng, qkv, vstart, rotated, start, length, B, O, S):
    """host_rows_mass of a dense scoring arena at the suffix rows -> (B, O, T, L, H, F + 2), T = max length, zeros behind length[n]."""
    T = int(max(length))
    where = [(n, o, j) for n in range(B) for o in range(O) for j in range(int(length[n]))]
    rows = host_rows_mass(eng, qkv, vstart, rotated, [n * O + o for n, o, _ in where], [int(start[n]) + j for n, _, j in where], S)
    out = torch.zeros(B, O, T, eng.L, eng.H, eng.F + 2, dtype=torch.float64)
    for r, at in enumerate(where):
        out[at] = rows[r]
    return out


def misplaced_is_seen(got, fix, b, axis, live):
    """got, fix (B, O, T, L, H, F + 2): the share of the ordered pairs of neighbours (e, e') along `axis` in which got[e] differs
    from fix[e'] by more than b in some component. live (B, O, T) bool (broadcast over L, H): which entries take part — the rows
    in front of length[n]; on the option axis only rows whose context differs between options c and c + 1 (sep_option_live)."""
    ax = AXES[axis]
    n = got.shape[ax]
    lo, hi = torch.arange(n - 1), torch.arange(1, n)
    miss = []
    for a, c in ((lo, hi), (hi, lo)):
        d = (got.index_select(ax, a) - fix.index_select(ax, c)).abs().amax(-1)              # (B, O', T', L', H')
        if axis == "option":
            keep = live                                                                      # (B, O - 1, T)
        elif axis == "row":
            keep = live.index_select(2, a) & live.index_select(2, c)
        else:
            keep = live
        miss.append(d[keep[..., None, None].expand_as(d)] > b)
    return float(torch.cat(miss).double().mean())


if __name__ == "__main__":
    # python -m tests.score_mass_util (on a GPU): the end-to-end figures — the host fp64 summary of the dense scoring arena against
    # the fixtures, per fixture and build; nothing of the summary kernels or of score_options(frame_attention=True) runs
    from tests.gpu_util import build_model
    from tests.test_score_gpu import fixture_cfg, golden_batch, load
    for name in FIXTURES:
        g, fix = load("score_" + name), load_fixture(name)
        want = torch.from_numpy(fix["mass"]).double()
        for dtype in (torch.float32, torch.bfloat16, torch.float16):
            model, _ = build_model(fixture_cfg("score_" + name), dtype)
            eng = model.eval().ensure_engine()
            batch = golden_batch(g)
            B, O, S = batch["text_id"]["vqa"].shape
            qkv, vstart, rotated = dense_scoring_arena(eng, batch)
            host = host_option_mass(eng, qkv, vstart, rotated, fix["start"].tolist(), fix["length"].tolist(), B, O, S)
            fig = float((host - want).abs().max())
            print(f"{name} {dtype}: host fp64 summary of the dense scoring arena - fixture {fig:.3e} -> b = {max(4 * fig, BOUND):.3e}")
