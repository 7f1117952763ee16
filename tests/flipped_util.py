"""Helpers of the flipped-scoring tests (tests/test_flipped_cpu.py, tests/test_flipped_gpu.py), built on the CPU only: the
fixtures of tools/gen_golden_flipped.py as batches, the launch schedule of the fvqa_attn_suffix_wide grid, and an fp64 restatement
of that kernel's contract from the operands it is handed — with a switch that plants one defect, so that the test can show it
sees such errors."""
import math
import os

import numpy as np
import torch

from fvqa import synth
from tests import cached_attn_util as U

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TASKS = ("vqa", "vaq", "qav")
F = 10
S_FIX = 192                                   # sequence length of the fixtures
FIXTURES = ["flipped_tiny", "flipped_tiny_gen", "flipped_7b_l2_peakedperm"]


def load(name):
    return dict(np.load(os.path.join(GOLDEN, name + ".npz")))


def golden_batch(g, samples=None):
    """The validation batch of a fixture as score_flipped takes it (`samples`: a sub-batch)."""
    idx = list(range(g["answer"].shape[0])) if samples is None else list(samples)
    t = lambda k: torch.from_numpy(g[k])[idx]                    # noqa: E731
    return {"video": t("video"), "text_id": {k: t(f"text_id_{k}") for k in TASKS}, "label": {"vqa": t("reader_label_vqa")},
            "video_start": {"vqa": g["vstart_vqa"][idx].tolist(), "vaq": g["vstart_vaq"][idx].tolist()},
            "prefix_index": {"vqa": g["reader_prefix_vqa"][idx].tolist()}, "answer": t("answer"), "qtype": t("qtype"),
            "vid": [f"v{i}" for i in idx]}


def fixture_cfg(name, **over):
    base = name[len("flipped_"):].replace("_gen", "").replace("_peakedperm", "")
    return synth.preset(base, vaq=True, qav=True, vocab_size=32000, max_seq_len=S_FIX, batch_size=4,
                        peaked_perm="peakedperm" in name, **over)


# ------------------------------------------------------------------------------------------------ fvqa_attn_suffix_wide
WIDE_T = [1, 16, 17, 32, 33, 63, 64]
WIDE_S, WIDE_H, WIDE_B = 96, 2, 2
WIDE_STARTS = [0, 1, 31, 32, 33, None]        # None: S - T


def wide_schedule(T):
    """The launches of one suffix length: (O, start (B,), len (B,), A, F, vstart (B,)) — every O of {1, 3, 5}, every start of
    {0, 1, 31, 32, 33, S - T}, every len of {0, 1, T - 1, T} mixed within a batch, A of {0, 10}, F of {0, 3, 10}, and the frame
    window in the cache, across start, inside the suffix and absent, each factor's values rotating against the others' (a full
    product would be 2592 launches per T; the six below hold every value of every factor, every window placement with F = 3,
    and F = 10 in the cache, across start and inside the suffix)."""
    S = WIDE_S
    starts = [S - T if s is None else s for s in WIDE_STARTS]
    lens = [0, 1, T - 1, T]
    out = []
    for i in range(6):
        O = [1, 3, 5][i % 3]
        st = [starts[i], starts[(i + 3) % 6]]
        ln = [lens[(i + 1) % 4], lens[(i + 3) % 4]]
        if i == 0:
            ln = [T, T - 1]
        A = [10, 0][i % 2]
        Fw = [10, 3, 0, 3, 10, 10][i]
        vs = []
        for b in range(2):
            kind, s0 = ["cache", "across", "inside", "none"][(i + b) % 4], st[b]
            if kind == "cache" and s0 - Fw - 1 >= 0:
                vs.append(max(0, s0 - Fw - 3))
            elif kind == "across" and s0 >= 1:
                vs.append(max(0, s0 - Fw // 2 - 1))
            elif kind == "none":
                vs.append(-1)
            else:                                                  # inside the suffix (rows behind it are biased when T allows)
                vs.append(min(s0 + 1, S - 1))
        out.append((O, st, ln, A, Fw, vs))
    return out


def wide_case(dtype, cache_rotated, T, O, start, length, A, Fw, vstart, seed):
    """cached_attn_util.suffix_case at the grid's shape: its operands and `want`, the rows of the full-sequence fp64 oracle.
    A = 0 (the oracle has no such form): the case is built with one adapter row, the kernel is handed the cache without it, and
    `want` is wide_restated — which the A = 10 cases tie to the oracle (tests/test_flipped_cpu.py)."""
    c = U.suffix_case(dtype, cache_rotated, WIDE_B, WIDE_S, WIDE_H, O, T, vstart, start, length, max(A, 1), Fw, seed)
    if A == 0:
        c["cache"] = c["cache"][: WIDE_B * WIDE_S].contiguous()
        c["A"] = 0
        c["want"] = wide_restated(c, dtype, cache_rotated)
    return c


def wide_restated(c, dtype, cache_rotated, defect=None):
    """fvqa_attn_suffix_wide's contract (include/fvqa.h) in fp64 from the operands of a wide_case: the query at (n, c, j) sits at
    start[n] + j, sees the cache rows [0, start[n]), rows 0..j of its own option and the adapter keys; gate2 on [vs, vs + F) for
    query positions >= vs + F. -> (rows, D), zeros at padding rows. defect: None, or one planted error —
      "causal"  the query also sees row j + 1 of its option (where that row is live);
      "option"  option c >= 1 reads option c - 1's suffix keys and values;
      "gate2"   no gate2 where the window starts inside the suffix."""
    N, S, H, O, T, A, Fw, D = c["N"], c["S"], c["H"], c["O"], c["T"], c["A"], c["F"], c["D"]
    _, _, c64, s64 = U.tables(S)
    suf = c["suf"].view(N, O, T, 3, H, U.DH)
    cache = c["cache"]
    seqs = cache[: N * S].view(N, S, 3, H, U.DH)
    ak = cache[N * S:, D:2 * D].double().view(A, H, U.DH)
    av = cache[N * S:, 2 * D:].double().view(A, H, U.DH)
    g1, g2 = c["g1"].double(), c["g2"].double()
    out = torch.zeros(N, O, T, D, dtype=torch.float64)
    for n in range(N):
        st = int(c["start"][n])
        L = max(0, min(int(c["length"][n]), T, S - st))
        vs = int(c["vstart"][n])
        pk = seqs[n, :st, 1].double()
        if not cache_rotated:
            pk = U.rot_rows(pk, torch.arange(st)[:, None], c64, s64).to(dtype).double()
        pv = seqs[n, :st, 2].double()
        pos = st + torch.arange(L)
        for o in range(O):
            src = o - 1 if defect == "option" and o >= 1 else o
            qh = U.rot_rows(suf[n, o, :L, 0].double(), pos[:, None], c64, s64).to(dtype).double()
            kh = U.rot_rows(suf[n, src, :L, 1].double(), pos[:, None], c64, s64).to(dtype).double()
            vh = suf[n, src, :L, 2].double()
            for j in range(L):
                see = j + 1 + (1 if defect == "causal" and j + 1 < L else 0)
                kr, v = torch.cat([pk, kh[:see]]), torch.cat([pv, vh[:see]])
                w = -1 if defect == "gate2" and vs >= st else vs
                out[n, o, j] = _row(qh[j], kr, v, g2, w, Fw, st + j, ak, av, g1).reshape(D)
    return out.reshape(-1, D)


def _row(qhat, kr, v, g2, vs, Fw, p, ak, av, g1):
    """One query row at position p over ALL the keys handed in (cached_attn_util.one_row_ref's formula; the keys may run past p —
    a planted defect — and there may be no adapter key)."""
    sc = 1.0 / math.sqrt(U.DH)
    s_t = torch.einsum("hd,thd->ht", qhat, kr) * sc
    if vs >= 0 and p >= vs + Fw:
        s_t[:, vs:vs + Fw] += g2[:, None]
    o = torch.einsum("ht,thd->hd", torch.softmax(s_t, -1), v)
    if ak.shape[0]:
        pa = torch.softmax(torch.einsum("hd,ahd->ha", qhat, ak) * sc, -1)
        o = o + torch.tanh(g1)[:, None] * torch.einsum("ha,ahd->hd", pa, av)
    return o
