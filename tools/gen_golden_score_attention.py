#!/usr/bin/env python3
"""TEST INFRASTRUCTURE — generates tests/golden/score_mass_tiny.npz and score_mass_7b_l2_peakedperm.npz, the reference's own
frame-attention summary at the rows that score an answer option (tests/test_score_mass_*.py), by running the REFERENCE in the
build container. Never imported by the product.

The set-up is tools/gen_golden_score.py's — the reference's multiple-choice validation (llama/model_my_original_mod.py with
`inference=True`, not a generation task: the B * O option sequences in one batch) on the validation batch of its own reader —,
run under the `F.softmax` spy of tools/gen_golden_attention.py: the output of the TEXT softmax of Attention.forward (the (B * O,
H, S, S) one; the adapter's is (.., S, A)), one call per layer, reduced row by row to the summary of include/fvqa.h
fvqa_attn_decode_mass. Kept are the suffix rows of fvqa.score.plan_options — of option c of sample n the positions start[n] + j,
j < length[n] —, zeros behind length[n].

Stored: mass (B, O, T, L, H, F + 2) fp32, start, length (B,), and the largest component difference of every pair of neighbours
along the row, layer, head and option axes (`sep_row`, `sep_layer`, `sep_head`; `sep_option`, with `sep_option_live`: whether
the two rows' contexts differ, i.e. the position is not in front of the first token in which options c and c + 1 differ — the
rows in front of it are equal by construction, asserted here as an exact 0 — only the live pairs count).

Asserted — what the end-to-end test relies on: a summary delivered one row, layer, head or option off its place must miss the
build's end-to-end bound b, so in at least 90 % of the pairs of neighbours the reference's own two summaries differ by more than b
in some component. PREMISE lists, per fixture and build, b (tests/test_score_mass_gpu.py E2E_FIGURE, profiles/
score_frame_attention.log) and the axes the reference gives that for; the shares of every axis are printed.

usage: gen_golden_score_attention.py            (both fixtures)
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "flipped-vqa_amd"))
from fvqa import score, synth  # noqa: E402
import oracle.gen_golden as G  # noqa: E402
import gen_golden_attention as GA  # noqa: E402
import gen_golden_score as GS  # noqa: E402

FIXTURES = [("tiny", ""), ("7b_l2", "peakedperm")]
AXES = ("row", "layer", "head", "option")
# fixture -> build -> (b, the axes on which at least 90 % of the reference's neighbours lie more than b apart)
PREMISE = {
    "tiny": {"fp32": (3e-5, AXES), "fp16": (1.851e-4, AXES), "bf16": (1.303e-3, AXES[:3])},
    "7b_l2_peakedperm": {"fp32": (3e-5, AXES), "fp16": (2.465e-4, AXES), "bf16": (2.227e-3, AXES[:3])},
}
# (the option axis under bf16: the options' summaries lie closer together than that build's b — shares 0.781 and 0.581; an option
# delivered off its place is what the kernel-level swap test of tests/test_score_mass_gpu.py sees, in every storage type)


def reference_mass(pname, mode):
    st = GS.setup()
    M2, batch = st["M2"], st["batch"]
    cfg = synth.preset(pname, vaq=False, qav=False, vocab_size=32000, max_seq_len=128, batch_size=4, peaked=mode == "peaked",
                       peaked_perm=mode == "peakedperm")
    model, margs = G.build_reference(M2, cfg)
    margs.is_generation_task = False
    model.eval()
    ids, lab = batch["text_id"]["vqa"], batch["label"]["vqa"]
    B, O, S = ids.shape
    vstart = [int(v) for v in batch["video_start"]["vqa"]]
    assert len(set(vstart)) == 1                              # (the reference reads video_start[0] for the whole batch)
    L, F, H = cfg.adapter_layer, cfg.max_feats, cfg.n_heads
    plan = score.plan_options(ids, lab, batch["prefix_index"]["vqa"], vstart, F)
    seen = []
    real_F = M2.F

    class SpyF:
        def __getattr__(self, name):
            return getattr(real_F, name)

        @staticmethod
        def softmax(x, dim=-1, **kw):
            y = real_F.softmax(x, dim=dim, **kw)
            if x.dim() == 4 and x.shape[-1] == x.shape[-2] == S:
                assert x.shape[0] == B * O
                seen.append(torch.stack([GA.summary_rows(p.detach().float(), vstart[0], F) for p in y]))     # (B * O, S, H, F + 2)
            return y

    M2.F = SpyF()
    try:
        with torch.no_grad():
            model(batch, inference=True)
    finally:
        M2.F = real_F
    assert len(seen) == L, (len(seen), L)                     # one text softmax per layer
    T = plan.T
    mass = np.zeros((B, O, T, L, H, F + 2), dtype=np.float32)
    for i, m in enumerate(seen):
        m = m.view(B, O, S, H, F + 2)
        for n in range(B):
            s, ln = int(plan.start[n]), int(plan.length[n])
            mass[n, :, :ln, i] = m[n, :, s:s + ln].numpy()
    live = np.arange(T)[None, :] < plan.length.numpy()[:, None]
    assert np.abs(mass.sum(-1)[live[:, None, :].repeat(O, 1)] - 1).max() < 1e-5
    del model
    return batch, plan, mass


def separations(mass, ids, start, length):
    """mass (B, O, T, L, H, F + 2) -> {axis: largest component difference of every pair of neighbours}, pairs with a padding row
    left out of the row axis (NaN), and `option_live` (B, O - 1, T): the two rows' contexts differ."""
    B, O, T = mass.shape[:3]
    live = np.arange(T)[None, :] < length[:, None]                                        # (B, T)
    sep = {"row": np.abs(np.diff(mass, axis=2)).max(-1), "layer": np.abs(np.diff(mass, axis=3)).max(-1),
           "head": np.abs(np.diff(mass, axis=4)).max(-1), "option": np.abs(np.diff(mass, axis=1)).max(-1)}
    both = (live[:, 1:] & live[:, :-1])[:, None, :, None, None]
    sep["row"] = np.where(both, sep["row"], np.nan)
    for k in ("layer", "head"):
        sep[k] = np.where(live[:, None, :, None, None], sep[k], np.nan)
    S = ids.shape[-1]
    differs = ids[:, 1:] != ids[:, :-1]                                                   # (B, O - 1, S)
    first = np.where(differs, np.arange(S), S).min(-1)                                    # (B, O - 1)
    pos = start[:, None] + np.arange(T)[None, :]                                          # (B, T)
    opt_live = (pos[:, None, :] >= first[:, :, None]) & live[:, None, :]
    dead = sep["option"][~opt_live & live[:, None, :]]
    assert dead.size == 0 or float(dead.max()) == 0.0, "rows in front of the first differing token must be equal"
    return sep, opt_live


def share_apart(sep, b, opt_live=None):
    v = sep[opt_live] if opt_live is not None else sep[~np.isnan(sep)]
    return float((v > b).mean()), float(np.quantile(v, 0.1))


def run(pname, mode):
    name = pname + ("_" + mode if mode else "")
    batch, plan, mass = reference_mass(pname, mode)
    ids = batch["text_id"]["vqa"].numpy()
    start, length = plan.start.numpy(), plan.length.numpy()
    sep, opt_live = separations(mass, ids, start, length)
    for ax in AXES:
        _, q10 = share_apart(sep[ax], 0.0, opt_live if ax == "option" else None)
        print(f"  [{name}] {ax}: 10 % quantile of the neighbour separation {q10:.2e}")
    for build, (b, axes) in PREMISE[name].items():
        for ax in AXES:
            frac, _ = share_apart(sep[ax], b, opt_live if ax == "option" else None)
            print(f"  [{name}] {build} {ax}: neighbours more than b = {b:.3e} apart: {frac:.3f}" + ("" if ax in axes else "  (not held)"))
            assert ax not in axes or frac >= 0.9, f"{name} {build} {ax}: neighbouring summaries are too alike for the bound"
    zero_rows = [j for j in range(plan.T) if not opt_live[:, :, j].any()]
    out = {"mass": mass, "start": start.astype(np.int64), "length": length.astype(np.int64),
           "sep_row": sep["row"].astype(np.float32), "sep_layer": sep["layer"].astype(np.float32),
           "sep_head": sep["head"].astype(np.float32), "sep_option": sep["option"].astype(np.float32),
           "sep_option_live": opt_live}
    path = os.path.join(ROOT, "tests", "golden", f"score_mass_{name}.npz")
    np.savez_compressed(path, **out)
    F = mass.shape[-1] - 2
    print(f"[score_mass_{name}] mass {mass.shape}, start {start.tolist()} length {length.tolist()}, suffix rows equal across every "
          f"pair of options: {zero_rows}, video mass mean {float(mass[..., :F].sum(-1).mean()):.4f} -> {path} "
          f"{os.path.getsize(path) // 1024} KiB", flush=True)


if __name__ == "__main__":
    for pname, mode in FIXTURES:
        run(pname, mode)
