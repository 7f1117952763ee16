#!/usr/bin/env python3
"""TEST INFRASTRUCTURE — generates tests/golden/score_<preset>[_<variant>].npz: the reference's multiple-choice validation
(engine.py:86-93 over llama/model_my_original_mod.py:332-377,506 — `inference=True`, not a generation task) run in the build
container, the way oracle/gen_golden_eval.py makes the generation fixtures: the fp32-shim reference model with closed-form
weights (oracle.gen_golden.install_shims / build_reference, handed the module that still carries the per-option branch), the
validation batch built by the reference's own NExT-QA reader with is_generation_task=False on the synthetic table of
oracle/gen_golden_loader.py (four samples, five options).

Stored: the batch (ids, labels, prefix / video-start indices, answers, question types, frame features), `individual_losses`
(B, O, S-1), `count`, the per-option `mean`, `prediction`, and per sample `gap` = (second-lowest mean - lowest mean) / lowest
mean: how decided the reference's own choice is — what a 16-bit build can be held to.

usage: gen_golden_score.py <preset> [peaked|peakedperm]      (no arguments: every fixture below, gaps printed)

Which 7b_l2 variant the bf16 / fp16 pins use: the one whose recorded gaps are largest. This script prints them (min / median
over the four samples, as generated):
    score_7b_l2             random LM head                      1.7e-4 / 8.4e-4
    score_7b_l2_peaked      head tied to the embeddings         4.2e-3 / 4.2e-3     (not kept)
    score_7b_l2_peakedperm  head tied through a permutation     5.1e-3 / 5.2e-3     <- the 16-bit pins
score_7b_l2 stays as the fp32 fixture at 7B width; the `peaked` file is not committed.
"""
import os
import sys
import tempfile
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "flipped-vqa_amd"))
from fvqa import synth  # noqa: E402
import oracle.gen_golden as G  # noqa: E402
import oracle.gen_golden_loader as GL  # noqa: E402
from oracle.fake_sp import FakeSentencePiece  # noqa: E402

FIXTURES = [("tiny", ""), ("7b_l2", ""), ("7b_l2", "peaked"), ("7b_l2", "peakedperm")]
_STATE = {}


def setup():
    """Shims + the validation batch of the reference's reader (once per process)."""
    if _STATE:
        return _STATE
    M = G.install_shims()                       # Tensor.cuda / half shims + stub tokenizer; the reference first on sys.path
    import llama.model_my_original_mod as M2    # the module that still has the per-option branch
    M2.Tokenizer = M.Tokenizer
    sys.modules.setdefault("pysrt", types.ModuleType("pysrt"))
    real_load = torch.load
    torch.load = lambda p, *a, **k: real_load(p, *a, **{**k, "weights_only": False}) if os.path.exists(p) else {}
    import dataloader as D
    import llama.tokenizer as T
    import pandas as pd

    g = torch.Generator().manual_seed(11)
    feats = {k: torch.randn(n, 768, generator=g) for k, n in GL.FRAMES.items()}
    tmp = tempfile.mkdtemp()
    os.makedirs(os.path.join(tmp, "data", "nextqa", "video_features"))
    rows = GL.ROWS
    cols = {"video": [r[0] for r in rows], "question": [r[1] for r in rows], "answer": [r[2] for r in rows],
            "type": [r[3] for r in rows]}
    for i in range(5):
        cols[f"a{i}"] = [r[4][i] for r in rows]
    pd.DataFrame(cols).to_csv(os.path.join(tmp, "data", "nextqa", "val.csv"), index=False)
    torch.save(feats, os.path.join(tmp, "data", "nextqa", "video_features", "clipvitl14.pth"))
    os.chdir(tmp)
    largs = types.SimpleNamespace(max_feats=10, max_seq_len=128, dataset="nextqa", audio=False, audio_only=False,
                                  audio_merge="none", debug=False, is_generation_task=False)
    tok = object.__new__(T.Tokenizer)
    tok.args, tok.sp_model = largs, FakeSentencePiece()
    tok.n_words, tok.bos_id, tok.eos_id, tok.pad_id = 32000, 1, 2, -1
    tok.v_token_id, tok.q_token_id, tok.a_token_id, tok.nl_id = 15167, 16492, 22550, 13
    ds = D.NextQA(args=largs, tokenizer=tok, split="val")
    _STATE.update(M2=M2, batch=D.batch_collate([ds[i] for i in range(4)]))
    return _STATE


def run(pname: str, mode: str):
    st = setup()
    M2, batch = st["M2"], st["batch"]
    assert mode in ("", "peaked", "peakedperm"), mode
    cfg = synth.preset(pname, vaq=False, qav=False, vocab_size=32000, max_seq_len=128, batch_size=4, peaked=mode == "peaked",
                       peaked_perm=mode == "peakedperm")
    model, margs = G.build_reference(M2, cfg)
    margs.is_generation_task = False
    model.eval()
    with torch.no_grad():
        il = model(batch, inference=True).float()                      # (B, O, S-1)
    count = (il != 0).sum(-1)                                          # reference engine.py:88
    mean = il.sum(-1) / count
    prediction = mean.argmin(-1)                                       # engine.py:93
    two = mean.sort(-1).values[:, :2]
    gap = (two[:, 1] - two[:, 0]) / two[:, 0]
    out = {"individual_losses": il.numpy(), "count": count.numpy().astype(np.int64), "mean": mean.numpy(),
           "prediction": prediction.numpy().astype(np.int64), "gap": gap.numpy().astype(np.float32),
           "text_id_vqa": batch["text_id"]["vqa"].numpy(), "label_vqa": batch["label"]["vqa"].numpy(),
           "prefix_vqa": np.array(batch["prefix_index"]["vqa"], dtype=np.int64),
           "vstart_vqa": np.array(batch["video_start"]["vqa"], dtype=np.int64),
           "answer": batch["answer"].numpy(), "video": batch["video"].numpy(), "qtype": batch["qtype"].numpy()}
    path = os.path.join(ROOT, "tests", "golden", f"score_{pname}{'_' + mode if mode else ''}.npz")
    np.savez_compressed(path, **out)
    print(f"[score_{pname}{'_' + mode if mode else ''}] prediction {out['prediction']} answer {out['answer']} "
          f"gaps {np.array2string(out['gap'], precision=4)} (min {out['gap'].min():.4g}, median {np.median(out['gap']):.4g}) "
          f"mean range [{float(mean.min()):.4f}, {float(mean.max()):.4f}] -> {path} {os.path.getsize(path) // 1024} KiB",
          flush=True)
    del model


def main():
    if len(sys.argv) > 1:
        run(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else "")
        return
    for pname, mode in FIXTURES:
        run(pname, mode)


if __name__ == "__main__":
    main()
