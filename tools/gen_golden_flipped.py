#!/usr/bin/env python3
"""TEST INFRASTRUCTURE — generates tests/golden/flipped_<preset>[_<variant>][_gen].npz: per answer option the three flipped losses
of the reference (VQA, VAQ, QAV), the way tools/gen_golden_score.py makes the VQA-only fixtures. Needs the reference checkout.

The validation batch comes from the reference's own NExT-QA reader on a table of this script: four samples, five options,
questions of 4, 12, 35 and 75 words, so that the VAQ suffix of a sample — from the answer, where the options differ, to the end
of the question — is below 16 rows, between 17 and 32, between 33 and 64 and above 64 (sequences of 192 positions: at 128 the
longest would be cut). `_gen` fixtures use the reader with is_generation_task=True: the options are the answer TEXTS, of
different lengths.

The oracle: the fp32-shim reference model with vaq = qav = True, its TRAINING forward (llama/model.py:250-365) called on one
(sample, option) row at a time with that option's ids, the VQA label of the reader and the VAQ / QAV labels and frame indices of
fvqa.flipped.option_rows (each option at its own positions); the three returned losses are that option's means.

Stored: the batch with the reader's own labels and indices, mean_{vqa,vaq,qav} (B, O), count_{vqa,vaq,qav}, and per task and for
the total (the sum of the three) `gap` = (second-lowest - lowest) / lowest over the options of a sample: how decided the
reference's own choice is — what a prediction can be compared on.

usage: gen_golden_flipped.py [<preset> [peakedperm] [gen]]       (no arguments: every fixture below, gaps printed)
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
from fvqa import flipped, synth  # noqa: E402
import oracle.gen_golden as G  # noqa: E402
import oracle.gen_golden_loader as GL  # noqa: E402
from oracle.fake_sp import FakeSentencePiece  # noqa: E402

S = 192
F = 10
TASKS = ("vqa", "vaq", "qav")
FIXTURES = [("tiny", "", False), ("tiny", "", True), ("7b_l2", "peakedperm", False)]
WORDS = ("the man in a red shirt walks slowly across green field near old wooden house while two small dogs run behind him and "
         "his friend waves from window before they all sit down under big tree to eat some bread with cheese as sun sets over "
         "hills far away then children arrive on bikes carrying bags full of apples which they share among everyone there until "
         "night falls").split()


def question(n_words: int, lead: str) -> str:
    return " ".join([lead] + WORDS[: n_words - 1])


ROWS = [  # video, question, answer, type, a0..a4
    ("v3", question(4, "why"), 2, "CW", ["to play", "it is scared", "chasing a ball", "to eat", "for fun"]),
    ("v10", question(12, "how"), 0, "DC", ["two", "three of them", "four", "five", "six people in all"]),
    ("v16", question(35, "what"), 4, "TN", ["stand up", "wave", "sleep", "eat", "read a book"]),
    ("v25", question(75, "where"), 1, "DL", ["park", "in the kitchen", "beach", "school", "car"]),
]
_STATE = {}


def setup(gen: bool):
    """Shims + the validation batch of the reference's reader (once per process and reader mode)."""
    if "M" not in _STATE:
        _STATE["M"] = G.install_shims()         # Tensor.cuda / half shims + stub tokenizer; the reference first on sys.path
        sys.modules.setdefault("pysrt", types.ModuleType("pysrt"))
        real_load = torch.load
        torch.load = lambda p, *a, **k: real_load(p, *a, **{**k, "weights_only": False}) if os.path.exists(p) else {}
    if gen in _STATE:
        return _STATE["M"], _STATE[gen]
    import dataloader as D
    import llama.tokenizer as T
    import pandas as pd

    g = torch.Generator().manual_seed(11)
    feats = {k: torch.randn(n, 768, generator=g) for k, n in GL.FRAMES.items()}
    tmp = tempfile.mkdtemp()
    os.makedirs(os.path.join(tmp, "data", "nextqa", "video_features"))
    cols = {"video": [r[0] for r in ROWS], "question": [r[1] for r in ROWS], "answer": [r[2] for r in ROWS],
            "type": [r[3] for r in ROWS]}
    for i in range(5):
        cols[f"a{i}"] = [r[4][i] for r in ROWS]
    pd.DataFrame(cols).to_csv(os.path.join(tmp, "data", "nextqa", "val.csv"), index=False)
    torch.save(feats, os.path.join(tmp, "data", "nextqa", "video_features", "clipvitl14.pth"))
    cwd = os.getcwd()
    os.chdir(tmp)
    largs = types.SimpleNamespace(max_feats=F, max_seq_len=S, dataset="nextqa", audio=False, audio_only=False,
                                  audio_merge="none", debug=False, is_generation_task=gen)
    tok = object.__new__(T.Tokenizer)
    tok.args, tok.sp_model = largs, FakeSentencePiece()
    tok.n_words, tok.bos_id, tok.eos_id, tok.pad_id = 32000, 1, 2, -1
    tok.v_token_id, tok.q_token_id, tok.a_token_id, tok.nl_id = 15167, 16492, 22550, 13
    ds = D.NextQA(args=largs, tokenizer=tok, split="val")
    _STATE[gen] = D.batch_collate([ds[i] for i in range(len(ROWS))])
    os.chdir(cwd)
    return _STATE["M"], _STATE[gen]


def gaps(v: torch.Tensor) -> np.ndarray:
    two = v.sort(-1).values[:, :2]
    return ((two[:, 1] - two[:, 0]) / two[:, 0]).numpy().astype(np.float32)


def run(pname: str, mode: str, gen: bool):
    M, batch = setup(gen)
    assert mode in ("", "peakedperm"), mode
    cfg = synth.preset(pname, vaq=True, qav=True, vocab_size=32000, max_seq_len=S, batch_size=1, peaked_perm=mode == "peakedperm")
    model, _ = G.build_reference(M, cfg)
    model.eval()
    ids = batch["text_id"]
    B, O, _ = ids["vqa"].shape
    rows = flipped.option_rows(batch, F)
    vs = batch["video_start"]
    mean = torch.zeros(3, B, O)
    with torch.no_grad():
        for n in range(B):
            for c in range(O):
                one = {"video": batch["video"][n:n + 1], "text_id": {t: ids[t][n:n + 1, c:c + 1] for t in TASKS},
                       "label": {"vqa": batch["label"]["vqa"][n:n + 1, c:c + 1], "vaq": rows["label"]["vaq"][n:n + 1, c:c + 1],
                                 "qav": rows["label"]["qav"][n:n + 1, c:c + 1]},
                       "video_start": {"vqa": [int(vs["vqa"][n])], "vaq": [int(vs["vaq"][n])]},
                       "video_index": {"qav": rows["video_index"]["qav"][n, c][None]}}
                mean[:, n, c] = torch.stack([x.float().reshape(()) for x in model(one)])
    count = {"vqa": (batch["label"]["vqa"][:, :, 1:] > 0).sum(-1), "vaq": (rows["label"]["vaq"][:, :, 1:] > 0).sum(-1),
             "qav": (rows["label"]["qav"][:, :, 1:] >= 0).sum(-1)}
    out = {"answer": batch["answer"].numpy(), "video": batch["video"].numpy(), "qtype": batch["qtype"].numpy(),
           "gap_total": gaps(mean.sum(0)), "is_generation_task": np.array(gen)}
    for k, t in enumerate(TASKS):
        out[f"text_id_{t}"] = ids[t].numpy()
        out[f"reader_label_{t}"] = batch["label"][t].numpy()
        out[f"reader_prefix_{t}"] = np.array(batch["prefix_index"][t], dtype=np.int64)
        out[f"mean_{t}"] = mean[k].numpy()
        out[f"count_{t}"] = count[t].numpy().astype(np.int64)
        out[f"gap_{t}"] = gaps(mean[k])
    out["vstart_vqa"] = np.array(vs["vqa"], dtype=np.int64)
    out["vstart_vaq"] = np.array(vs["vaq"], dtype=np.int64)
    out["reader_video_index_qav"] = batch["video_index"]["qav"].numpy()
    name = f"flipped_{pname}{'_' + mode if mode else ''}{'_gen' if gen else ''}"
    path = os.path.join(ROOT, "tests", "golden", name + ".npz")
    np.savez_compressed(path, **out)
    # what the tests can compare predictions on: a gap above four times the bound they hold the means to
    lcp = {t: [int(torch.nonzero((ids[t][n] != ids[t][n, :1]).any(0))[0]) for n in range(B)] for t in TASKS}
    print(f"[{name}] answer {out['answer']} first difference {lcp}", flush=True)
    for t in TASKS + ("total",):
        g = out[f"gap_{t}"]
        pred = (mean.sum(0) if t == "total" else mean[TASKS.index(t)]).argmin(-1).tolist()
        print(f"[{name}] {t}: prediction {pred} gaps {np.array2string(g, precision=4)} samples with gap > 4e-3 (fp32 bar 1e-3 x 4): "
              f"{np.nonzero(g > 4e-3)[0].tolist()}", flush=True)
    print(f"[{name}] mean range [{float(mean.min()):.4f}, {float(mean.max()):.4f}] -> {path} {os.path.getsize(path) // 1024} KiB",
          flush=True)
    del model


def main():
    if len(sys.argv) > 1:
        run(sys.argv[1], "peakedperm" if "peakedperm" in sys.argv[2:] else "", "gen" in sys.argv[2:])
        return
    for pname, mode, gen in FIXTURES:
        run(pname, mode, gen)


if __name__ == "__main__":
    main()
