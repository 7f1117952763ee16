"""The generation API without a GPU: the new C entry is exported by both builds and refuses bad operands before any launch,
`prompt_batch` builds the prompt the validation reader builds, the new command-line flags exist and reach the loader, and the
sampling rule of include/fvqa.h (fvqa_decode_next), stated here in fp64 numpy, reproduces the supports observed from the
reference's own sampler (tests/golden/sampler_support.npz, tools/gen_golden_generate.py)."""
import ctypes as C
import json
import os
import sys
import types

import numpy as np
import pandas as pd
import pytest
import torch

import dataloader
from fvqa import _lib, generate
from llama.tokenizer import Tokenizer
from oracle.fake_sp import FakeSentencePiece

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
A = C.c_void_p(256)
BUILDS = [("bf16", _lib.BF16), ("f16", _lib.F16)]


def kept_set(logits, T, top_p):
    """The rule in fp64: p = softmax(logits / T); order by p descending, ties by index ascending; a token is kept iff the
    total probability in front of it is <= top_p. -> (sorted kept indices, p)."""
    x = np.asarray(logits, dtype=np.float64) / T
    p = np.exp(x - x.max())
    p /= p.sum()
    order = np.lexsort((np.arange(p.size), -p))
    front = np.cumsum(p[order]) - p[order]
    return np.sort(order[front <= top_p]), p


def _args(dt, temperature=0.0, top_p=1.0, u=A):
    #      logits u emb  T           top_p  eos stop ids pos done x  tok kept act pos64 B  V    D    S   dtype stream
    return [A, u, A, temperature, top_p, 2, 1, A, A, A, A, A, A, A, A, 3, 509, 128, 16, dt, None]


@pytest.mark.parametrize("which,h16", BUILDS)
def test_decode_next_is_exported_and_checks_its_operands_on_the_host(which, h16):
    """Every call here must be refused: one that passed validation would launch a kernel on fake addresses."""
    lib = _lib.load(which)
    assert lib.fvqa_version() == _lib.ABI_VERSION == 18          # an added entry changes no signature
    fn = lib.fvqa_decode_next
    assert len(_args(h16)) == len(_lib.SIGNATURES["fvqa_decode_next"][1])
    for dt in (h16, _lib.F32):
        base = _args(dt, temperature=0.7, top_p=0.9)
        for at in (0, 1, 2, 7, 8, 9, 10, 11, 12, 13):             # every required pointer; u is required when sampling
            a = list(base)
            a[at] = None
            assert fn(*a) == -1, at
        for at in (15, 16, 17, 18):                               # B, V, D, S <= 0
            for bad in (0, -4):
                a = list(base)
                a[at] = bad
                assert fn(*a) == -2, (at, bad)
        for t in (-0.5, float("nan")):
            assert fn(*_args(dt, temperature=t, top_p=0.9)) == -1, t
        for p in (0.0, -0.1, 1.0001, float("nan")):
            assert fn(*_args(dt, temperature=0.7, top_p=p)) == -1, p
        a = list(base)
        a[0] = C.c_void_p(258)                                    # fp32 logits off their 4-byte boundary
        assert fn(*a) == -3
    other = _lib.F16 if h16 == _lib.BF16 else _lib.BF16
    assert fn(*_args(other)) == -1                                # the other build's 16-bit code
    assert fn(*_args(7)) == -1


# ------------------------------------------------------------------------------------------------ prompt_batch
G = dict(np.load(os.path.join(GOLDEN, "loader_nextqa.npz")))


@pytest.fixture(scope="module")
def data_root(tmp_path_factory):
    root = tmp_path_factory.mktemp("data")
    rows = json.loads(str(G["rows_json"]))
    cols = {"video": [r[0] for r in rows], "question": [r[1] for r in rows], "answer": [r[2] for r in rows],
            "type": [r[3] for r in rows]}
    for i in range(5):
        cols[f"a{i}"] = [r[4][i] for r in rows]
    os.makedirs(root / "nextqa" / "video_features")
    pd.DataFrame(cols).to_csv(root / "nextqa" / "val.csv", index=False)
    torch.save({str(k): torch.from_numpy(G[f"feat__{k}"]) for k in G["feat_names"]},
               root / "nextqa" / "video_features" / "clipvitl14.pth")
    return str(root), rows


def _reader(root, gen, **kw):
    args = types.SimpleNamespace(max_feats=10, max_seq_len=128, dataset="nextqa", audio=False, audio_only=False,
                                 audio_merge="none", debug=False, is_generation_task=gen, synthetic=True, data_root=root, **kw)
    tok = Tokenizer("/nonexistent/tokenizer.model", args)
    tok.sp_model = FakeSentencePiece()
    return dataloader.NextQA(args=args, tokenizer=tok, split="val"), tok, args


@pytest.mark.parametrize("gen", [True, False])
def test_prompt_batch_is_the_val_readers_prompt(data_root, gen):
    """Generation mode: the question alone; multiple choice (`options`): the lettered choices after it, as the reader writes
    o_text. Either way every position in front of prefix_index equals the reader's row (pinned to the reference by
    loader_nextqa.npz), everything from it on is 0, and video_start / prefix_index are the reader's."""
    root, rows = data_root
    ds, tok, _ = _reader(root, gen)
    samples = [ds[i] for i in range(len(ds))]
    name = "s128_gen_val" if gen else "s128_val"
    assert np.array_equal(torch.stack([s["text_id"]["vqa"] for s in samples]).numpy(), G[f"{name}__text_id__vqa"])
    fits = [i for i, s in enumerate(samples) if s["prefix_index"]["vqa"] <= 127]
    assert len(fits) >= 4
    feats = [torch.from_numpy(G[f"feat__{rows[i][0]}"]) if f"feat__{rows[i][0]}" in G else torch.zeros(1, 768) for i in fits]
    b = generate.prompt_batch(tok, [rows[i][1] for i in fits], video=feats,
                              options=None if gen else [rows[i][4] for i in fits], max_seq_len=128, max_feats=10)
    assert set(b["text_id"]) == {"vqa"} and b["text_id"]["vqa"].shape == (len(fits), 1, 128)
    assert "answer" not in b
    for k, i in enumerate(fits):
        s = samples[i]
        p = s["prefix_index"]["vqa"]
        assert b["prefix_index"]["vqa"][k] == p and b["video_start"]["vqa"][k] == s["video_start"]["vqa"]
        row = b["text_id"]["vqa"][k, 0]
        assert torch.equal(row[:p], s["text_id"]["vqa"][0, :p])
        assert int(row[p:].abs().sum()) == 0
        assert torch.equal(b["video"][k], s["video"])
    assert b["label"]["vqa"].shape == b["text_id"]["vqa"].shape


def test_prompt_batch_refuses_a_prompt_that_does_not_fit(data_root):
    root, rows = data_root
    _, tok, _ = _reader(root, True)
    q = rows[0][1]
    p = generate.prompt_batch(tok, [q], max_seq_len=128, max_feats=10)["prefix_index"]["vqa"][0]
    generate.prompt_batch(tok, [q], max_seq_len=p + 1, max_feats=10)           # exactly max_seq_len - 1: fits
    with pytest.raises(ValueError):
        generate.prompt_batch(tok, [q], max_seq_len=p, max_feats=10)
    with pytest.raises(ValueError):
        generate.prompt_batch(tok, [q + " and then " * 60], max_seq_len=128, max_feats=10)


# ------------------------------------------------------------------------------------------------ flags
def test_new_flags_and_the_val_batch_size(data_root):
    import train
    a = train.get_args_parser().parse_args([])
    assert a.gen_stop_eos is False and a.val_batch_size is None
    a = train.get_args_parser().parse_args(["--gen_stop_eos", "--val_batch_size", "32"])
    assert a.gen_stop_eos is True and a.val_batch_size == 32
    root, _ = data_root
    _, tok, args = _reader(root, True, batch_size=2, num_workers=0, pin_mem=False)
    assert dataloader.load_data(args, tok, split="val").batch_size == 2
    args.val_batch_size = None
    assert dataloader.load_data(args, tok, split="val").batch_size == 2
    args.val_batch_size = 3
    assert dataloader.load_data(args, tok, split="val").batch_size == 3
    pd.read_csv(os.path.join(root, "nextqa", "val.csv")).to_csv(os.path.join(root, "nextqa", "train.csv"), index=False)
    assert dataloader.load_data(args, tok, split="train").batch_size == 2


def test_answer_cli_parses_the_documented_line():
    sys.path.insert(0, os.path.join(ROOT, "flipped-vqa_amd"))
    import answer
    a = answer.get_args_parser().parse_args(
        ["--model", "7B", "--llama_model_path", "./pretrained/llama/", "--resume", "ckpt.pth", "--features", "clip.pth",
         "--audio_features", "clip_audio.npy", "--question", "what is the man doing", "--options", "a", "b", "c",
         "--max_new_tokens", "31", "--temperature", "0", "--top_p", "1", "--seed", "0"])
    assert a.question == "what is the man doing" and a.options == ["a", "b", "c"] and a.features == "clip.pth"
    assert a.max_new_tokens == 31 and a.temperature == 0.0 and a.top_p == 1.0 and a.seed == 0 and a.resume == "ckpt.pth"
    assert a.dtype == "bf16" and a.audio is False
    a = answer.get_args_parser().parse_args(["--random_init", "--synthetic", "--question", "why"])
    assert a.options is None and a.seed is None and a.random_init and a.synthetic
    ids = answer.WordHashVocabulary(32000).encode("Question: Why?\nAnswer: The answer is x")
    assert ids.count(22550) == 1 and ids.count(16492) == 1 and ids.count(13) == 1 and min(ids) >= 3 and max(ids) < 32000
    assert len(ids) - (ids.index(22550) + 5) == 1                    # the layouts' "answer starts 5 tokens after Answer"


# ------------------------------------------------------------------------------------------------ the rule
def test_the_rule_reproduces_the_reference_samplers_supports():
    S = np.load(os.path.join(GOLDEN, "sampler_support.npz"))
    assert S["logits"].shape == (4, 512) and int(S["draws"]) == 50000
    sizes = []
    for lg, (r, T, top_p), sup in zip(S["logits"], S["params"], S["support"]):
        sup = sup[sup >= 0]
        kept, p = kept_set(lg, T, top_p)
        assert np.array_equal(kept, sup), (r, T, top_p)
        # the fixture's premises: no boundary within 5e-3 of top_p, every kept token likely enough to be seen in 50 000 draws
        front = np.cumsum(np.sort(p)[::-1]) - np.sort(p)[::-1]
        assert np.abs(front - top_p).min() >= 5e-3 and p[kept].min() >= 1e-2
        sizes.append(kept.size)
    assert sizes[:3] == [7, 5, 5]
