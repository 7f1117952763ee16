"""The audio modes through the outer layers on the GPU: `python train.py --audio ...` on synthetic batches with a resume, and
two data-parallel ranks whose flat buffer holds the 1792-wide visual_proj of `concat`."""
import json
import math
import os
import socket
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_train_py_concat_end_to_end_and_resume(tmp_path):
    """tests/test_train_gpu.py's CLI run — the same flags, the VQA loss — in `concat`: loss finite and falling over a resume
    (measured 10.44 -> 9.65); the checkpoint (trainables only, the reference's key names) holds the 1792-wide visual_proj and no
    audio_proj. (Not with --vaq --qav: at this run's learning rate, blr 0.64, the QAV loss of the synthetic 7B RISES from the first
    epoch to the second with or without audio — video-only 10.9 -> 15.5, concat 16.1 -> 77.6, while VQA and VAQ fall in both — so a
    three-loss total cannot tell a working step from a broken one here.)"""
    pkg = os.path.join(ROOT, "flipped-vqa_amd")
    env = dict(os.environ, FVQA_SYNTHETIC_TOKENIZER="1")
    out = str(tmp_path / "run")
    base = [sys.executable, "train.py", "--model", "7B", "--random_init", "--synthetic", "--synthetic_batches", "6",
            "--batch_size", "4", "--max_seq_len", "128", "--warmup_epochs", "0", "--blr", "0.64", "--output_dir", out,
            "--llama_model_path", str(tmp_path / "no_assets") + "/", "--audio", "--audio_merge", "concat"]
    r = subprocess.run(base + ["--epochs", "1"], cwd=pkg, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    log = [json.loads(x) for x in open(os.path.join(out, "log.txt"))]
    assert len(log) == 1 and log[0]["epoch"] == 0 and math.isfinite(log[0]["train_loss"])
    ck = torch.load(os.path.join(out, "checkpoint_best.pth"), map_location="cpu", weights_only=False)
    assert set(ck) == {"model", "optimizer", "epoch", "scaler", "args"} and ck["epoch"] == 0
    assert len(ck["model"]) == 3 + 2 * 32 and not any("audio" in n for n in ck["model"])
    assert tuple(ck["model"]["visual_proj.weight"].shape) == (4096, 768 + 1024)
    r2 = subprocess.run(base + ["--epochs", "2", "--resume", os.path.join(out, "checkpoint_best.pth")], cwd=pkg, env=env,
                        capture_output=True, text=True, timeout=600)
    assert r2.returncode == 0, (r2.stdout[-1500:], r2.stderr[-1500:])
    log = [json.loads(x) for x in open(os.path.join(out, "log.txt"))]
    assert [x["epoch"] for x in log] == [0, 1]
    assert math.isfinite(log[1]["train_loss"]) and log[1]["train_loss"] < log[0]["train_loss"]


def test_train_py_audio_only_writes_no_visual_proj(tmp_path):
    pkg = os.path.join(ROOT, "flipped-vqa_amd")
    env = dict(os.environ, FVQA_SYNTHETIC_TOKENIZER="1")
    out = str(tmp_path / "run")
    cmd = [sys.executable, "train.py", "--model", "7B", "--random_init", "--synthetic", "--synthetic_batches", "3",
           "--batch_size", "2", "--max_seq_len", "128", "--warmup_epochs", "0", "--blr", "0.64", "--output_dir", out,
           "--llama_model_path", str(tmp_path / "no_assets") + "/", "--audio", "--audio_only", "--adapter_layer", "2",
           "--epochs", "1"]
    r = subprocess.run(cmd, cwd=pkg, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    log = [json.loads(x) for x in open(os.path.join(out, "log.txt"))]
    assert math.isfinite(log[0]["train_loss"])
    ck = torch.load(os.path.join(out, "checkpoint_best.pth"), map_location="cpu", weights_only=False)
    assert "visual_proj.weight" not in ck["model"] and "temporal_emb.weight" in ck["model"]
    assert not any("audio" in n for n in ck["model"])


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.mark.parametrize("mode", ["concat", "sum"])
def test_two_audio_replicas_stay_bitwise_equal(tmp_path, mode):
    """Two ranks (train.py's wiring, tests/audio_dp_worker.py) that start from different trainables AND different frozen audio
    weights leave DataParallel's constructor with rank 0's of both and hold bitwise-equal parameters after every step; in `concat`
    the flat buffer carries the 1792-wide visual_proj and both of its column ranges are stepped."""
    from tests import audio_dp_worker as W
    world, port = 2, str(_free_port())
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="4")
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "audio_dp_worker.py"), str(r), str(world), port,
                               str(tmp_path), mode], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
             for r in range(world)]
    outs = [p.communicate(timeout=600)[0] for p in procs]
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o[-3000:]
    t0, t1 = (torch.load(tmp_path / f"rank{r}.pt") for r in range(world))
    off, size, shape = t0["visual_proj"]
    K = 768 + 1024 if mode == "concat" else 768
    assert shape == (256, K) and size == 256 * K and t0["numel"] == t1["numel"] > size
    assert t0["names"] == t1["names"] and "visual_proj.weight" in t0["names"]
    assert torch.equal(t0["p_init"], t1["p_init"])            # rank 0's start on both, although rank 1 was perturbed otherwise
    if mode == "sum":
        assert t0["audio_proj"] is not None and torch.equal(t0["audio_proj"], t1["audio_proj"])
    prev = t0["p_init"]
    for i in range(W.N_STEPS):
        assert torch.equal(t0[f"p{i}"], t1[f"p{i}"]), f"replicas diverged at step {i}"
        assert math.isfinite(t0[f"loss{i}"]) and math.isfinite(t1[f"loss{i}"])
        w_now, w_prev = t0[f"p{i}"][off:off + size].view(shape), prev[off:off + size].view(shape)
        assert not torch.equal(w_now[:, :768], w_prev[:, :768])
        if mode == "concat":                                  # the audio columns of the one weight are trained as well
            assert not torch.equal(w_now[:, 768:], w_prev[:, 768:])
        prev = t0[f"p{i}"]


def test_concat_generation_matches_reference():
    """Greedy generation in `concat` against the reference's own (tools/gen_golden_audio_eval.py; permuted peaked LM head, so the
    31 ids of a row all differ): fp32 build, exact ids, chosen options and similarities as tests/test_eval.py asks of eval_tiny. The
    prefill goes through the same front end as the training step; the sub-batch it builds carries "audio"."""
    import numpy as np
    from fvqa import synth
    from tests import audio_util
    from tests.parity import load_golden
    from tests.test_eval import golden_batch
    g = load_golden("audio_eval_tiny_concat_peakedperm")
    pi = synth.vocab_permutation(32000).numpy()
    for b in range(g["ids_after"].shape[0]):                  # the fixture moves along the permutation
        p0 = int(g["prefix_vqa"][b])
        gen = g["ids_after"][b, p0:p0 + 31]
        assert len(set(gen.tolist())) == len(gen) >= 20 and np.array_equal(gen[1:], pi[gen[:-1]])
    cfg = synth.preset("tiny", vaq=False, qav=False, vocab_size=32000, max_seq_len=128, batch_size=4, peaked_perm=True,
                       audio="concat")
    model, _ = audio_util.build_model(cfg, torch.float32)
    model.eval()
    batch = golden_batch(g)
    batch["audio"] = torch.from_numpy(g["audio"])
    best, extracted = model(batch, inference=True)
    ids = model.last_generation["ids"].cpu().numpy()
    assert ids.shape == g["ids_after"].shape and len(extracted) == ids.shape[0]
    assert np.array_equal(ids, g["ids_after"])
    assert np.array_equal(best.cpu().numpy(), g["best"])
    assert np.allclose(model.last_generation["similarities"].cpu().numpy(), g["sims"], atol=2e-5)
    no_audio = dict(batch)
    del no_audio["audio"]
    with pytest.raises(KeyError):                             # a missing feature is an error, not a video-only fallback
        model(no_audio, inference=True)
    assert torch.isfinite(model(synth.make_batch(cfg, seed=0))[0])      # the training path still works on the same engine
