"""Helpers of the audio-fusion tests: the reference's three audio arguments from a SynthConfig, the product model in an audio
mode, and a step runner that does not need `batch["video"]` (the audio-only batch has none)."""
import json

import torch

import llama
from fvqa import synth
from llama_vqa import fill_closed_form
from tests import gpu_util
from tests.parity import load_golden

GOLDENS = ["audio_tiny_only", "audio_tiny_concat", "audio_tiny_sum", "audio_tiny_attn1", "audio_tiny_attnF",
           "audio_7b_l2_b8_concat_peaked", "audio_7b_l2_b8_attn1_peaked"]


def audio_args(mode: str) -> dict:
    """SynthConfig.audio -> (audio, audio_only, audio_merge) as train.validate_args leaves them."""
    if mode == "none":
        return dict(audio=False, audio_only=False, audio_merge="none")
    if mode == "only":
        return dict(audio=True, audio_only=True, audio_merge=None)
    return dict(audio=True, audio_only=False, audio_merge=mode)


def golden_cfg(name: str):
    """(fixture, SynthConfig it was generated from): the case travels inside the fixture (tools/gen_golden_audio.py)."""
    g = load_golden(name)
    return g, synth.preset(str(g["case_preset"]), **json.loads(str(g["case_over"])))


def build_model(cfg, dtype=torch.float32, device="cuda", fill=True):
    args = gpu_util.make_args(cfg, **audio_args(cfg.audio))
    ma = llama.ModelArgs(max_seq_len=cfg.max_seq_len, max_batch_size=32, adapter_len=cfg.adapter_len,
                         adapter_layer=cfg.adapter_layer, **cfg.params_json())
    ma.vocab_size = cfg.vocab_size
    prev = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        with torch.device(device):
            model = llama.Transformer(ma, args)
    finally:
        torch.set_default_dtype(prev)
    for n, p in model.named_parameters():          # llama_vqa.py:71-76
        p.requires_grad = synth.is_trainable(n)
        if p.requires_grad:
            p.data = p.data.float()
    if fill:
        fill_closed_form(model, cfg)
    return model, args


def run_step(model, batch, loss_weights=(1.0, 1.0, 1.0), lm_head="all"):
    """tests.gpu_util.run_step for a batch that may have no "video": that helper reads the batch size from it."""
    if "video" in batch:
        return gpu_util.run_step(model, batch, loss_weights, lm_head)
    B = batch["text_id"]["vqa"].shape[0]
    shaped = dict(batch, video=torch.empty(B, 0))       # read for its first dimension only; the audio-only model never looks at it
    return gpu_util.run_step(model, shaped, loss_weights, lm_head)
