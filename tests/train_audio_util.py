"""Helpers of the --train_audio tests: the product model of an audio mode with the flag on or off, frozen by the MODEL's rule
(Transformer.is_trainable), and the fixtures tools/gen_golden_audio_train.py takes from the reference."""
import torch

import llama
from llama_vqa import fill_closed_form
from tests import audio_util, gpu_util

TINY = ["audio_train_tiny_only", "audio_train_tiny_sum", "audio_train_tiny_attn1", "audio_train_tiny_attn3",
        "audio_train_tiny_attnF"]
WIDE = ["audio_train_7b_l2_b8_sum_peaked", "audio_train_7b_l2_b8_attnF_peaked"]
GOLDENS = TINY + WIDE
AUDIO_PREFIXES = ("audio_proj.", "video_audio_cross_attn.")
# (mode, audio_len): every mode the flag acts on, `attention` with one key, a few, and max_feats
MODES = [("only", 0), ("sum", 0), ("attention", 1), ("attention", 3), ("attention", 0)]


def build_model(cfg, dtype=torch.float32, device="cuda", train_audio=True, fill=True):
    args = gpu_util.make_args(cfg, train_audio=train_audio, **audio_util.audio_args(cfg.audio))
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
    for n, p in model.named_parameters():          # llama_vqa.py's loop: the model's rule, not the bare name rule
        p.requires_grad = model.is_trainable(n)
        if p.requires_grad:
            p.data = p.data.float()
    if fill:
        fill_closed_form(model, cfg)
    return model, args


def audio_names(model):
    return [n for n, _ in model.named_parameters() if n.startswith(AUDIO_PREFIXES)]
