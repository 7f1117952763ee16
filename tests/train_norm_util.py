"""Helpers of the --train_norm tests: the product model with the flag on or off, frozen by the MODEL's rule
(Transformer.is_trainable), and the fixtures tools/gen_golden_norm_train.py takes from the reference."""
import torch

import llama
from fvqa import synth
from llama_vqa import fill_closed_form
from tests import gpu_util

TINY = ["norm_train_tiny_all", "norm_train_tiny_vqa", "norm_train_tiny_l3_a2_all"]
WIDE = ["norm_train_7b_l2_b8_all_peaked"]
GOLDENS = TINY + WIDE


def build_model(cfg, dtype=torch.float32, device="cuda", train_norm=True, fill=True):
    args = gpu_util.make_args(cfg, train_norm=train_norm)
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


def norm_names(model):
    """The norm weights the flag trains, in the flat block's order."""
    return synth.norm_train_names(model.engine_layer_ids())


def all_norm_names(model):
    return [n for n, _ in model.named_parameters() if n == "norm.weight" or n.endswith(("attention_norm.weight", "ffn_norm.weight"))]
