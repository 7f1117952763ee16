#!/usr/bin/env python3
"""Option-scoring measurement on the MI355X box (fvqa/score.py): `score_options` in both routes on a make_option_batch —
7B full depth, bf16, B = 8, five options, S = 128 by default — interleaved (shared, dense, shared, dense ...) after a warm-up
of each, every call bracketed by device events; the shared route's prompt pass and suffix pass on their own; which GEMM kernel
took the suffix rows' projections (the library's launch record + fvqa_gemm_sk_describe). With --errors: the per-option-mean
errors of both routes against the reference-generated 7B-width fixture in bf16 and fp16 — the figures the bounds of
tests/test_score_gpu.py are set from. With --frame_attention: the cost of score_options(frame_attention=True), the keyword off and
on in interleaved pairs on both routes (profiles/score_frame_attention.log). With --vocab N_MEMBERS: fvqa.vocab.score_vocab's tree
route, its dense route and generate(constraints=..., num_beams=8) on one vocabulary, interleaved, and the tree attention's time per
layer beside the layer's projections; with --vocab_errors: the errors its tests' bounds are set from (profiles/score_vocab.log).
Everything is appended to --log (profiles/score_options.log)."""
import argparse
import ctypes as C
import os
import statistics
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "flipped-vqa_amd"))
os.environ.setdefault("FVQA_SYNTHETIC_TOKENIZER", "1")
import numpy as np  # noqa: E402
import torch  # noqa: E402

import llama  # noqa: E402
from fvqa import _lib, build, ops, score, synth  # noqa: E402
from llama_vqa import fill_closed_form  # noqa: E402

PIN = "score_7b_l2_peakedperm"


def make_model(cfg, dtype):
    args = types.SimpleNamespace(
        max_feats=cfg.max_feats, bias=cfg.bias, tau=cfg.tau, llama_model_path="/nonexistent/", vaq=False, qav=False,
        synthetic=True, vocab_size=cfg.vocab_size, audio=False, audio_only=False, audio_merge="none", debug=False)
    ma = llama.ModelArgs(max_seq_len=cfg.max_seq_len, max_batch_size=32, adapter_len=cfg.adapter_len,
                         adapter_layer=cfg.adapter_layer, **cfg.params_json())
    ma.vocab_size = cfg.vocab_size
    prev = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        with torch.device("cuda"):
            model = llama.Transformer(ma, args)
    finally:
        torch.set_default_dtype(prev)
    for n, p in model.named_parameters():
        p.requires_grad = synth.is_trainable(n)
        if p.requires_grad:
            p.data = p.data.float()
    fill_closed_form(model, cfg)
    return model.eval()


def ms(ev):
    return ev[1].elapsed_time(ev[2])


def timing(a, say):
    cfg = synth.preset("7b", vaq=False, qav=False, batch_size=a.batch_size, n_layers=a.n_layers, adapter_layer=a.n_layers)
    model = make_model(cfg, torch.bfloat16)
    eng = model.ensure_engine()
    batch = synth.make_option_batch(cfg, n_options=a.n_options, seed=1)
    plan = score.plan_options(batch["text_id"]["vqa"], batch["label"]["vqa"], batch["prefix_index"]["vqa"],
                              batch["video_start"]["vqa"], cfg.max_feats)
    B, O, S, T = a.batch_size, a.n_options, cfg.max_seq_len, plan.T
    rows_sh, rows_de = B * S + B * O * T, B * O * S
    say(f"shape: 7B width, {a.n_layers} layers, bf16, B={B}, O={O}, S={S}; suffix rows per option T={T} "
        f"(lengths {plan.length.tolist()}), scored rows {plan.rows.shape[0]}")
    say(f"rows through the layers: shared {rows_sh} (prompt {B * S} + suffix {B * O * T}), dense {rows_de}: "
        f"{rows_de / rows_sh:.2f}x fewer")
    for r in ("shared", "dense"):
        for _ in range(a.warmup):
            score.score_options(eng, batch, route=r)
    torch.cuda.synchronize()
    # outputs of the two routes on this batch (faster and different is not faster)
    rs, rd = score.score_options(eng, batch, route="shared"), score.score_options(eng, batch, route="dense")
    d = float(((rs["mean"] - rd["mean"]).abs() / rd["mean"].abs()).max())
    say(f"outputs: per-option mean, shared vs dense, largest relative difference {d:.3e}; predictions equal on "
        f"{int((rs['prediction'] == rd['prediction']).sum())} of {B} samples; counts equal: "
        f"{bool(torch.equal(rs['count'], rd['count']))}")
    total = {"shared": [], "dense": []}
    parts = {"prompt pass": [], "suffix pass": []}
    for _ in range(a.reps):
        for r in ("shared", "dense"):
            ev = []
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            score.score_options(eng, batch, route=r, events=ev)
            e1.record()
            e1.synchronize()
            total[r].append(e0.elapsed_time(e1))
            for x in ev:
                if x[0] in parts:
                    parts[x[0]].append(ms(x))
    med = {k: statistics.median(v) for k, v in {**total, **parts}.items()}
    for k in ("shared", "dense"):
        v = total[k]
        say(f"score_options {k:6s}: median {med[k]:8.3f} ms  min {min(v):8.3f}  max {max(v):8.3f}  ({a.reps} reps, interleaved)")
    say(f"  shared route, prompt pass alone: median {med['prompt pass']:8.3f} ms; suffix pass alone (layers on "
        f"{B * O * T} rows + head on the scored rows + pick): median {med['suffix pass']:8.3f} ms")
    say(f"  dense / shared = {med['dense'] / med['shared']:.2f}x")
    # which GEMM kernel took the suffix rows' projections
    R = B * O * T
    ops.gemm_timing_enable(True, 1)
    try:
        score.score_options(eng, batch, route="shared")
        rec = ops.gemm_timing_read()
    finally:
        ops.gemm_timing_enable(False)
    fl = {"qkv": 2.0 * R * 3 * eng.D * eng.D, "wo": 2.0 * R * eng.D * eng.D, "w13": 2.0 * R * 2 * eng.Hf * eng.D,
          "w2": 2.0 * R * eng.D * eng.Hf}
    say(f"launch record of one shared call: {len(rec)} launches of the persistent GEMM kernels")
    for name, f in fl.items():
        mine = [(us, k) for (us, flops, k) in rec if abs(flops - f) < 1.0]
        if not mine:
            say(f"  {name:4s} ({R} rows): not the persistent kernel (no launch of {f:.3g} FLOP in the record): the 128 x 128 kernel")
            continue
        kinds = sorted({k for _, k in mine})
        us = statistics.median([u for u, _ in mine if u >= 0] or [float('nan')])
        what = ["4-wave whole-tile kernel" if k & 128 else "persistent 256-row kernel" + (", split-K" if k & 16 else "")
                for k in kinds]
        say(f"  {name:4s} ({R} rows): {len(mine)} launches, kind {kinds} = {what}, median {us:.1f} us")
    keys = ("tm", "tn", "nw_tile", "gran", "gpt", "ts", "mgroups", "n_teams", "full", "rem", "s", "pstride")
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    for name, (N, K) in {"qkv": (3 * eng.D, eng.D), "wo": (eng.D, eng.D), "w13": (2 * eng.Hf, eng.D),
                         "w2": (eng.D, eng.Hf)}.items():
        plan_ = (C.c_int32 * 16)()
        _lib.load().fvqa_gemm_sk_describe(R, N, K, _lib.BF16, min(n_cu, 256), C.cast(plan_, C.c_void_p), -1, None, 0)
        say(f"  fvqa_gemm_sk_describe({R}, {N}, {K}): " + " ".join(f"{k}={v}" for k, v in zip(keys, plan_)))
    return med


def frame_attention_cost(a, say):
    """What score_options(frame_attention=True) costs: the keyword off and on, interleaved in pairs, on both routes (the shared
    route swaps fvqa_attn_suffix for fvqa_attn_suffix_mass in every layer; the dense route adds one fvqa_attn_row_mass launch
    per layer on its arena) — 7B, full depth, bf16, B x five options as `timing`."""
    if a.reps < 3:
        sys.exit("--frame_attention: at least 3 pairs (--reps)")
    cfg = synth.preset("7b", vaq=False, qav=False, batch_size=a.batch_size, n_layers=a.n_layers, adapter_layer=a.n_layers)
    model = make_model(cfg, torch.bfloat16)
    eng = model.ensure_engine()
    batch = synth.make_option_batch(cfg, n_options=a.n_options, seed=1)
    say(f"frame_attention cost: 7B width, {a.n_layers} layers, bf16, B={a.batch_size} x {a.n_options} options, S={cfg.max_seq_len}, "
        f"{a.reps} interleaved (off, on) pairs per route after {a.warmup} warm-up calls of each")
    for r in score.ROUTES:
        for kw in ({}, {"frame_attention": True}):
            for _ in range(a.warmup):
                out = score.score_options(eng, batch, route=r, **kw)
        torch.cuda.synchronize()
        fa = out["frame_attention"]
        t = {False: [], True: []}
        for _ in range(a.reps):
            for on in (False, True):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                score.score_options(eng, batch, route=r, **({"frame_attention": True} if on else {}))
                e1.record()
                e1.synchronize()
                t[on].append(e0.elapsed_time(e1))
        m0, m1 = statistics.median(t[False]), statistics.median(t[True])
        say(f"  {r:6s}: off median {m0:8.3f} ms (min {min(t[False]):8.3f}, max {max(t[False]):8.3f}); on median {m1:8.3f} ms "
            f"(min {min(t[True]):8.3f}, max {max(t[True]):8.3f}); on - off = {m1 - m0:+.3f} ms = {100 * (m1 - m0) / m0:+.2f} %; "
            f"frame_attention {tuple(fa.shape)}")


def errors(say):
    g = dict(np.load(os.path.join(ROOT, "tests", "golden", PIN + ".npz")))
    cfg = synth.preset("7b_l2", vaq=False, qav=False, vocab_size=32000, max_seq_len=128, batch_size=4, peaked_perm=True)
    batch = {"video": torch.from_numpy(g["video"]), "text_id": {"vqa": torch.from_numpy(g["text_id_vqa"])},
             "label": {"vqa": torch.from_numpy(g["label_vqa"])}, "video_start": {"vqa": g["vstart_vqa"].tolist()},
             "prefix_index": {"vqa": g["prefix_vqa"].tolist()}}
    say(f"errors against {PIN} (reference-generated; gaps {np.array2string(g['gap'], precision=5)}):")
    for dtype in (torch.float32, torch.bfloat16, torch.float16):
        model = make_model(cfg, dtype)
        eng = model.ensure_engine()
        for r in ("dense", "shared"):
            out = score.score_options(eng, batch, route=r)
            mean = out["mean"].cpu().numpy()
            e_mean = float((np.abs(mean - g["mean"]) / np.abs(g["mean"])).max())
            il = out["individual_losses"].cpu().numpy()
            e_il = float(np.abs(il - g["individual_losses"]).max() / np.abs(g["individual_losses"]).max())
            pred = out["prediction"].cpu().numpy()
            say(f"  {str(dtype):15s} {r:6s}: per-option mean, largest relative error {e_mean:.4e}; individual_losses / max "
                f"{e_il:.4e}; prediction {pred.tolist()} (fixture {g['prediction'].tolist()})")
        del model, eng
        torch.cuda.empty_cache()


def vocab_members(n: int, seed: int = 5):
    """n distinct answers of one to four tokens over a pool of 64 tokens: shared prefixes, members that are prefixes of others."""
    rng = np.random.default_rng(seed)
    pool = rng.choice(np.arange(1000, 30000), 64, replace=False)
    out, seen = [], set()
    while len(out) < n:
        m = tuple(int(t) for t in rng.choice(pool, int(rng.integers(1, 5))))
        if m not in seen:
            seen.add(m)
            out.append(list(m))
    return out


def vocab_timing(a, say):
    """score_vocab's tree route, its dense route and generate(constraints=..., num_beams=8) on one vocabulary of --vocab members,
    interleaved, --reps triples after --warmup calls of each; then one tree call with every projection and every tree attention
    between device events: the attention's time per layer beside the layer's four projections."""
    from fvqa import generate, vocab
    cfg = synth.preset("7b", vaq=False, qav=False, batch_size=a.batch_size, n_layers=a.n_layers, adapter_layer=a.n_layers)
    eng = make_model(cfg, torch.bfloat16).ensure_engine()
    opt = synth.make_option_batch(cfg, n_options=1, seed=1)
    prefix = [int(p) for p in opt["prefix_index"]["vqa"]]
    ids = opt["text_id"]["vqa"][:, 0:1].clone()
    for b, p in enumerate(prefix):
        ids[b, 0, p:] = 0
    batch = {"video": opt["video"], "text_id": {"vqa": ids}, "label": {"vqa": opt["label"]["vqa"][:, 0:1]},
             "video_start": opt["video_start"], "prefix_index": {"vqa": prefix}}
    members = vocab_members(a.vocab)
    plan = vocab.plan_vocab(vocab.constrain.compile_constraints(members, 2, cfg.vocab_size), a.batch_size, prefix, cfg.max_seq_len)
    B, S, R = a.batch_size, cfg.max_seq_len, plan.R
    say(f"vocabulary: {a.vocab} members of 1..4 tokens, {R} rows (internal nodes) and {int(plan.n_edges[0])} edges per sample; "
        f"7B width, {a.n_layers} layers, bf16, B={B}, S={S}")
    say(f"rows through the layers: tree {B * S + B * R} (prompt {B * S} + tree {B * R}), dense {B * a.vocab * S}, "
        f"beam of 8: {B * S} + up to 5 token steps of {8 * B} rows")
    arms = {"tree": lambda ev=None: vocab.score_vocab(eng, batch, members, route="tree", events=ev),
            "dense": lambda ev=None: vocab.score_vocab(eng, batch, members, route="dense", events=ev),
            "beam8": lambda ev=None: generate.generate(eng, batch, temperature=0.0, constraints=members, num_beams=8,
                                                       length_penalty=1.0, max_new_tokens=8)}
    for k in arms:
        for _ in range(a.warmup):
            arms[k]()
    torch.cuda.synchronize()
    rt, rd, rb = arms["tree"](), arms["dense"](), arms["beam8"]()
    d = float((rt["mean"] - rd["mean"]).abs().max() / rd["mean"][rd["count"] > 0].abs().max())
    say(f"outputs: mean, tree vs dense, largest difference over the largest |mean| {d:.3e}; predictions equal on "
        f"{int((rt['prediction'] == rd['prediction']).sum())} of {B}; the beam's choice equals the tree's prediction on "
        f"{int((rb['choice'].to(rt['prediction'].device) == rt['prediction']).sum())} of {B} (the beam is approximate: 8 slots)")
    total, parts = {k: [] for k in arms}, {}
    for _ in range(a.reps):
        for k in arms:
            ev = []
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            arms[k](ev)
            e1.record()
            e1.synchronize()
            total[k].append(e0.elapsed_time(e1))
            for x in ev:
                parts.setdefault((k, x[0]), []).append(ms(x))
    med = {k: statistics.median(v) for k, v in total.items()}
    for k, v in total.items():
        say(f"{k:6s}: median {med[k]:10.3f} ms  min {min(v):10.3f}  max {max(v):10.3f}  ({a.reps} reps, interleaved)")
    for (k, name), v in parts.items():
        say(f"  {k} route, {name}: median {statistics.median(v):10.3f} ms")
    say(f"  dense / tree = {med['dense'] / med['tree']:.2f}x, beam8 / tree = {med['beam8'] / med['tree']:.2f}x")
    # one tree call, each projection and each tree attention between events
    seen = {"attn": [], "gemm": []}
    real = {"attn": ops.attn_suffix_tree, "gemm": ops.gemm_nt}

    def spy(kind):
        def f(*args, **kw):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = real[kind](*args, **kw)
            e1.record()
            seen[kind].append((args[0].shape[0], e0, e1))
            return out
        return f
    ops.attn_suffix_tree, ops.gemm_nt = spy("attn"), spy("gemm")
    try:
        arms["tree"]()
        torch.cuda.synchronize()
    finally:
        ops.attn_suffix_tree, ops.gemm_nt = real["attn"], real["gemm"]
    t_attn = sum(e0.elapsed_time(e1) for _, e0, e1 in seen["attn"])
    t_proj = sum(e0.elapsed_time(e1) for rows, e0, e1 in seen["gemm"] if rows == B * R)
    n_proj = sum(1 for rows, _, _ in seen["gemm"] if rows == B * R)
    say(f"  tree pass per layer ({B * R} rows): fvqa_attn_suffix_tree {t_attn / a.n_layers:8.3f} ms, the layer's projections "
        f"(QKV, WO, W1|W3, W2: {n_proj} launches in all) {t_proj / a.n_layers:8.3f} ms")


def vocab_errors(say):
    """The figures tests/vocab_util.py's DENSE_MEAN_ERR is set from: the PARENT's dense teacher-forced pass (score_options'
    dense route on the members written out as options) against the reference-generated vocab fixtures, and both routes of
    score_vocab by the same figure (tests/test_vocab_gpu.py scale_err)."""
    sys.path.insert(0, ROOT)
    from fvqa import vocab
    from tests import vocab_util as VU
    from tests.test_vocab_gpu import scale_err
    for name in VU.FIXTURES:
        g = VU.load(name)
        cols = VU.first_columns(g)
        cfg = synth.preset(VU.MODEL_OF[name].replace("_peakedperm", ""), vaq=False, qav=False, vocab_size=32000, max_seq_len=128,
                           batch_size=4, peaked_perm=True)
        say(f"errors against {name} (reference-generated; gaps {np.array2string(g['gap'], precision=4)}):")
        for dtype in (torch.float32, torch.bfloat16, torch.float16):
            eng = make_model(cfg, dtype).ensure_engine()
            r = score.score_options(eng, VU.option_batch(g), route="dense")
            e = scale_err(-r["sum"].cpu().numpy() / np.maximum(g["count"], 1), g["mean"], cols)
            say(f"  {str(dtype):15s} parent's dense pass: mean {e:.4e}")
            for route in vocab.ROUTES:
                o = vocab.score_vocab(eng, VU.fixture_batch(g), VU.fixture_sets(g), route=route)
                say(f"  {str(dtype):15s} score_vocab {route:5s}: mean {scale_err(o['mean'].cpu().numpy(), g['mean'], cols):.4e} sum "
                    f"{scale_err(o['logprob_sum'].cpu().numpy(), g['logprob_sum'], cols):.4e}; prediction "
                    f"{o['prediction'].tolist()} (fixture {g['prediction'].tolist()})")
            del eng
            torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vocab", type=int, default=0, metavar="N_MEMBERS",
                    help="measure score_vocab (tree route, dense route) and generate(constraints=..., num_beams=8) on one vocabulary of "
                         "N members, interleaved, and nothing else (--log defaults to profiles/score_vocab.log)")
    ap.add_argument("--vocab_errors", action="store_true",
                    help="the parent's dense pass and both routes of score_vocab against the vocab fixtures (profiles/score_vocab.log)")
    ap.add_argument("--batch_size", type=int, default=8)
    ap.add_argument("--n_options", type=int, default=5)
    ap.add_argument("--n_layers", type=int, default=32)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--errors", action="store_true", help="also measure both routes' errors against the 7B-width fixture")
    ap.add_argument("--no_timing", action="store_true")
    ap.add_argument("--frame_attention", action="store_true",
                    help="measure score_options(frame_attention=True) against the call without it, interleaved, on both routes, and "
                         "nothing else (--log defaults to profiles/score_frame_attention.log)")
    ap.add_argument("--log", default=None)
    a = ap.parse_args()
    if a.log is None and (a.vocab or a.vocab_errors):
        a.log = os.path.join(ROOT, "profiles", "score_vocab.log")
    if a.log is None:
        a.log = os.path.join(ROOT, "profiles", "score_frame_attention.log" if a.frame_attention else "score_options.log")
    if not torch.cuda.is_available():
        sys.exit("score_bench.py measures on the GPU: no device found")
    os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
    log = open(a.log, "a")

    def say(s):
        print(s, flush=True)
        log.write(s + "\n")
        log.flush()

    say(f"# tools/score_bench.py on {torch.cuda.get_device_name(0)}, kernel sources {build.source_hash()[:12]}")
    with torch.no_grad():
        if a.frame_attention:
            frame_attention_cost(a, say)
            return
        if a.vocab or a.vocab_errors:
            if a.vocab_errors:
                vocab_errors(say)
            if a.vocab:
                vocab_timing(a, say)
            return
        if a.errors:
            errors(say)
        if not a.no_timing:
            timing(a, say)


if __name__ == "__main__":
    main()
