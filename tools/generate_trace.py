#!/usr/bin/env python3
"""What every mode of the generation and option-scoring API launches and returns, as one line per mode that two trees can be
diffed by: the tests' tiny fixture (tiny_peakedperm on rows 0 and 3 of its golden batch: B = 2, S = 128; fp32 and bf16) and, for
score_flipped, the first three samples of the flipped_tiny fixture (S = 192: the batch that takes the shared form), and per mode

  mode | ops calls | sha256 over the sequence of ops.* calls | torch operator dispatches | sha256 of every tensor in the result

An ops.* call enters the hash with its entry name, every tensor operand's shape, dtype and strides (no pointers) and every scalar
argument (keywords by name). The torch dispatches are counted as tests/test_generate_gpu.py counts them (TorchDispatchMode). The
same kernels on the same inputs in the same order give the same line: there is no tolerance. The tool uses the public API only
(fvqa.generate, fvqa.score, fvqa.vocab, the model's score_flipped and the fixtures of tests/), so it runs unchanged in any tree that has it. One thing of the engine's own
is taken out of the picture: it keeps a layer plan per arena under a key of device ADDRESSES (StepEngine.layer_plan), and every
evaluation call makes its video_start tensor anew, so whether a prefill finds the plan or builds it again hangs on where the
allocator put eight bytes. The tool drops the kept plans in front of every forward of a recorded call (a call may hold several:
the twin's pass, one prompt pass per task): each prefill then builds its plan, and no address decides what the trace holds.

  python tools/generate_trace.py [--out FILE] [--modes TEXT] [--rehearse] [--skip NAMES]
  (--modes: only the modes whose name holds TEXT; --rehearse: build the modes and their inputs, launch nothing; --skip: functions
  of fvqa.ops that stay unrecorded, for comparing against a tree that does not have them)"""
import argparse
import hashlib
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "flipped-vqa_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)
os.environ.setdefault("FVQA_SYNTHETIC_TOKENIZER", "1")
import torch  # noqa: E402
from torch.utils._python_dispatch import TorchDispatchMode  # noqa: E402

from fvqa import generate, ops, score, vocab  # noqa: E402

PRESET = "tiny_peakedperm"


def describe(x):
    """An operand as the hash sees it: no addresses, no values of tensors."""
    if torch.is_tensor(x):
        return ("tensor", tuple(x.shape), str(x.dtype), tuple(x.stride()))
    if x is None or isinstance(x, (bool, int, float, str, torch.dtype)):
        return repr(x)
    if isinstance(x, (list, tuple)):
        return tuple(describe(v) for v in x)
    if isinstance(x, dict):
        return tuple((k, describe(x[k])) for k in sorted(x))
    if hasattr(x, "__dict__"):                              # a TokenTrie on the device: its arrays
        return (type(x).__name__,) + tuple((k, describe(v)) for k, v in sorted(vars(x).items()) if torch.is_tensor(v))
    return type(x).__name__


class Trace:
    """Every callable of fvqa.ops replaced by a recording wrapper while a mode runs (the library's entries are looked up on the
    module at call time), torch's dispatches counted."""

    def __init__(self, skip=()):
        self.calls, self.sha, self.torch, self.skip = 0, hashlib.sha256(), 0, set(skip)

    def run(self, fn):
        trace = self

        class Count(TorchDispatchMode):
            def __torch_dispatch__(self, func, types_, args=(), kwargs=None):
                trace.torch += 1
                return func(*args, **(kwargs or {}))

        def recorded(name, real):
            def call(*a, **k):
                trace.calls += 1
                trace.sha.update(repr((name, describe(a), describe(k))).encode())
                return real(*a, **k)
            return call

        saved = {n: f for n, f in vars(ops).items() if n not in self.skip
                 and callable(f) and getattr(f, "__module__", None) == ops.__name__ and not isinstance(f, type)}
        for n, f in saved.items():
            setattr(ops, n, recorded(n, f))
        try:
            with Count():
                out = fn()
            torch.cuda.synchronize()
        finally:
            for n, f in saved.items():
                setattr(ops, n, f)
        return out


def forget_plans(eng) -> None:
    for arenas in ("_gen_arena", "_score_arena"):
        for ar in (getattr(eng, arenas, None) or {}).values():
            vars(ar).pop("_plan_key", None)


def forgetful(eng) -> None:
    """From here on every forward of this engine finds no kept plan."""
    real = eng.forward

    def forward(*a, **k):
        forget_plans(eng)
        return real(*a, **k)
    eng.forward = forward


def result_hash(out) -> str:
    """sha256 over every tensor of a result (nested dicts by key; numbers and names as they print)."""
    sha = hashlib.sha256()

    def walk(key, v):
        if torch.is_tensor(v):
            t = v.detach().cpu().contiguous()
            sha.update(repr((key, tuple(t.shape), str(t.dtype))).encode())
            sha.update(t.view(torch.uint8).numpy().tobytes() if t.numel() else b"")
        elif isinstance(v, dict):
            for k in sorted(v):
                walk(f"{key}.{k}", v[k])
        elif isinstance(v, (bool, int, float, str)):
            sha.update(repr((key, v)).encode())
    walk("", out if isinstance(out, dict) else {"result": out})
    return sha.hexdigest()


def modes(eng, batch, full, drafts):
    """-> [(name, callable)]. The member sets are those of tests/test_jump_gpu.py, tests/vocab_util.py (46 rows that cross a tile
    edge, 33 rows) and tests/test_treedraft_gpu.py (each sample's greedy answer among four decoys; a set the answer leaves at its
    first token: the narrow passes): they fit behind the 40 / 41-token prompts."""
    from tests import vocab_util as VU
    from tests.test_jump_gpu import sets_of
    from tests.test_treedraft_gpu import answers_of, decoys
    fx = types.SimpleNamespace(eng=eng, batch=batch, prefix=batch["prefix_index"]["vqa"])
    branchy, _ = sets_of(fx, "branchy")
    long_, _ = sets_of(fx, "long")
    g = lambda **kw: (lambda: generate.generate(eng, batch, **kw))  # noqa: E731
    so = lambda **kw: (lambda: {k: v for k, v in score.score_options(eng, full, **kw).items() if k != "plan"})  # noqa: E731
    members = [VU.crossing_members(), VU.random_members(33, 3, max_depth=12)]
    sv = lambda route: (lambda: {k: v for k, v in vocab.score_vocab(eng, batch, members, route=route).items() if k != "plan"})  # noqa: E731
    greedy = {}

    def drafted(kind, **kw):                                # draft sets around the greedy answers, which the unrecorded run finds
        def run():
            if "a" not in greedy:
                greedy["a"] = answers_of(generate.generate(eng, batch, temperature=0.0, stop_at_eos=True, max_new_tokens=31))
            ans = greedy["a"]
            sets = ([[a] + decoys(a, max(2, len(a) // 2)) for a in ans] if kind == "answer" else
                    decoys(ans[0], max(2, len(ans[0]) // 2))[:1] + [[9, 9, 9]])
            return generate.generate(eng, batch, max_new_tokens=31, draft_answers=sets, **kw)
        return run
    return [
        ("greedy_decode", lambda: generate.greedy_decode(eng, batch)),
        ("generate", g()),
        ("stop_at_eos=False", g(stop_at_eos=False)),
        ("temperature=0.8 top_p=0.9 seed=0", g(temperature=0.8, top_p=0.9, seed=0)),
        ("top_k=5 repetition_penalty=1.2 return_logprobs", g(top_k=5, repetition_penalty=1.2, return_logprobs=True)),
        ("num_return_sequences=3 sampled", g(temperature=0.8, seed=0, num_return_sequences=3)),
        ("constraints greedy", g(constraints=branchy)),
        ("constraints sampled", g(constraints=branchy, temperature=0.8, seed=0)),
        ("contrast=blind", g(contrast="blind")),
        ("contrast + constraints", g(contrast="blind", constraints=branchy)),
        ("contrast + num_return_sequences=2", g(contrast="blind", temperature=0.8, seed=0, num_return_sequences=2)),
        ("num_beams=3 length_penalty=0", g(num_beams=3, length_penalty=0.0)),
        ("num_beams=3 length_penalty=1", g(num_beams=3, length_penalty=1.0)),
        ("num_beams=3 + constraints", g(num_beams=3, constraints=branchy)),
        ("lookahead=4 prompt lookup", g(lookahead=4)),
        ("lookahead=4 draft_tokens return_logprobs", lambda: generate.generate(eng, batch, lookahead=4, draft_tokens=drafts(),
                                                                               return_logprobs=True)),
        ("jump_forward=4", g(constraints=branchy, jump_forward=4)),
        ("jump_forward=4 return_logprobs", g(constraints=branchy, jump_forward=4, return_logprobs=True)),
        ("jump_forward=16", g(constraints=long_, jump_forward=16)),
        ("score_options shared", so(route="shared")),
        ("score_options shared frame_attention", so(route="shared", frame_attention=True)),
        ("score_options dense frame_attention", so(route="dense", frame_attention=True)),
        ("score_options contrast=blind", so(contrast="blind")),
        ("score_vocab tree", sv("tree")),
        ("score_vocab dense", sv("dense")),
        ("lookahead=4 draft_answers", drafted("answer", lookahead=4)),
        ("lookahead=64 draft_answers return_logprobs", drafted("answer", lookahead=64, return_logprobs=True)),
        ("lookahead=4 draft_answers without the answer", drafted("none", lookahead=4)),
        ("lookahead=4 draft_tokens sampled", lambda: generate.generate(eng, batch, lookahead=4, draft_tokens=drafts(),
                                                                       temperature=0.8, top_p=0.9, seed=0)),
        ("lookahead=4 draft_answers sampled", drafted("answer", lookahead=4, temperature=0.8, top_p=0.9, seed=0)),
    ] + ([                                                  # (a tree without the pick rules and the vote has none of these)
        ("no_repeat_ngram_size=2 min_new_tokens=4", g(no_repeat_ngram_size=2, min_new_tokens=4)),
        ("min_p=0.1 sampled", g(temperature=1.5, min_p=0.1, seed=0)),
        ("min_p + top_k + repetition_penalty + num_return_sequences=3", g(temperature=1.5, min_p=0.05, top_k=20, repetition_penalty=1.2,
                                                                           no_repeat_ngram_size=3, seed=0, num_return_sequences=3)),
        ("vote num_return_sequences=5", g(temperature=3.0, min_p=0.05, seed=0, num_return_sequences=5, vote=True)),
        ("vote + constraints", g(temperature=3.0, seed=0, num_return_sequences=5, vote=True, constraints=branchy)),
        ("vote + contrast", g(temperature=3.0, seed=0, num_return_sequences=4, vote=True, contrast="blind")),
    ] if hasattr(ops, "sample_vote") else [])


FLIPPED, FLIPPED_ROWS = "flipped_tiny", (0, 1, 2)
FLIPPED_TASKS = (("vqa", "vaq", "qav"), ("vqa",), ("vaq",), ("qav",))


def flipped_modes(model, batch):
    """score_flipped in both routes: all three tasks and each task alone."""
    f = lambda **kw: (lambda: {k: v for k, v in model.score_flipped(batch, **kw).items() if k != "plan"})  # noqa: E731
    return [(f"score_flipped {route} {'+'.join(tasks)}", f(route=route, tasks=tasks, answer=batch["answer"]))
            for route in ("shared", "dense") for tasks in FLIPPED_TASKS]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="", help="also write the lines to this file")
    ap.add_argument("--modes", default="", help="only the modes whose name holds this text")
    ap.add_argument("--rehearse", action="store_true", help="stop in front of the first device call")
    ap.add_argument("--skip", default="", help="names of fvqa.ops, comma-separated, that are not recorded: a body one tree puts "
                    "between an entry and its checks and the other tree does not have; what it calls is recorded as before")
    a = ap.parse_args()
    from tests import flipped_util as FU
    from tests.test_beam_gpu import ROWS, eos_batch
    batch, full = eos_batch(PRESET, ROWS), eos_batch(PRESET, ROWS)
    fbatch = FU.golden_batch(FU.load(FLIPPED), FLIPPED_ROWS)
    lines = []
    for dtype in (torch.float32, torch.bfloat16):
        eng = None
        if not a.rehearse:
            from tests.test_generate_gpu import model_of
            eng = model_of(PRESET, dtype).ensure_engine()
        else:
            eng = types.SimpleNamespace(V=32000, F=10)
        plan = score.plan_options(full["text_id"]["vqa"], full["label"]["vqa"], None, full["video_start"]["vqa"], eng.F)
        assert plan.shared, plan.why_dense                  # (the last mode asks for the shared route)
        answer = {}

        def drafts():                                       # the full-length greedy answer, offered as the draft
            if "t" not in answer:
                answer["t"] = generate.generate(eng, batch, stop_at_eos=False)["tokens"].to(torch.int32)
            return answer["t"]
        todo = [(name, fn, eng) for name, fn in modes(eng, batch, full, drafts)]
        fmodel = None
        if not a.rehearse:
            from tests.gpu_util import build_model
            fmodel = build_model(FU.fixture_cfg(FLIPPED), dtype)[0].eval()
        todo += [(name, fn, fmodel and fmodel.ensure_engine()) for name, fn in flipped_modes(fmodel, fbatch)]
        todo = [m for m in todo if a.modes in m[0]]
        if a.rehearse:
            print(f"{dtype}: {len(todo)} modes built, B = {len(batch['prefix_index']['vqa'])}, S = {batch['text_id']['vqa'].shape[2]}, "
                  f"prompts of {batch['prefix_index']['vqa']} tokens; score_flipped on {len(FLIPPED_ROWS)} samples of {FLIPPED}, "
                  f"S = {fbatch['text_id']['vqa'].shape[2]}; nothing launched")
            continue
        if any("lookahead" in m[0] for m in todo):
            drafts()
        for e in {id(m[2]): m[2] for m in todo}.values():
            forgetful(e)
        for name, fn, _ in todo:
            fn()                                            # once unrecorded: caches of the engine's own (arenas, beam cache) exist
            tr = Trace(filter(None, a.skip.split(",")))
            out = tr.run(fn)
            lines.append(f"{str(dtype)[6:]:9s}| {name:46s}| ops calls {tr.calls:5d} {tr.sha.hexdigest()[:16]} | torch dispatches "
                         f"{tr.torch:5d} | result {result_hash(out)[:16]}")
            print(lines[-1], flush=True)
    if a.out and lines:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
