#!/usr/bin/env python3
"""TEST INFRASTRUCTURE — generates tests/golden/audio_eval_tiny_concat_peakedperm.npz: the reference's generation path
(llama/model.py:367-546 `Transformer.inference`) in `concat` mode, made the way oracle/gen_golden_eval.py makes
eval_tiny_peakedperm — by that script itself (its `main`, unchanged: the reference's NExT-QA reader for the validation batch,
the permuted peaked LM head, the spies on ids / similarities / margins), with three things redirected:
  * the reference model is built with the audio arguments (tools/gen_golden_audio.py build_reference, audio = "concat");
  * the collated batch gets an "audio" field (closed form, fvqa.synth.hashed_uniform): (B, max_feats, 1024);
  * the result goes to its own file and carries the audio next to the frames.
"""
import dataclasses
import math
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "flipped-vqa_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from fvqa import synth  # noqa: E402
import oracle.gen_golden as G  # noqa: E402
import oracle.gen_golden_eval as E  # noqa: E402
import gen_golden_audio as A  # noqa: E402

MODE, NAME = "concat", "audio_eval_tiny_concat_peakedperm"


def eval_audio(B: int, F: int = 10):
    return synth.hashed_uniform("eval.audio", (B, F, 1024), math.sqrt(3.0))


def main():
    G.install_shims()                           # puts the reference first on sys.path
    sys.modules.setdefault("pysrt", types.ModuleType("pysrt"))
    import dataloader as D                      # the reference package
    collate = D.batch_collate

    def collate_with_audio(samples):
        b = collate(samples)
        b["audio"] = eval_audio(len(samples))
        return b

    D.batch_collate = collate_with_audio
    G.build_reference = lambda M, cfg: A.build_reference(M, dataclasses.replace(cfg, audio=MODE))
    path = os.path.join(ROOT, "tests", "golden", NAME + ".npz")

    class Numpy:                                # E's `np`, with the save going to this fixture's own file
        def __getattr__(self, k):
            return getattr(np, k)

        @staticmethod
        def savez_compressed(_, **out):
            out["audio"] = eval_audio(out["video"].shape[0]).numpy()
            np.savez_compressed(path, **out)

    E.np = Numpy()
    sys.argv = [sys.argv[0], "tiny", "peakedperm"]
    E.main()
    print("->", path, os.path.getsize(path) // 1024, "KiB")


if __name__ == "__main__":
    main()
