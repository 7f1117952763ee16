"""Contrastive decoding against a twin prompt, without a GPU: the rule of include/fvqa.h (fvqa_decode_next_pair) restated in fp64
numpy — `contrast_pick`, built on `penalised` / `kept_set_ex` of tests/test_sampling_cpu.py through tests/test_constrained_cpu.py's
`pick_trie`, and the yardstick of tests/test_contrast_gpu.py — and checked on planted rows; the C entry exported by both builds at
ABI 18 and refusing bad operands before any launch; `generate`'s keyword, the scoring combination and the flags."""
import ctypes as C
import os
import sys
import types

import numpy as np
import pytest
import torch

from fvqa import _lib, generate, ops, score
from tests.test_constrained_cpu import pick_trie
from tests.test_sampling_cpu import kept_set_ex, penalised  # noqa: F401  (what pick_trie is built on)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A = C.c_void_p(256)
BUILDS = [("bf16", _lib.BF16), ("f16", _lib.F16)]
EOS = 2


# ------------------------------------------------------------------------------------------------ the rule in fp64
def log_softmax64(row):
    x = np.asarray(row, dtype=np.float64)
    m = x.max()
    return x - (m + np.log(np.exp(x - m).sum()))


def contrast_parts(lp_row, ln_row, allowed, alpha, beta):
    """-> (c over the whole row, P = the plausible tokens ascending, the smallest distance of an allowed token to the
    plausibility bound). lp_row / ln_row: the raw logits of the positive / negative row; allowed: ascending tokens, None = all.
    lp = l - logsumexp(l) over the whole raw row; P = {i allowed: l+_i - max_allowed l+ >= logf(beta)};
    c_i = l+_i + alpha * (lp+_i - lp-_i)."""
    lpos = np.asarray(lp_row, dtype=np.float64)
    allowed = np.arange(lpos.size) if allowed is None else np.asarray(allowed, dtype=np.int64)
    c = lpos + alpha * (log_softmax64(lp_row) - log_softmax64(ln_row))
    rel = lpos[allowed] - lpos[allowed].max()
    bound = float(np.log(np.float32(beta))) if beta > 0 else -np.inf        # logf(beta), as the rule states it
    dist = float(np.abs(rel - bound).min()) if beta > 0 else np.inf
    return c, allowed[rel >= bound], dist


def contrast_pick(lp_row, ln_row, allowed, R, r, T, top_k, top_p, alpha, beta, u):
    """The token step of a pair in fp64 -> (token, n_kept, n_plausible): everything downstream of the contrast — the penalty
    (on c), the greedy pick with the lowest index on ties, e, Z, top-k against |P|, the nucleus cut, the walk — is
    tests/test_constrained_cpu.py::pick_trie on the row c with P as the allowed tokens."""
    c, P, _ = contrast_parts(lp_row, ln_row, allowed, alpha, beta)
    tok, kept = pick_trie(c, P, R, r, T, top_k, top_p, u)
    return tok, kept, int(P.size)


def test_neutral_parameters_are_the_plain_rule():
    rng = np.random.default_rng(3)
    for V in (64, 509):
        lp = (3.0 * rng.standard_normal(V)).astype(np.float32)
        ln = (3.0 * rng.standard_normal(V)).astype(np.float32)
        c, P, _ = contrast_parts(lp, ln, None, 0.0, 0.0)
        assert np.array_equal(c, lp.astype(np.float64)) and np.array_equal(P, np.arange(V))     # c is l+ itself, P everything
        for T, top_k, top_p, u in ((0.0, 0, 1.0, 0.0), (0.8, 0, 0.9, 0.37), (1.0, 8, 1.0, 0.9), (0.7, 5, 0.8, 0.05)):
            R = [int(lp.argmax()), 5, 5]
            got = contrast_pick(lp, ln, None, R, 1.3, T, top_k, top_p, 0.0, 0.0, u)
            assert got == pick_trie(lp, np.arange(V), R, 1.3, T, top_k, top_p, u) + (V,)
        # identical twins: any alpha is the plain rule too
        assert contrast_pick(lp, lp, None, [], 1.0, 0.0, 0, 1.0, 2.0, 0.0, 0.0) == (int(lp.argmax()), 1, V)


def test_beta_one_keeps_the_maxima_only():
    lp = np.array([1.0, 4.0, 0.5, 4.0, 3.9999], dtype=np.float32)
    ln = np.array([0.0, 9.0, 0.0, 0.0, -9.0], dtype=np.float32)            # the contrast favours token 3 of the two maxima
    c, P, _ = contrast_parts(lp, ln, None, 1.0, 1.0)
    assert P.tolist() == [1, 3]
    assert contrast_pick(lp, ln, None, [], 1.0, 0.0, 0, 1.0, 1.0, 1.0, 0.0) == (3, 1, 2)
    assert contrast_pick(lp, ln, None, [], 1.0, 0.0, 0, 1.0, 0.0, 1.0, 0.0) == (1, 1, 2)      # alpha 0: the lowest index of the tie
    # sampling walks P alone, whatever u
    for u in (0.0, 0.5, 0.999999):
        assert contrast_pick(lp, ln, None, [], 1.0, 1.0, 0, 1.0, 1.0, 1.0, u)[0] in (1, 3)


def test_an_implausible_token_wins_without_the_bound_and_is_excluded_with_it():
    """Token 7 has a tiny lp+ and a far tinier lp-: the difference is huge, and at beta = 0 it wins the contrast — the failure
    the plausible set exists for. At beta = 0.1 it lies 16 below the maximum (log 0.1 = -2.3) and takes no part."""
    V = 32
    lp = np.zeros(V, dtype=np.float32)
    ln = np.zeros(V, dtype=np.float32)
    lp[3], lp[4] = 6.0, 5.0
    ln[3], ln[4] = 6.0, 2.0                                                 # 4 gains from the contrast, 3 does not
    lp[7], ln[7] = -10.0, -60.0
    assert contrast_pick(lp, ln, None, [], 1.0, 0.0, 0, 1.0, 1.0, 0.0, 0.0) == (7, 1, V)
    tok, kept, n_pl = contrast_pick(lp, ln, None, [], 1.0, 0.0, 0, 1.0, 1.0, 0.1, 0.0)
    assert (tok, kept, n_pl) == (4, 1, 2)                                   # P = {3, 4}: 5 + (lp+ - lp-) beats 6 + 0
    assert contrast_pick(lp, ln, None, [], 1.0, 0.0, 0, 1.0, 0.0, 0.1, 0.0) == (3, 1, 2)      # alpha 0: the plain arg-max
    # the sampled walk never returns it either, and n_kept <= n_plausible
    for u in (0.0, 0.3, 0.9, 0.9999999):
        tok, kept, n_pl = contrast_pick(lp, ln, None, [], 1.0, 1.0, 0, 1.0, 1.0, 0.1, u)
        assert tok in (3, 4) and kept <= n_pl == 2


def test_inside_a_trie_node_the_maximum_and_the_set_are_taken_over_the_allowed_tokens():
    lp = np.array([9.0, 2.0, 1.0, -1.5, -4.0, 8.0], dtype=np.float32)      # 0 and 5, the largest, are not allowed
    ln = np.array([9.0, 2.0, -3.0, -9.0, -4.0, 8.0], dtype=np.float32)
    al = [1, 2, 3, 4]
    c, P, dist = contrast_parts(lp, ln, al, 1.0, 0.1)
    assert P.tolist() == [1, 2] and dist > 0.1                              # within log(0.1) = -2.30 of the ALLOWED maximum 2.0
    assert contrast_parts(lp, ln, None, 1.0, 0.1)[1].tolist() == [0, 5]     # over the whole row the set is another one
    assert contrast_pick(lp, ln, al, [], 1.0, 0.0, 0, 1.0, 1.0, 0.1, 0.0) == (2, 1, 2)        # 1 + 4 beats 2 + 0 (up to one lse)
    assert contrast_pick(lp, ln, al, [], 1.0, 0.0, 0, 1.0, 1.0, 0.0, 0.0) == (3, 1, 4)        # beta 0: -1.5 + 7.5 wins
    assert contrast_pick(lp, ln, al, [], 1.0, 1.0, 1, 1.0, 1.0, 0.1, 0.7) == (2, 1, 2)        # top-k cuts inside P
    # the penalty applies to c: 2's c = 1 + 4 + d, d = lse- - lse+ (about -0.0); divided by 3 it falls behind 1's c = 2 + d
    assert contrast_pick(lp, ln, al, [2], 3.0, 0.0, 0, 1.0, 1.0, 0.1, 0.0)[0] == 1


# ------------------------------------------------------------------------------------------------ the C entry
def _args(dt, temperature=0.7, alpha=1.0, beta=0.1, n_seq=3, trie=True):
    t = A if trie else None
    #      logits u emb T          top_p top_k r   alpha  beta eos stop ids pos done gen x tok kept npl lp act cnt pos64
    return [A, A, A, temperature, 0.9, 8, 1.2, alpha, beta, 2, 1, A, A, A, A, A, A, A, A, A, A, A, A,
            t, t, t, t, 4, 3, n_seq, 509, 128, 16, dt, None]              # node nf et ec n_nodes n_edges B V D S dtype stream


@pytest.mark.parametrize("which,h16", BUILDS)
def test_the_pair_entry_is_exported_and_checks_its_operands_on_the_host(which, h16):
    """Every call here must be refused: one that passed validation would launch a kernel on fake addresses."""
    lib = _lib.load(which)
    assert lib.fvqa_version() == _lib.ABI_VERSION == 18          # an added entry changes no signature
    fn = lib.fvqa_decode_next_pair
    assert len(_args(h16)) == len(_lib.SIGNATURES["fvqa_decode_next_pair"][1])
    assert callable(ops.decode_next_pair)                         # declared = bound = exported
    for dt in (h16, _lib.F32):
        for trie in (True, False):
            base = _args(dt, trie=trie)
            for at in (0, 1, 2, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21):     # every required pointer; u when sampling
                a = list(base)
                a[at] = None
                assert fn(*a) == -1, at
            for alpha in (-0.5, -1e-9, float("nan")):
                assert fn(*_args(dt, alpha=alpha, trie=trie)) == -1, alpha
                assert fn(*_args(dt, temperature=0.0, alpha=alpha, trie=trie)) == -1, alpha     # in greedy mode too
            for beta in (-0.1, 1.0001, 2.0, float("nan")):
                assert fn(*_args(dt, beta=beta, trie=trie)) == -1, beta
            for n_seq, want in ((32768, -2), (65535, -2), (0, -2), (-3, -2)):   # 2 * n_seq rows: the ticket counts in 16 bits
                assert fn(*_args(dt, n_seq=n_seq, trie=trie)) == want, n_seq
            for at in (30, 31, 32):                                  # V, D, S <= 0
                a = list(base)
                a[at] = 0
                assert fn(*a) == -2, at
            for at in (0, 14, 18, 19, 21):                           # logits, gen_start, n_plausible, logprob, counter off 4 bytes
                a = list(base)
                a[at] = C.c_void_p(258)
                assert fn(*a) == -3, at
            # the checks of the entry it extends still hold
            for at, bad in ((3, -0.5), (4, 0.0), (5, -1), (6, 0.9)):
                a = list(base)
                a[at] = bad
                assert fn(*a) == -1, (at, bad)
        base = _args(dt)
        for at in (23, 24, 25, 26):                                  # a trie given in part; off its boundary
            a = list(base)
            a[at] = None
            assert fn(*a) == -1, at
            a[at] = C.c_void_p(258)
            assert fn(*a) == -3, at
        a = list(base)
        a[27] = 0                                                    # n_nodes <= 0 with a trie
        assert fn(*a) == -2
    other = _lib.F16 if h16 == _lib.BF16 else _lib.BF16
    assert fn(*_args(other)) == -1 and fn(*_args(7, trie=False)) == -1     # the other build's 16-bit code; no code at all


# ------------------------------------------------------------------------------------------------ generate
def _data(B=2, S=16, audio=False, feats=(10, 768)):
    d = {"text_id": {"vqa": torch.zeros(B, 1, S, dtype=torch.int64)}, "prefix_index": {"vqa": [min(10, S - 1)] * B},
         "video": torch.ones(B, *feats)}
    if audio:
        d["audio"] = torch.ones(B, 10, 1024)
    return d


def test_generate_refuses_what_contrast_cannot_serve():
    """All refused before the engine is touched (there is none here)."""
    eng = types.SimpleNamespace(model=None, pack=None, device="cpu", V=509)
    ok_twin = {"video": torch.zeros(2, 10, 768)}
    for kw, match in ((dict(contrast="blind", contrast_alpha=-0.1), "contrast_alpha"),
                      (dict(contrast="blind", contrast_alpha=float("nan")), "contrast_alpha"),
                      (dict(contrast="blind", contrast_beta=-0.01), "contrast_beta"),
                      (dict(contrast="blind", contrast_beta=1.5), "contrast_beta"),
                      (dict(contrast="blind", contrast_beta=float("nan")), "contrast_beta"),
                      (dict(contrast=ok_twin, num_beams=2), "num_beams"),
                      (dict(contrast="blind", num_beams=3), "num_beams"),
                      (dict(contrast={"audio": torch.zeros(2, 10, 1024)}), "no such features"),      # a key the batch lacks
                      (dict(contrast={"video": torch.zeros(2, 10, 768), "text": torch.zeros(2)}), "no such features"),
                      (dict(contrast={"video": torch.zeros(2, 9, 768)}), "shape"),
                      (dict(contrast={"video": torch.zeros(1, 10, 768)}), "shape"),
                      (dict(contrast={"video": [[0.0]]}), "shape"),
                      (dict(contrast="deaf"), "blind"),
                      (dict(contrast={}), "blind")):
        with pytest.raises(ValueError, match=match):
            generate.generate(eng, _data(), **kw)
    with pytest.raises(ValueError, match="video"):
        generate.generate(eng, {"prefix_index": {"vqa": [3]}}, contrast="blind")          # a batch with no features at all
    # two rows per sample: 2 * B * n <= 65535
    with pytest.raises(ValueError, match="two rows"):
        generate.generate(eng, _data(B=32768, S=4, feats=(1, 2)), contrast="blind")
    with pytest.raises(ValueError, match="two rows"):
        generate.generate(eng, _data(B=8192, S=4, feats=(1, 2)), contrast="blind", temperature=0.8, num_return_sequences=4)
    # what can be served passes these checks and goes on to the prefill's first read of the batch
    for kw in (dict(contrast="blind"), dict(contrast=ok_twin, contrast_alpha=0.0, contrast_beta=1.0),
               dict(contrast="blind", contrast_beta=0.0, temperature=0.8, num_return_sequences=3)):
        with pytest.raises(KeyError, match="label"):
            generate.generate(eng, _data(), **kw)
    with pytest.raises(KeyError, match="label"):
        generate.generate(eng, _data(audio=True), contrast={"audio": torch.zeros(2, 10, 1024)})
    tw = generate._twin(_data(audio=True), "blind", 1.0, 0.1)
    assert set(tw) == {"video", "audio"} and all(not bool(v.any()) for v in tw.values())
    assert tuple(tw["audio"].shape) == (2, 10, 1024)


def test_without_the_keyword_nothing_changes(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("contrast=None went to the pair path")
    monkeypatch.setattr(generate, "_twin", boom)
    monkeypatch.setattr(ops, "decode_next_pair", boom)
    eng = types.SimpleNamespace(model=None, pack=None, device="cpu")
    for kw in ({}, {"contrast": None}, {"temperature": 0.7, "contrast": None, "contrast_alpha": -5.0, "contrast_beta": 9.0}):
        with pytest.raises(ValueError, match="prefix_index"):    # the first thing the existing path asks for
            generate.generate(eng, {}, **kw)
    seen = {}
    monkeypatch.setattr(generate, "beam_search", lambda *a, **k: seen.update(k))
    generate.generate(eng, {}, num_beams=2)
    assert seen and not any(k.startswith("contrast") for k in seen)                 # beam search is called as it was
    # the scoring path: without the keyword the result has the keys it had
    called = []
    monkeypatch.setattr(score, "plan_options", lambda *a, **k: types.SimpleNamespace(shared=True, why_dense=""))
    monkeypatch.setattr(score, "_shared", lambda eng, data, *a: (called.append(data) or (0, 1, 2, 3, 4)))
    d = {"text_id": {"vqa": torch.zeros(1, 2, 8, dtype=torch.int64)}, "label": {"vqa": torch.zeros(1, 2, 8, dtype=torch.int64)},
         "video_start": {"vqa": [1]}}
    r = score.score_options(types.SimpleNamespace(V=9, F=2), d, route="shared")
    assert set(r) == {"individual_losses", "sum", "count", "mean", "prediction", "route", "plan"} and len(called) == 1


# ------------------------------------------------------------------------------------------------ scoring
def test_scoring_combination_on_hand_made_means():
    nan = float("nan")
    mp = torch.tensor([[1.0, 2.0, 3.0, 0.5],       # plain: option 3 — but it has no scored token
                       [2.0, 1.5, 1.5, 9.0],       # a tie of the plain means
                       [1.0, 1.2, 5.0, 5.0],
                       [nan, 4.0, 3.0, nan]])
    mn = torch.tensor([[1.0, 2.5, 3.0, 9.0],
                       [1.0, 1.0, 1.0, 9.0],       # ... and of the combination: 1.5 + (1.5 - 1.0) twice, under 2 + 1
                       [0.2, 1.4, 5.0, 5.0],       # 0: 1 + .8 = 1.8; 1: 1.2 - .2 = 1.0 -> the blind twin knew option 0 already
                       [nan, 1.0, 3.5, nan]])
    cnt = torch.tensor([[3, 3, 2, 0], [1, 2, 2, 4], [2, 2, 2, 2], [0, 5, 5, 0]])
    got = score.contrast_pick(mp, mn, cnt, 1.0)
    assert got.dtype == torch.int64 and got.tolist() == [0, 1, 1, 2]    # row 0: 1.0, 1.5, 3.0; row 3: 7.0 against 2.5
    assert score.contrast_pick(mp, mn, cnt, 0.0).tolist() == [0, 1, 0, 2]               # alpha 0: the plain argmin over count > 0
    assert score.contrast_pick(mp, mn, cnt, 4.0).tolist() == [1, 1, 1, 2]               # row 0: 1.0 against 2 - 2 = 0
    assert score.contrast_pick(mp, mn, torch.zeros_like(cnt), 1.0).tolist() == [0, 0, 0, 0]
    # a twin equal to the batch: the plain prediction whatever alpha
    assert score.contrast_pick(mp[:3], mp[:3], cnt[:3], 7.0).tolist() == [0, 1, 0]
    with pytest.raises(ValueError, match="contrast_alpha"):
        score.score_options(None, {"video": torch.zeros(1, 10, 768)}, contrast="blind", contrast_alpha=-1.0)
    with pytest.raises(ValueError, match="no such features"):
        score.score_options(None, {"video": torch.zeros(1, 10, 768)}, contrast={"audio": torch.zeros(1, 10, 1024)})


def test_score_options_scores_the_twin_by_the_same_route(monkeypatch):
    seen = []

    def fake(eng, data, ids_h, lab_h, vs_list, plan, events):
        seen.append(data)
        blind = not bool(data["video"].any())
        mean = torch.tensor([[3.0, 1.0, 2.0]]) if blind else torch.tensor([[1.0, 1.25, 5.0]])
        return "il-blind" if blind else "il", mean * 2, torch.tensor([[2, 2, 2]]), mean, mean.argmin(1)
    monkeypatch.setattr(score, "plan_options", lambda *a, **k: types.SimpleNamespace(shared=True, why_dense=""))
    monkeypatch.setattr(score, "_shared", fake)
    d = {"text_id": {"vqa": torch.zeros(1, 3, 8, dtype=torch.int64)}, "label": {"vqa": torch.zeros(1, 3, 8, dtype=torch.int64)},
         "video_start": {"vqa": [1]}, "video": torch.ones(1, 10, 768)}
    r = score.score_options(types.SimpleNamespace(V=9, F=2), d, route="shared", contrast="blind", contrast_alpha=1.0)
    assert len(seen) == 2 and seen[0] is d and seen[1]["text_id"] is d["text_id"] and bool(d["video"].all())
    assert r["individual_losses"] == "il" and r["mean"].tolist() == [[1.0, 1.25, 5.0]]   # the batch's own
    assert r["mean_blind"].tolist() == [[3.0, 1.0, 2.0]]
    assert r["prediction_plain"].tolist() == [0] and r["prediction_blind"].tolist() == [1]
    assert r["prediction"].tolist() == [0]                       # -1.0, 1.5, 8.0
    r = score.score_options(types.SimpleNamespace(V=9, F=2), d, route="shared", contrast={"video": d["video"] * 0},
                            contrast_alpha=0.0)
    assert r["prediction"].tolist() == r["prediction_plain"].tolist() == [0]


# ------------------------------------------------------------------------------------------------ the flags
def test_the_parsers_accept_the_flags_and_refuse_a_contrastive_beam_search():
    import train
    a = train.get_args_parser().parse_args([])
    assert a.contrast is None and a.contrast_alpha == 1.0 and a.contrast_beta == 0.1
    a = train.get_args_parser().parse_args(["--contrast", "blind", "--contrast_alpha", "0.5", "--contrast_beta", "0.2",
                                            "--gen_constrain", "options"])
    assert a.contrast == "blind" and a.contrast_alpha == 0.5 and a.contrast_beta == 0.2 and a.gen_constrain == "options"
    assert train.get_args_parser().parse_args(["--num_beams", "3"]).num_beams == 3          # without --contrast: as before
    for bad in (["--contrast", "blind", "--num_beams", "2"], ["--contrast", "deaf"], ["--contrast", "blind", "--contrast_alpha", "-1"],
                ["--contrast", "blind", "--contrast_beta", "1.5"]):
        with pytest.raises(SystemExit):
            train.get_args_parser().parse_args(bad)
    sys.path.insert(0, os.path.join(ROOT, "flipped-vqa_amd"))
    import answer
    base = ["--random_init", "--synthetic", "--question", "why"]
    assert answer.get_args_parser().parse_args(base).contrast is None
    a = answer.get_args_parser().parse_args(base + ["--contrast", "blind", "--contrast_alpha", "2", "--contrast_beta", "0"])
    assert a.contrast == "blind" and a.contrast_alpha == 2.0 and a.contrast_beta == 0.0
    with pytest.raises(SystemExit):
        answer.get_args_parser().parse_args(base + ["--contrast", "blind", "--num_beams", "4"])


def test_the_model_passes_the_flags_through(monkeypatch):
    from llama.model import Transformer
    m = types.SimpleNamespace(args=types.SimpleNamespace(contrast="blind", contrast_alpha=0.5, contrast_beta=0.2))
    assert Transformer._contrast_kw(m) == {"contrast": "blind", "contrast_alpha": 0.5, "contrast_beta": 0.2}
    assert Transformer._contrast_kw(types.SimpleNamespace(args=types.SimpleNamespace())) == {}
    seen = {}

    def fake(eng, data, **kw):
        seen.update(kw)
        return {"individual_losses": 1, "prediction": 2, "mean": 3, "count": 4, "route": "shared", "mean_blind": 5,
                "prediction_blind": 6, "prediction_plain": 7, "plan": None}
    monkeypatch.setattr(score, "score_options", fake)
    me = types.SimpleNamespace(ensure_engine=lambda: None)
    assert Transformer.score_options.__wrapped__(me, {}, contrast="blind", contrast_alpha=2.0) == 1
    assert seen == {"contrast": "blind", "contrast_alpha": 2.0}
    assert set(me.last_scoring) == {"prediction", "mean", "count", "route", "mean_blind", "prediction_blind", "prediction_plain"}
    seen.clear()
    Transformer.score_options.__wrapped__(me, {})
    assert seen == {}                                             # without the keyword score_options is called as it was
