"""The generation API on the GPU: the token-step kernel alone (fvqa_decode_next, csrc/sample.hip) against numpy / the fp64
statement of its rule / the supports observed from the reference's own sampler, and `generate` end to end against
`greedy_decode` and the fixtures made from the reference's `Transformer.inference` (tools/gen_golden_generate.py)."""
import json
import os
import types

import numpy as np
import pytest
import torch

import engine
from fvqa import generate, ops, synth
from tests.test_eval import GOLDS, golden_batch
from tests.test_generate_cpu import kept_set

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
GEN_EOS = {p: dict(np.load(os.path.join(GOLDEN, f"gen_eos_{p}_peakedperm.npz"))) for p in ("tiny", "7b_l2")}
SUPPORT = dict(np.load(os.path.join(GOLDEN, "sampler_support.npz")))
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
EPS = 1e-4          # of a row's total mass: five times (7.5e-6: <= 125 sequential fp32 adds per thread) + (1e-5: __expf)
DEV = "cuda"


# ------------------------------------------------------------------------------------------------ the kernel alone
def step(logits, *, emb=None, u=None, ids=None, pos=None, done=None, S=16, D=128, dtype=torch.float32, **kw):
    """One launch on host arrays -> dict of host arrays (the in/out operands after the step included)."""
    logits = torch.as_tensor(np.asarray(logits, dtype=np.float32), device=DEV)
    B, V = logits.shape
    if emb is None:
        emb = torch.randn(V, D, generator=torch.Generator().manual_seed(1)).to(dtype).to(DEV)
    t = lambda a, dt: torch.as_tensor(np.asarray(a), dtype=dt, device=DEV).contiguous()   # noqa: E731
    ids = t(np.zeros((B, S)) if ids is None else ids, torch.int64)
    pos = t(np.full(B, 3) if pos is None else pos, torch.int32)
    done = t(np.zeros(B) if done is None else done, torch.int32)
    x = torch.full((B, emb.shape[1]), float("nan"), dtype=emb.dtype, device=DEV)
    tok, kept = torch.full((B,), -7, dtype=torch.int32, device=DEV), torch.full((B,), -7, dtype=torch.int32, device=DEV)
    act = torch.full((1,), -7, dtype=torch.int32, device=DEV)
    pos64 = torch.full((B,), -7, dtype=torch.int64, device=DEV)
    ops.decode_next(logits, emb, ids, pos, done, x, tok, kept, act, u=None if u is None else t(u, torch.float32), pos64=pos64,
                    **kw)
    torch.cuda.synchronize()
    return {"token": tok.cpu().numpy(), "n_kept": kept.cpu().numpy(), "n_active": int(act), "ids": ids.cpu().numpy(),
            "pos": pos.cpu().numpy(), "done": done.cpu().numpy(), "x": x.cpu(), "emb": emb.cpu(), "pos64": pos64.cpu().numpy()}


@pytest.mark.parametrize("V", [509, 32000])
def test_greedy_is_numpys_first_index_argmax(V):
    rng = np.random.default_rng(V)
    lg = rng.standard_normal((3, V)).astype(np.float32)
    r = step(lg)
    assert np.array_equal(r["token"], lg.argmax(1)) and np.array_equal(r["n_kept"], [1, 1, 1]) and r["n_active"] == 3
    tie = rng.standard_normal((3, V)).astype(np.float32)
    top = np.float32(tie.max() + 1)
    tie[0, 7] = tie[0, 300] = top                     # duplicated maximum: the lower index
    tie[1, 0] = top
    tie[2, V - 1] = top
    r = step(tie)
    assert r["token"].tolist() == [7, 0, V - 1]
    tie[0, 300] = np.nextafter(top, np.float32(np.inf))
    assert step(tie)["token"].tolist() == [300, 0, V - 1]


@pytest.mark.parametrize("dtype", DTYPES)
def test_next_embedding_is_the_tokens_row_bitwise(dtype):
    for V, D in ((509, 128), (509, 36)):              # (36 elements: rows that are no multiple of 16 bytes in 16-bit storage)
        lg = np.random.default_rng(5).standard_normal((3, V)).astype(np.float32)
        r = step(lg, D=D, dtype=dtype)
        assert r["x"].dtype == dtype
        assert torch.equal(r["x"].view(torch.uint8), r["emb"][torch.from_numpy(r["token"]).long()].view(torch.uint8))


def test_row_bookkeeping():
    V, S, EOS = 509, 16, 2
    lg = np.full((5, V), -1.0, dtype=np.float32)
    for b, t in enumerate([40, EOS, 77, 88, EOS]):
        lg[b, t] = 3.0
    ids0 = np.arange(5 * S).reshape(5, S) % 400 + 3
    pos0 = [3, 4, S - 1, 6, -1]                       # row 2 has no room; row 4 starts at position 0
    done0 = [0, 0, 0, 1, 0]
    r = step(lg, ids=ids0, pos=pos0, done=done0, S=S, eos_id=EOS, stop_at_eos=True)
    want = ids0.copy()
    want[0, 4], want[1, 5], want[4, 0] = 40, EOS, EOS
    assert np.array_equal(r["ids"], want)             # rows 2 (full) and 3 (done) untouched
    assert r["pos"].tolist() == [4, 5, S - 1, 6, 0] and r["pos64"].tolist() == [4, 5, S - 1, 6, 0]
    assert r["done"].tolist() == [0, 1, 1, 1, 1] and r["n_active"] == 1
    assert r["token"].tolist() == [40, EOS, -1, -1, EOS] and r["n_kept"].tolist() == [1, 1, 0, 0, 1]
    emb = r["emb"]
    assert torch.equal(r["x"][0], emb[40]) and torch.equal(r["x"][1], emb[EOS])
    assert torch.equal(r["x"][2], emb[int(ids0[2, S - 1])]) and torch.equal(r["x"][3], emb[int(ids0[3, 6])])   # valid rows
    r = step(lg, ids=ids0, pos=pos0, done=done0, S=S, eos_id=EOS, stop_at_eos=False)
    assert np.array_equal(r["ids"], want) and r["done"].tolist() == [0, 0, 1, 1, 0] and r["n_active"] == 3
    r = step(lg[:2], ids=ids0[:2], pos=[S - 1, S - 1], done=[0, 1], S=S)
    assert r["n_active"] == 0 and np.array_equal(r["ids"], ids0[:2])


def spread_u(n):
    u = ((np.arange(n) + 0.5) / n).astype(np.float32)
    u[0], u[-1] = 0.0, np.float32(1 - 2.0 ** -24)
    return u


@pytest.mark.parametrize("row", range(4))
def test_sampler_is_pinned_to_the_references_support(row):
    """64 copies of a fixture row under 64 spread uniforms (0 and 1 - 2^-24 among them): n_kept is the size of the support the
    reference's own sample_top_p showed over 50 000 draws, every returned token lies in it, every token of it is returned."""
    lg = SUPPORT["logits"][row]
    _, T, top_p = SUPPORT["params"][row]
    sup = SUPPORT["support"][row]
    sup = sup[sup >= 0]
    r = step(np.tile(lg, (64, 1)), u=spread_u(64), temperature=float(T), top_p=float(top_p))
    assert np.array_equal(r["n_kept"], np.full(64, sup.size)), (r["n_kept"], sup.size)
    assert set(r["token"].tolist()) == set(sup.tolist())


def fp64_counts(lg, T, top_p):
    return kept_set(lg, T, top_p)[0].size


@pytest.mark.parametrize("T,top_p", [(0.8, 0.95), (1.0, 0.5), (0.3, 0.9), (1.5, 0.99)])
@pytest.mark.parametrize("V,scale", [(32000, 6.0), (509, 3.0)])
def test_broad_rows_follow_the_rule_in_fp64(V, scale, T, top_p):
    rng = np.random.default_rng(V + int(100 * T))
    lg = (scale * rng.standard_normal((16, V))).astype(np.float32)
    u = rng.random(16).astype(np.float32)
    r = step(lg, u=u, temperature=T, top_p=top_p)
    for b in range(16):
        x = lg[b].astype(np.float64) / T
        p = np.exp(x - x.max())
        p /= p.sum()
        order = np.lexsort((np.arange(V), -p))
        front = np.cumsum(p[order]) - p[order]
        n = int(r["n_kept"][b])
        n_lo, n_hi = int((front <= top_p - EPS).sum()), int((front <= top_p + EPS).sum())
        print(f"V={V} T={T} top_p={top_p} row {b}: n_kept {n} in [{n_lo}, {n_hi}]")
        assert n_lo <= n <= n_hi, (b, n, n_lo, n_hi)
        kept = np.sort(order[:n])                      # the n_kept highest tokens, walked in index order
        tok = int(r["token"][b])
        assert tok in kept, (b, tok)
        cdf = np.cumsum(p[kept])
        M = cdf[-1]
        k = int(np.searchsorted(kept, tok))
        lo, hi = (cdf[k - 1] if k else 0.0) - EPS * M, cdf[k] + EPS * M
        assert lo <= float(u[b]) * M <= hi, (b, tok, lo, float(u[b]) * M, hi)


def test_edge_parameters():
    rng = np.random.default_rng(9)
    for V, scale in ((509, 3.0), (32000, 6.0)):
        lg = (scale * rng.standard_normal((16, V))).astype(np.float32)
        u = spread_u(16)
        r = step(lg, u=u, temperature=1.0, top_p=1e-6)
        assert np.array_equal(r["n_kept"], np.ones(16)) and np.array_equal(r["token"], lg.argmax(1))
        r = step(lg, u=u, temperature=1.0, top_p=1.0)
        for b in range(16):
            assert r["n_kept"][b] >= fp64_counts(lg[b], 1.0, 1.0 - EPS)
        r = step(lg, u=u, temperature=1e-3, top_p=0.9)
        assert ((0 <= r["token"]) & (r["token"] < V)).all() and (r["n_kept"] >= 1).all()
        assert torch.isfinite(r["x"].float()).all()
        a = step(lg, u=u, temperature=0.8, top_p=0.95)
        b2 = step(lg, u=u, temperature=0.8, top_p=0.95)
        for k in ("token", "n_kept", "ids", "pos", "done"):
            assert np.array_equal(a[k], b2[k]), k
        assert torch.equal(a["x"], b2["x"]) and a["n_active"] == b2["n_active"]
    with pytest.raises(ValueError):
        step(lg, temperature=0.8, top_p=0.95)          # sampling without uniforms


# ------------------------------------------------------------------------------------------------ end to end
_MODELS = {}


def model_of(pname, dtype):
    """One model per (preset, dtype) for the whole module; `pname` as in tests/test_eval.py (tiny, 7b_l2_peakedperm, ...)."""
    from tests.gpu_util import build_model
    key = (pname, dtype)
    if key not in _MODELS:
        perm = pname.endswith("_peakedperm")
        peaked = pname.endswith("_peaked")
        base = pname[:pname.rindex("_peaked")] if perm or peaked else pname
        cfg = synth.preset(base, vaq=False, qav=False, vocab_size=32000, max_seq_len=128, batch_size=4, peaked=peaked,
                           peaked_perm=perm)
        m, _ = build_model(cfg, dtype)
        _MODELS[key] = m.eval()
    m = _MODELS[key]
    m.args.gen_stop_eos = False
    return m


CASES = [("tiny_peakedperm", torch.float32), ("tiny_peakedperm", torch.bfloat16), ("tiny_peakedperm", torch.float16),
         ("7b_l2_peakedperm", torch.bfloat16)]


@pytest.mark.parametrize("pname,dtype", CASES)
def test_full_length_greedy_is_greedy_decode(pname, dtype):
    m = model_of(pname, dtype)
    eng = m.ensure_engine()
    G = GOLDS[pname]
    batch = golden_batch(G)
    ref = generate.greedy_decode(eng, batch)
    out = generate.generate(eng, batch, temperature=0.0, stop_at_eos=False, max_new_tokens=31)
    assert torch.equal(out["ids"], ref) and out["steps"] == 31
    assert np.array_equal(out["ids"].cpu().numpy(), G["ids_after"])          # (16-bit builds too: the peaked margins)
    assert out["n_generated"].tolist() == [31] * 4 and tuple(out["tokens"].shape) == (4, 31)
    for b, p in enumerate(G["prefix_vqa"]):
        assert np.array_equal(out["tokens"][b].cpu().numpy(), G["ids_after"][b, p:p + 31])


@pytest.mark.parametrize("pname,dtype", CASES)
def test_eos_stop(pname, dtype, tmp_path):
    m = model_of(pname, dtype)
    eng = m.ensure_engine()
    G = GEN_EOS[pname[:pname.rindex("_peaked")]]
    k, prefix = G["eos_k"], G["prefix_vqa"]
    batch = golden_batch(G)
    full = generate.generate(eng, batch, temperature=0.0, stop_at_eos=False, max_new_tokens=31)
    assert np.array_equal(full["ids"].cpu().numpy(), G["ids_after"])
    assert torch.equal(full["ids"], generate.greedy_decode(eng, batch))
    out = generate.generate(eng, batch, temperature=0.0, stop_at_eos=True, max_new_tokens=31)
    ids = out["ids"].cpu().numpy()
    assert out["n_generated"].tolist() == k.tolist()
    assert out["steps"] <= int(k.max()) + 1 == 13
    for b in range(4):
        end = prefix[b] + k[b]
        assert np.array_equal(ids[b, :end], G["ids_after"][b, :end]) and ids[b, end - 1] == 2      # up to and with the EOS
        assert np.array_equal(ids[b, end:], G["text_id_vqa"][b, 0, end:])                          # behind it: the prompt's ids
    # the validation path with --gen_stop_eos on and off
    m.args.gen_stop_eos = False
    best0, ex0 = m(batch, inference=True)
    sims0, ids0 = m.last_generation["similarities"].clone(), m.last_generation["ids"].clone()
    m.args.gen_stop_eos = True
    best1, ex1 = m(batch, inference=True)
    assert torch.equal(best0, best1) and torch.equal(sims0, m.last_generation["similarities"]) and ex0 == ex1
    assert not torch.equal(ids0, m.last_generation["ids"])                    # (the flag did take the other path)
    opt = types.SimpleNamespace(param_groups=[{"lr": 0.25}])
    stats, files = [], []
    for flag in (False, True):
        m.args.gen_stop_eos = flag
        d = tmp_path / f"stop{int(flag)}"
        args = types.SimpleNamespace(is_generation_task=True, dataset="nextqa", debug=False, output_dir=str(d))
        stats.append(engine.val_one_epoch(m, [golden_batch(G), golden_batch(G)], opt, epoch=1, args=args))
        files.append(json.load(open(d / "extracted_answers" / "extracted_answers_epoch1.json")))
    m.args.gen_stop_eos = False
    assert stats[0] == stats[1] and files[0] == files[1]


def test_sampling_end_to_end():
    m = model_of("tiny", torch.float32)                 # random LM head: near-flat logits
    eng = m.ensure_engine()
    batch = golden_batch(GOLDS["tiny"])
    kw = dict(temperature=1.0, top_p=0.95, stop_at_eos=False, max_new_tokens=31)
    a = generate.generate(eng, batch, seed=7, **kw)
    b = generate.generate(eng, batch, seed=7, **kw)
    c = generate.generate(eng, batch, seed=8, **kw)
    assert torch.equal(a["ids"], b["ids"]) and torch.equal(a["tokens"], b["tokens"])
    assert not torch.equal(a["tokens"], c["tokens"])
    g = generate.generate(eng, batch, temperature=1.0, top_p=1e-6, stop_at_eos=False, max_new_tokens=31, seed=3)
    assert torch.equal(g["ids"], generate.greedy_decode(eng, batch))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_twenty_rows_per_token_step(dtype):
    """--val_batch_size: the 7b_l2_peaked batch five times over (B = 20, a row count of the few-rows projections)."""
    m = model_of("7b_l2_peaked", dtype)
    G = GOLDS["7b_l2_peaked"]
    one = golden_batch(G)
    rep = lambda t: torch.cat([t] * 5)                  # noqa: E731
    batch = {"video": rep(one["video"]), "text_id": {"vqa": rep(one["text_id"]["vqa"])},
             "label": {"vqa": rep(one["label"]["vqa"])}, "video_start": {"vqa": one["video_start"]["vqa"] * 5},
             "prefix_index": {"vqa": one["prefix_index"]["vqa"] * 5}}
    out = generate.generate(m.ensure_engine(), batch, temperature=0.0, stop_at_eos=False, max_new_tokens=31)
    assert np.array_equal(out["ids"].cpu().numpy(), np.concatenate([G["ids_after"]] * 5))


def test_prompt_to_answer_on_the_synthetic_model():
    import answer
    m = model_of("tiny", torch.float32)
    tok = answer.copy.copy(m.tokenizer)
    tok.sp_model = answer.WordHashVocabulary(tok.n_words)
    batch = generate.prompt_batch(tok, ["what is the man doing", "why did the dog bark?"], options=["sleeping", "eating", "running"],
                                  max_seq_len=128, max_feats=10)
    ans = m.generate(batch, max_new_tokens=9, temperature=0.7, top_p=0.9, seed=0)
    g = m.last_generation
    assert set(g) == {"ids", "n_generated", "steps"} and len(ans) == 2
    n = g["n_generated"].tolist()
    assert all(1 <= x <= 9 for x in n) and g["steps"] <= 9
    for b, p in enumerate(batch["prefix_index"]["vqa"]):
        row = g["ids"][b].cpu()
        assert torch.equal(row[:p], batch["text_id"]["vqa"][b, 0, :p]) and int(row[p + n[b]:].abs().sum()) == 0
        assert isinstance(ans[b], list) and len(ans[b]) <= n[b]           # no vocabulary: token ids, cut at the EOS
        assert ans[b] == row[p:p + len(ans[b])].tolist()


def test_without_the_flags_nothing_changes(monkeypatch):
    """One `model(batch, inference=True)` without any of the new flags issues exactly what `greedy_decode` + `match_answers` —
    the two functions the validation path consisted of before the generation API, unchanged by it — issue on their own: the same
    number of library entry calls and of torch operator dispatches, and not one call of the new token-step entry.
    This counts calls at the Python boundary (every launch of this path is issued from an `ops.*` call or a torch operator), not
    kernels in a device trace, and its yardstick is this tree's `greedy_decode` + `match_answers`, not a run of the commit
    before: a change INSIDE those two functions would not be seen here. They are pinned bit for bit by tests/test_eval.py."""
    from torch.utils._python_dispatch import TorchDispatchMode
    m = model_of("tiny_peakedperm", torch.float32)
    eng = m.ensure_engine()
    batch = golden_batch(GOLDS["tiny_peakedperm"])
    count = {"lib": 0, "torch": 0, "decode_next": 0}

    class Count(TorchDispatchMode):
        def __torch_dispatch__(self, func, types_, args=(), kwargs=None):
            count["torch"] += 1
            return func(*args, **(kwargs or {}))

    def counted(name, fn):
        def call(*a, **k):
            count["lib"] += 1
            count["decode_next"] += name == "decode_next"
            return fn(*a, **k)
        return call

    for name, fn in list(vars(ops).items()):
        if callable(fn) and getattr(fn, "__module__", None) == ops.__name__ and not isinstance(fn, type):
            monkeypatch.setattr(ops, name, counted(name, fn))

    def run(f):
        for k in count:
            count[k] = 0
        with Count():
            f()
        torch.cuda.synchronize()
        return dict(count)

    def parent():
        ids = generate.greedy_decode(eng, batch)
        generate.match_answers(m, batch, ids)

    want = run(parent)
    del m.args.gen_stop_eos                              # as a run that never heard of the flag
    got = run(lambda: m(batch, inference=True))
    m.args.gen_stop_eos = False
    got_off = run(lambda: m(batch, inference=True))
    assert want["lib"] > 31 * 8 and want["decode_next"] == 0
    assert got == want and got_off == want
    m.args.gen_stop_eos = True
    on = run(lambda: m(batch, inference=True))
    m.args.gen_stop_eos = False
    assert on["decode_next"] >= 1 and on["torch"] < want["torch"]          # (the opt-in path: fewer torch kernels)

