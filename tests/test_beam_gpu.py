"""Beam search on the GPU: the beam step (fvqa_beam_step) against the fp64 restatement of tests/test_beam_cpu.py, the cache move
(fvqa_kv_beam_move) bit for bit against torch indexing, and `generate(num_beams=...)` end to end — against greedy on the
reference-made fixtures, against teacher-forced dense forwards of what it returns, and against a search written in Python that
takes every step's logits from dense forwards and never touches the new kernels."""
import os
import re
import subprocess
import sys
import types

import pytest
import torch

from fvqa import generate, ops
from tests.test_beam_cpu import beam_step_ref
from tests.test_eval import golden_batch
from tests.test_generate_gpu import CASES, GEN_EOS, model_of

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
NEG = float("-inf")
EOS = 2


# ------------------------------------------------------------------------------------------------ the beam step alone
S_STEP, D_STEP = 16, 36      # (36 elements: 16-bit rows that are no multiple of 16 bytes, fp32 rows that are)


def step_case(B, K, V, seed):
    """State and logits of one launch, host tensors. Planted per shape: twin slots (same score, same logits row) whose row holds
    an exact in-row tie at its maximum — both tie kinds decide slots inside the best K —, finished slots (one that wins, one that
    loses), an empty slot (-inf), a slot out of room. -> (dict of inputs, planted: per sample the set of tied (parent, token))."""
    g = torch.Generator().manual_seed(seed)
    N = B * K
    lg = (4.0 * torch.randn(N, V, generator=g)).float()
    score = -(0.25 + 3.0 * torch.rand(N, generator=g)).float()
    done = torch.zeros(N, dtype=torch.int32)
    pos = torch.randint(3, 9, (N,), generator=g).to(torch.int32)
    ngen = (pos - 2).clone()
    ids = torch.randint(3, V, (N, S_STEP), generator=g)
    planted = [set() for _ in range(B)]

    def in_row_tie(n, a, b):
        lg[n, a] = lg[n, b] = lg[n].max() + 3.0

    if K == 1:                                   # (2, 1, V): a tie inside the row; a row out of room
        in_row_tie(0, 7, V - 3)
        planted[0] = {(0, 7), (0, V - 3)}
        pos[1] = S_STEP - 1
    else:                                        # sample 0: twins 0 and 1
        in_row_tie(0, 11, V - 5)
        lg[1] = lg[0]
        score[1] = score[0] = -1.0
        planted[0] = {(0, 11), (0, V - 5), (1, 11), (1, V - 5)}
    if K >= 4:
        done[2], score[2] = 1, -0.5              # a finished slot in front of every live candidate
        score[K - 1] = NEG                       # an empty slot
        s1 = K                                   # sample 1
        pos[s1], score[s1] = S_STEP - 1, -0.3    # out of room with the best score: carried as slot 0
        done[s1 + 2], score[s1 + 2] = 1, -50.0   # a finished slot that drops out
    if K == 8:
        done[4], score[4] = 1, -2.2
        pos[5], score[5] = S_STEP - 1, -6.0
        done[K + 6], score[K + 6] = 1, -1.7
    return {"logits": lg, "score": score, "done": done, "pos": pos, "ngen": ngen, "ids": ids}, planted


def run_step(c, K, dtype, emb, count_any_live=False):
    N, V = c["logits"].shape
    d = lambda t: t.to(DEV).contiguous()                                       # noqa: E731
    st = {k: d(c[k]) for k in ("score", "done", "pos", "ngen")}
    ids_out = torch.full((N, S_STEP), -9, dtype=torch.int64, device=DEV)
    x = torch.full((N, emb.shape[1]), float("nan"), dtype=dtype, device=DEV)
    i32 = lambda n: torch.full((n,), -7, dtype=torch.int32, device=DEV)         # noqa: E731
    parent, token, act = i32(N), i32(N), i32(1)
    pos64 = torch.full((N,), -7, dtype=torch.int64, device=DEV)
    counter = torch.zeros(1, dtype=torch.int32, device=DEV)
    ops.beam_step(d(c["logits"]), emb, d(c["ids"]), ids_out, st["pos"], st["score"], st["done"], st["ngen"], pos64, parent,
                  token, x, act, counter, num_beams=K, eos_id=EOS, stop_at_eos=True, count_any_live=count_any_live)
    torch.cuda.synchronize()
    out = {"parent": parent, "token": token, "ids": ids_out, "pos": st["pos"], "score": st["score"], "done": st["done"],
           "ngen": st["ngen"], "pos64": pos64, "x": x, "n_active": act, "counter": counter}
    return {k: v.cpu() for k, v in out.items()}


# seeds for which every gap that is not a planted tie exceeds GAP (asserted in the test: a seed that stops doing so fails it)
STEP_SHAPES = [(3, 4, 512, 5), (2, 8, 32000, 4), (1, 2, 32000, 3), (2, 1, 512, 4)]
GAP = 1e-3


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("B,K,V,seed", STEP_SHAPES)
def test_beam_step_follows_the_rule_in_fp64(B, K, V, seed, dtype):
    c, planted = step_case(B, K, V, seed)
    emb = torch.randn(V, D_STEP, generator=torch.Generator().manual_seed(1)).to(dtype).to(DEV)
    r = run_step(c, K, dtype, emb)
    lg64 = c["logits"].double()
    # the bound on a score: 4 x what torch's own fp32 log_softmax deviates from fp64 on these logits (floor 1e-6)
    dev32 = float((torch.log_softmax(c["logits"], -1).double() - torch.log_softmax(lg64, -1)).abs().max())
    bound = max(4.0 * dev32, 1e-6)
    n_run = n_any = 0
    worst = 0.0
    for b in range(B):
        sl = slice(b * K, (b + 1) * K)
        want = beam_step_ref(lg64[sl], c["score"][sl].double(), c["done"][sl].tolist(), c["pos"][sl].tolist(), c["ids"][sl],
                             c["ngen"][sl].tolist(), eos_id=EOS)
        rk = want["ranked"]
        for (v0, p0, t0), (v1, p1, t1) in zip(rk[:-1], rk[1:]):                 # near ties would make the order undecidable
            if (p0, t0) in planted[b] and (p1, t1) in planted[b]:
                assert v0 == v1
            elif v1 != NEG:
                assert v0 - v1 > GAP, (b, (v0, p0, t0), (v1, p1, t1))
        assert r["parent"][sl].tolist() == want["parent"] and r["token"][sl].tolist() == want["token"], b
        assert torch.equal(r["ids"][sl], want["ids"])
        assert r["pos"][sl].tolist() == want["pos"] == r["pos64"][sl].tolist()
        assert r["done"][sl].tolist() == want["done"] and r["ngen"][sl].tolist() == want["n_generated"]
        for i in range(K):
            n, j, tok = b * K + i, b * K + want["parent"][i], want["token"][i]
            src = tok if tok >= 0 else int(c["ids"][j, int(c["pos"][j])])       # carried: the embedding of its current token
            assert torch.equal(r["x"][n].view(torch.uint8), emb[src].cpu().view(torch.uint8)), (b, i)
            got, ref = float(r["score"][n]), want["score"][i]
            if tok < 0 or ref == NEG:
                assert got == ref                                               # carried: the parent's score as it was
            else:
                worst = max(worst, abs(got - ref))
                assert abs(got - ref) <= bound, (b, i, got, ref, bound)
        n_run += want["done"][0] == 0
        n_any += 0 in want["done"]
    print(f"B={B} K={K} V={V}: largest score error {worst:.3e}, bound {bound:.3e} (torch fp32 log_softmax {dev32:.3e})")
    assert int(r["n_active"]) == n_run and int(r["counter"]) == 0
    again = run_step(c, K, dtype, emb)                                          # two launches: the same bits
    for k in r:
        assert torch.equal(r[k].view(torch.uint8) if r[k].is_floating_point() else r[k],
                           again[k].view(torch.uint8) if again[k].is_floating_point() else again[k]), k
    assert int(run_step(c, K, dtype, emb, count_any_live=True)["n_active"]) == n_any


# ------------------------------------------------------------------------------------------------ the cache move
L_MV, S_MV, A_MV = 3, 16, 10


def poison(L, n_seq, D, dtype, seed):
    """A cache (L, n_seq * S + A, 3 * D) of random values: whatever a launch writes that it should not have written shows."""
    g = torch.Generator().manual_seed(seed)
    rows = n_seq * S_MV + A_MV
    return torch.randint(-30000, 30000, (L, rows, 3 * D), generator=g).to(dtype).to(DEV)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("D", [256, 4096])
def test_fan_out_is_torch_indexing_bit_for_bit(D, dtype):
    B, K = 2, 3
    N = B * K
    src, dst = poison(L_MV, B, D, dtype, 1), poison(L_MV, N, D, dtype, 2)
    before = dst.clone()
    prefix = [5, 16, 0, 9, 12, 1]                                              # per destination slot (0: nothing; 16: every row)
    seq = [0, 0, 0, 1, 1, 1]
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)              # noqa: E731
    ops.kv_beam_move(dst, src, i32(seq), i32([0] * N), i32(prefix), S=S_MV, A=A_MV)
    torch.cuda.synchronize()
    want = before.clone()
    for n in range(N):
        want[:, n * S_MV:n * S_MV + prefix[n], D:] = src[:, seq[n] * S_MV:seq[n] * S_MV + prefix[n], D:]
    want[:, N * S_MV:, D:] = src[:, B * S_MV:, D:]                             # the adapter rows, behind the sequence rows
    assert torch.equal(dst.view(torch.uint8), want.view(torch.uint8))
    assert torch.equal(dst[:, :, :D].view(torch.uint8), before[:, :, :D].view(torch.uint8))        # the q third


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("D", [256, 4096])
def test_the_move_inside_a_cache_gets_cycles_right(D, dtype):
    """Sample 0 (slots 0-2): a 3-cycle; sample 1 (3-5): a swap and an identity slot; sample 2 (6-8): slot 7 keeps its rows and
    hands them to both other slots. Ranges differ per slot; the window is shorter than the sequence."""
    K, N, W = 3, 9, 6
    parent = [1, 2, 0, 1, 0, 2, 1, 1, 1]
    lo = [4, 4, 4, 9, 9, 9, 2, 2, 2]
    hi = [9, 10, 8, 12, 15, 11, 5, 7, 8]
    cache = poison(L_MV, N, D, dtype, 3)
    before = cache.clone()
    scratch = torch.empty(ops.kv_beam_move_scratch(N, W, D, L_MV, dtype), dtype=torch.uint8, device=DEV)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)              # noqa: E731
    ops.kv_beam_move(cache, cache, i32(parent), i32(lo), i32(hi), S=S_MV, A=A_MV, scratch=scratch, window_rows=W, group=K)
    torch.cuda.synchronize()
    want = before.clone()
    for n in range(N):
        s = n // K * K + parent[n]
        if s != n:
            want[:, n * S_MV + lo[n]:n * S_MV + hi[n], D:] = before[:, s * S_MV + lo[n]:s * S_MV + hi[n], D:]
    assert torch.equal(cache.view(torch.uint8), want.view(torch.uint8))
    for n in (5, 7):                                                           # the slots that are their own parent: untouched
        assert torch.equal(cache[:, n * S_MV:(n + 1) * S_MV].view(torch.uint8), before[:, n * S_MV:(n + 1) * S_MV].view(torch.uint8))
    assert torch.equal(cache[:, :, :D].view(torch.uint8), before[:, :, :D].view(torch.uint8))      # the q third
    assert torch.equal(cache[:, N * S_MV:].view(torch.uint8), before[:, N * S_MV:].view(torch.uint8))   # the adapter rows


# ------------------------------------------------------------------------------------------------ end to end
def eos_batch(pname, rows=None):
    G = GEN_EOS[pname[:pname.rindex("_peaked")]]
    b = golden_batch(G)
    if rows is not None:
        idx = torch.tensor(rows)
        b = {"video": b["video"][idx], "text_id": {"vqa": b["text_id"]["vqa"][idx]}, "label": {"vqa": b["label"]["vqa"][idx]},
             "video_start": {"vqa": [b["video_start"]["vqa"][i] for i in rows]},
             "prefix_index": {"vqa": [b["prefix_index"]["vqa"][i] for i in rows]}, "vid": [b["vid"][i] for i in rows]}
    return b


@pytest.mark.parametrize("pname,dtype", CASES)
def test_one_beam_is_greedy(pname, dtype, monkeypatch):
    eng = model_of(pname, dtype).ensure_engine()
    batch = eos_batch(pname)
    ref = generate.generate(eng, batch, temperature=0.0, stop_at_eos=True)
    one = generate.generate(eng, batch, temperature=0.0, stop_at_eos=True, num_beams=1)
    for k in ("ids", "n_generated", "tokens"):
        assert torch.equal(one[k], ref[k]), k
    assert one["steps"] == ref["steps"] and "beams" not in one
    monkeypatch.setattr(generate, "_BEAM_PATH_AT_ONE", True)                   # the new kernels at K = 1
    forced = generate.generate(eng, batch, temperature=0.0, stop_at_eos=True, num_beams=1)
    assert "beams" in forced and tuple(forced["beams"]["ids"].shape) == (4, 1, 128)
    assert torch.equal(forced["ids"], ref["ids"]) and torch.equal(forced["n_generated"], ref["n_generated"])
    assert forced["steps"] == ref["steps"]


# Samples 0 and 3 of gen_eos_tiny: the greedy answer of sample 0 ends with its first token (a hypothesis is finished and carried
# from step 1 on), sample 3 re-seats its lower slots at three of the first four steps (parents [0, 0, 1], [0, 0, 0], [0, 0, 0]).
# In fp64 (the CPU oracle's forward) the smallest gap between neighbouring candidates down to rank K + 1 over those four steps
# is 1.7e-2 / 2.4e-2 — samples 1 and 2 come as close as 2.4e-3 / 1.2e-2 and are not used.
ROWS = [0, 3]
K_E2E = 3


def dense_logits(eng, batch, ids):
    """One dense forward (LM head on every row) of the id rows `ids` (B, S) in place of the batch's own: -> (B, S, V) fp32."""
    B, S = ids.shape
    sub = {"video": batch["video"], "text_id": {"vqa": ids.cpu().view(B, 1, S)}, "label": {"vqa": batch["label"]["vqa"][:, 0:1]},
           "video_start": {"vqa": batch["video_start"]["vqa"], "vaq": batch["video_start"]["vqa"]}}
    with generate.vqa_stream_only(eng, "_gen_arena", "all"):
        eng.forward(sub)
        return eng.arena(B, S).logits.view(B, S, eng.V).clone()


@pytest.fixture(scope="module")
def tiny():
    """The fp32 tiny model on ROWS, the beam search's result, and the per-token tolerance: with the GREEDY `generate` (the code
    that was there before the search) the largest difference between a token's log-probability from the decode loop's logits and
    from one dense forward of the finished row — the two paths reduce in different orders —, times 4, floor 1e-5.
    Measured on an MI355X: 1.8e-8 (the two paths agree far below the floor; 1e-5 is the tolerance). Measured again, and
    printed, on every run."""
    eng = model_of("tiny_peakedperm", torch.float32).ensure_engine()
    batch = eos_batch("tiny_peakedperm", ROWS)
    seen = []
    real = ops.decode_next

    def spy(lg, *a, **k):
        seen.append(lg.clone())
        return real(lg, *a, **k)

    ops.decode_next = spy
    try:
        g = generate.generate(eng, batch, temperature=0.0, stop_at_eos=False, max_new_tokens=12)
    finally:
        ops.decode_next = real
    dense = dense_logits(eng, batch, g["ids"]).double().log_softmax(-1)
    worst = 0.0
    for b, p in enumerate(batch["prefix_index"]["vqa"]):
        for t, lg in enumerate(seen):
            tok = int(g["ids"][b, p + t])
            worst = max(worst, abs(float(lg[b].double().log_softmax(-1)[tok]) - float(dense[b, p - 1 + t, tok])))
    tol = max(4.0 * worst, 1e-5)
    print(f"greedy decode against dense forward: largest per-token difference of a log-probability {worst:.3e} -> tolerance {tol:.3e}")
    out = generate.generate(eng, batch, temperature=0.0, stop_at_eos=True, num_beams=K_E2E)
    return types.SimpleNamespace(eng=eng, batch=batch, tol=tol, out=out, prefix=batch["prefix_index"]["vqa"])


def test_scores_are_the_models(tiny):
    """Every returned hypothesis, teacher-forced through one dense forward: the sum of log_softmax at its generated positions is
    the score the search reports (a wrong cache row after a re-seat would show here)."""
    beams = tiny.out["beams"]
    B = len(ROWS)
    assert tuple(beams["ids"].shape) == (B, K_E2E, 128) and tuple(tiny.out["score"].shape) == (B,)
    assert torch.equal(tiny.out["ids"], beams["ids"][:, 0]) and torch.equal(tiny.out["score"], beams["score"][:, 0])
    for k in range(K_E2E):
        lp = dense_logits(tiny.eng, tiny.batch, beams["ids"][:, k]).double().log_softmax(-1)
        for b, p in enumerate(tiny.prefix):
            n = int(beams["n_generated"][b, k])
            assert n >= 1
            want = sum(float(lp[b, p - 1 + t, int(beams["ids"][b, k, p + t])]) for t in range(n))
            got = float(beams["score"][b, k])
            print(f"sample {b} slot {k}: {n} tokens, score {got:.6f}, teacher-forced {want:.6f}")
            assert abs(got - want) <= n * tiny.tol, (b, k, got, want)
        assert bool((beams["score"][:, k] <= beams["score"][:, max(k - 1, 0)]).all())          # slot order is score order


def test_search_against_a_restatement_on_dense_forwards(tiny):
    """Four steps of the rule in Python; each step's logits come from dense forwards of the slots' id rows."""
    eng, batch = tiny.eng, tiny.batch
    B, K, T = len(ROWS), K_E2E, 4
    got = generate.beam_search(eng, batch, max_new_tokens=T, stop_at_eos=True, num_beams=K, early_stop=False)
    ids = batch["text_id"]["vqa"][:, 0].unsqueeze(1).repeat(1, K, 1).clone()                  # (B, K, S)
    pos = [[p - 1] * K for p in tiny.prefix]
    score = [[0.0] + [NEG] * (K - 1) for _ in range(B)]
    done = [[0] * K for _ in range(B)]
    ngen = [[0] * K for _ in range(B)]
    ended_early = False
    for t in range(T):
        at = [[None] * K for _ in range(B)]
        for k in range(K):
            lg = dense_logits(eng, batch, ids[:, k])
            for b in range(B):
                at[b][k] = lg[b, min(max(pos[b][k], 0), 127)].double().cpu()
        for b in range(B):
            r = beam_step_ref(torch.stack(at[b]), score[b], done[b], pos[b], ids[b], ngen[b], eos_id=EOS)
            for (v0, _, _), (v1, _, _) in zip(r["ranked"][:-1], r["ranked"][1:]):
                assert v1 == NEG or v0 - v1 > 100 * tiny.tol, (t, b, r["ranked"])               # the order is decidable
            assert got["parents"][t, b].tolist() == r["parent"], (t, b)
            assert got["step_tokens"][t, b].tolist() == r["token"], (t, b)
            ids[b], pos[b], score[b], done[b], ngen[b] = r["ids"], r["pos"], r["score"], r["done"], r["n_generated"]
        ended_early |= t < T - 1 and any(1 in d for d in done)
    assert ended_early                                                          # a finished hypothesis was carried
    assert torch.equal(got["beams"]["ids"].cpu(), ids)
    assert got["beams"]["done"].tolist() == done and got["beams"]["n_generated"].tolist() == ngen
    for b in range(B):
        for k in range(K):
            assert abs(float(got["beams"]["score"][b, k]) - score[b][k]) <= max(ngen[b][k], 1) * tiny.tol, (b, k)


def test_the_stop(tiny):
    eng, batch = tiny.eng, tiny.batch
    full = generate.beam_search(eng, batch, max_new_tokens=31, stop_at_eos=True, num_beams=K_E2E, early_stop=False)
    out = tiny.out
    assert full["steps"] == 31
    assert torch.equal(out["ids"], full["ids"]) and torch.equal(out["score"], full["score"])
    assert torch.equal(out["n_generated"], full["n_generated"])
    tok0 = full["step_tokens"][:, :, 0]                                        # slot 0 is finished once it takes EOS (or is carried)
    first = [int(((tok0[:, b] == EOS) | (tok0[:, b] < 0)).nonzero()[0]) + 1 for b in range(len(ROWS))]
    print(f"slot 0 finished at steps {first}; the early stop ran {out['steps']} steps")
    assert out["steps"] <= max(first) + 2 < 31
    pen = generate.beam_search(eng, batch, max_new_tokens=31, stop_at_eos=True, num_beams=K_E2E, length_penalty=1.0)
    bm = pen["beams"]
    for b in range(len(ROWS)):
        rank = (bm["score"][b].cpu() / bm["n_generated"][b].cpu().float() ** 1.0).tolist()    # score / n_generated ** penalty
        best = rank.index(max(rank))                                           # (the lowest slot on ties)
        assert torch.equal(pen["ids"][b], bm["ids"][b, best]) and float(pen["score"][b]) == float(bm["score"][b, best])
        assert int(pen["n_generated"][b]) == int(bm["n_generated"][b, best])
    assert bool(bm["done"].bool().all()) or pen["steps"] == 31                 # it ran until no slot was live


def test_the_surface():
    m = model_of("tiny_peakedperm", torch.float32)
    batch = eos_batch("tiny_peakedperm")
    ans = m.generate(batch, num_beams=3)
    g = m.last_generation
    assert len(ans) == 4 and set(g) == {"ids", "n_generated", "steps", "score"} and tuple(g["score"].shape) == (4,)
    for b, p in enumerate(batch["prefix_index"]["vqa"]):
        assert ans[b] == [t for t in g["ids"][b, p:p + int(g["n_generated"][b])].tolist() if t != EOS]
    m.args.num_beams = 3
    try:
        best, extracted = m(batch, inference=True)
    finally:
        del m.args.num_beams
    assert torch.equal(m.last_generation["ids"], g["ids"])
    want_best, want_sims, want_ex = generate.match_answers(m, batch, g["ids"])
    assert torch.equal(best, want_best) and extracted == want_ex
    assert torch.equal(m.last_generation["similarities"], want_sims)


def test_answer_cli_with_beams():
    r = subprocess.run([sys.executable, "answer.py", "--random_init", "--synthetic", "--num_beams", "3", "--question",
                        "what is the man doing", "--max_new_tokens", "4"], cwd=os.path.join(ROOT, "flipped-vqa_amd"),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    at = max(i for i, ln in enumerate(lines) if ln.startswith("["))
    head = re.fullmatch(r"\[(\d+) tokens, (\d+) steps, log-probability (-\d+\.\d+)\]", lines[at])
    assert head, lines[at]
    n = int(head.group(1))
    toks = lines[at + 1].split() if at + 1 < len(lines) else []
    assert 1 <= n <= 4 and len(toks) in (n, n - 1) and all(t.isdigit() for t in toks)      # (an EOS is counted, not printed)
