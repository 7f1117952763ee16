"""csrc/beam.hip at its edges: fvqa_beam_step and fvqa_beam_step_trie against the fp64 yardstick of tests/beam_edges_util.py on
cases whose winners collide in one thread's candidate list (sorted insertion, the dropped ninth, the shift after a pop, ties
inside a list), on vocabularies around and below the workgroup's width, rows of NaN and the missing tail, the positions and ids
at which the clamps act, both count modes, the ticket word at its 65535 arrivals, every branch of the embedding-row copy, edge
lists longer than the workgroup with unusable tokens and lost children; fvqa_kv_beam_move bit for bit against torch indexing
at its clamps, its window contract and its smallest geometries. Every integer output and x_next are exact, a carried score is
the bits it had, a new score is within max(4 * dev32, 1e-6) of fp64 (dev32: torch's own fp32 log_softmax against fp64 on the
case's logits); every case is launched twice and gives the same bits. tests/test_beam_edges_cpu.py proves every case decidable
and what it says; profiles/beam_edges.log holds one run's figures and the mutations this file was seen to catch."""
import pytest
import torch

from fvqa import ops
from tests import beam_edges_util as U

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
NEG = U.NEG

STEP_CASES = U.step_cases()
TRIE_CASES = U.trie_cases()
_REFS = {}


def refs_of(case):
    """The yardstick's answer, computed once per case and shared."""
    if case["name"] not in _REFS:
        _REFS[case["name"]] = U.reference(case)
    return _REFS[case["name"]]


def bits(t):
    return t.contiguous().view(torch.uint8) if t.is_floating_point() else t


def emb_of(case, dtype):
    flat, off = U.make_emb(case, dtype)
    V, D = case["logits"].shape[1], case["D"]
    return flat.to(DEV)[off:off + V * D].view(V, D)


def run_case(case, dtype, emb, count_any_live=False, counter=None):
    """One launch on sentinel-filled outputs -> dict of host tensors (tests/test_beam_gpu.py::run_step)."""
    N = case["logits"].shape[0]
    S = case["ids"].shape[1]
    d = lambda t: t.to(DEV).contiguous()                                       # noqa: E731
    st = {k: d(case[k]) for k in ("score", "done", "pos", "ngen")}
    ids_out = torch.full((N, S), -9, dtype=torch.int64, device=DEV)
    x = torch.full((N, emb.shape[1]), float("nan"), dtype=dtype, device=DEV)
    i32 = lambda n: torch.full((n,), -7, dtype=torch.int32, device=DEV)         # noqa: E731
    parent, token, act = i32(N), i32(N), i32(1)
    pos64 = torch.full((N,), -7, dtype=torch.int64, device=DEV)
    if counter is None:
        counter = torch.zeros(1, dtype=torch.int32, device=DEV)
    kw = dict(num_beams=case["K"], eos_id=case["eos"], stop_at_eos=case["stop"], count_any_live=count_any_live)
    out = {}
    if case["trie"] is None:
        ops.beam_step(d(case["logits"]), emb, d(case["ids"]), ids_out, st["pos"], st["score"], st["done"], st["ngen"], pos64,
                      parent, token, x, act, counter, **kw)
    else:
        nd = torch.tensor(case["node"], dtype=torch.int32, device=DEV)
        ops.beam_step_trie(d(case["logits"]), emb, d(case["ids"]), ids_out, st["pos"], st["score"], st["done"], st["ngen"], pos64,
                           parent, token, x, act, counter, nd, case["trie"].to(DEV), **kw)
        out["node"] = nd
    torch.cuda.synchronize()
    out.update({"parent": parent, "token": token, "ids": ids_out, "pos": st["pos"], "score": st["score"], "done": st["done"],
                "ngen": st["ngen"], "pos64": pos64, "x": x, "n_active": act, "counter": counter})
    return {k: v.cpu() for k, v in out.items()}


def check_case(case, dtype):
    emb = emb_of(case, dtype)
    emb_host = emb.cpu()
    refs = refs_of(case)
    K = case["K"]
    r = run_case(case, dtype, emb)
    bound, dev32 = U.score_bound(case["logits"])
    worst = 0.0
    for b, want in enumerate(refs):
        sl = slice(b * K, (b + 1) * K)
        where = (case["name"], b)
        assert r["parent"][sl].tolist() == want["parent"] and r["token"][sl].tolist() == want["token"], where
        assert torch.equal(r["ids"][sl], want["ids"]), where
        assert r["pos"][sl].tolist() == want["pos"] and r["pos64"][sl].tolist() == want["pos64"], where
        assert r["done"][sl].tolist() == want["done"] and r["ngen"][sl].tolist() == want["n_generated"], where
        if "node" in want:
            assert r["node"][sl].tolist() == want["node"], where
        for i in range(K):
            n, j, tok = b * K + i, b * K + want["parent"][i], want["token"][i]
            assert torch.equal(bits(r["x"][n]), bits(emb_host[want["x_src"][i]])), (where, i)
            got, ref = float(r["score"][n]), want["score"][i]
            if tok < 0:                                                         # carried: the bits the parent's score had
                assert torch.equal(bits(r["score"][n:n + 1]), bits(case["score"][j:j + 1])), (where, i)
            elif ref == NEG:
                assert got == NEG, (where, i)
            else:
                worst = max(worst, abs(got - ref))
                assert abs(got - ref) <= bound, (where, i, got, ref, bound)
    print(f"{case['name']} {dtype}: largest score error {worst:.3e}, bound {bound:.3e} (torch fp32 log_softmax {dev32:.3e})")
    assert int(r["n_active"]) == sum(w["running"][0] for w in refs) and int(r["counter"]) == 0
    again = run_case(case, dtype, emb)                                          # two launches: the same bits
    for k in r:
        assert torch.equal(bits(r[k]), bits(again[k])), (case["name"], k)
    any_live = run_case(case, dtype, emb, count_any_live=True)
    assert int(any_live["n_active"]) == sum(w["running"][1] for w in refs) and int(any_live["counter"]) == 0
    for k in r:
        assert k == "n_active" or torch.equal(bits(r[k]), bits(any_live[k])), (case["name"], k)


short = lambda dt: str(dt).split(".")[-1]                                      # noqa: E731
STEP_PARAMS = [pytest.param(name, dt, id=f"{name}-{short(dt)}") for name in U.STEP_NAMES
               for dt in ((torch.float32, torch.float16) if name in U.LARGE else DTYPES)]


@pytest.mark.parametrize("name,dtype", STEP_PARAMS)
def test_beam_step_at_its_edges(name, dtype):
    check_case(STEP_CASES[name], dtype)


@pytest.mark.parametrize("name", U.TRIE_NAMES)
def test_beam_step_trie_at_its_edges(name):
    check_case(TRIE_CASES[name], torch.float32)


@pytest.mark.parametrize("dtype", DTYPES, ids=short)
def test_the_ticket_at_65535_samples(dtype):
    """The documented limit of the 16-bit arrival count, every third sample finished; then a second launch on the same counter
    word, not zeroed again."""
    c = U.ticket_case(65535)
    want = U.ticket_ref(c)
    emb = emb_of(c, dtype)
    emb_host = emb.cpu()
    bound, dev32 = U.score_bound(c["logits"])
    counter = torch.zeros(1, dtype=torch.int32, device=DEV)
    first = None
    for turn in range(2):
        r = run_case(c, dtype, emb, count_any_live=bool(turn), counter=counter)
        assert int(r["n_active"]) == want["n_active"] == 43690 and int(r["counter"]) == 0, turn
        assert torch.equal(r["parent"].long(), want["parent"]) and torch.equal(r["token"].long(), want["token"])
        assert torch.equal(r["ids"], want["ids"]) and torch.equal(r["pos"], want["pos"])
        assert torch.equal(r["pos64"], want["pos"].long())
        assert torch.equal(r["done"], want["done"]) and torch.equal(r["ngen"], want["ngen"])
        assert torch.equal(bits(r["x"]), bits(emb_host[want["x_src"]]))
        carried = want["token"] < 0
        assert torch.equal(bits(r["score"][carried]), bits(c["score"][carried]))
        err = float((r["score"].double() - want["score"])[~carried].abs().max())
        print(f"{c['name']} {dtype} launch {turn}: largest score error {err:.3e}, bound {bound:.3e} "
              f"(torch fp32 log_softmax {dev32:.3e})")
        assert err <= bound
        if first is not None:
            for k in r:
                assert torch.equal(bits(r[k]), bits(first[k])), k
        first = r


# ------------------------------------------------------------------------------------------------ the cache move
@pytest.mark.parametrize("dtype", DTYPES, ids=short)
@pytest.mark.parametrize("name", U.MOVE_NAMES)
def test_kv_beam_move_at_its_edges(name, dtype):
    spec = U.move_cases()[name]
    before, src, D = U.move_tensors(spec, dtype)
    want = U.move_want(spec, before, src)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)              # noqa: E731
    dst = before.to(DEV)
    scratch = filled = None
    if "window" in spec:
        n_bytes = ops.kv_beam_move_scratch(spec["N"], spec["window"], D, spec["L"], dtype)
        assert n_bytes == spec["L"] * spec["N"] * spec["window"] * 2 * D * before.element_size()
        filled = torch.arange(n_bytes, dtype=torch.int64).mul_(37).remainder_(251).to(torch.uint8)
        scratch = filled.to(DEV)
        ops.kv_beam_move(dst, dst, i32(spec["src_seq"]), i32(spec["lo"]), i32(spec["hi"]), S=spec["S"], A=spec["A"], scratch=scratch,
                         window_rows=spec["window"], group=spec["group"])
    else:
        src_dev = src.to(DEV)
        ops.kv_beam_move(dst, src_dev, i32(spec["src_seq"]), i32(spec["lo"]), i32(spec["hi"]), S=spec["S"], A=spec["A"],
                         group=spec["group"])
        torch.cuda.synchronize()
        assert torch.equal(bits(src_dev.cpu()), bits(src))                      # the source is only read
    torch.cuda.synchronize()
    got = dst.cpu()
    assert torch.equal(bits(got), bits(want)), name                             # every row outside the ranges keeps its bits
    assert torch.equal(bits(got[:, :, :D]), bits(before[:, :, :D]))             # the q third
    if "window" in spec:
        n = spec["N"] * spec["S"]
        assert torch.equal(bits(got[:, n:]), bits(before[:, n:]))               # adapter rows stay
        if "every slot its own parent" in name:
            assert torch.equal(bits(got), bits(before)) and torch.equal(scratch.cpu(), filled)    # nothing moved, nothing staged
        else:
            assert not torch.equal(scratch.cpu(), filled)
    moved = int((bits(got) != bits(before)).any(-1).sum())
    print(f"{name} {dtype}: D = {D}, {moved} byte rows differ from before, all as torch indexing puts them")
