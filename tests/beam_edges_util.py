"""Case builders and the fp64 yardstick of tests/test_beam_edges_gpu.py (csrc/beam.hip: fvqa_beam_step, fvqa_beam_step_trie,
fvqa_kv_beam_move). CPU only; tests/test_beam_edges_cpu.py checks every premise stated here.

The yardstick is `beam_step_ref` / `beam_step_trie_ref` below: tests/test_beam_cpu.py::beam_step_ref and
tests/test_constrained_cpu.py::beam_step_trie_ref extended to the inputs those two never see. On every input they accept, the
extensions return what they return (asserted in the CPU tests on the cases of tests/test_beam_gpu.py::step_case and
tests/test_constrained_gpu.py::beam_trie_case). The extensions, each from the kernel's own text:

  NaN        `better`: "a NaN is never better"; the re-seat loop: "fewer than K comparable candidates: rows of NaN". So
             - a candidate whose value is NaN takes part nowhere (a live slot whose row holds a NaN has a NaN lse and offers
               nothing; a finished slot whose score is NaN offers nothing);
             - if fewer than K candidates remain, new slot i of the missing tail is a carried copy of OLD SLOT i: parent i,
               token -1, its score (the bits it had) and id row as they were, its node, done 1.
             torch.sort puts NaN first, so NaN candidates are dropped before the ranking.
  pos        a slot with pos < -1 is finished first, like one with pos + 1 >= S; pos = -1 is live and its token goes to column 0.
  order      candidates are ranked by (value descending, c = parent * V + token ascending) whatever the order of an edge list.
  trie       an edge token outside [0, V) is never offered; a child outside [0, n_nodes) is stored as n_nodes.
  x_next     the embedding row each new slot reads ("x_src"): its token, or for a carried slot the id at clamp(pos, 0, S - 1) of
             its row clamped into [0, V - 1]. pos64 = clamp(new pos, 0, S - 1).
  n_active   "running": the sample's new slot 0 is unfinished / any of its new slots is.

The candidate lists: each of the kernel's NT = 256 threads keeps the KMAX = 8 best candidates of its slice — tokens
v = tid (mod 256) of every parent, edge indices i = tid (mod 256) under a trie, the one candidate of a finished slot in thread
0 — so `owner` below says which thread's list a winner is popped from, and the builders plant winners that share one."""
import numpy as np
import torch

from fvqa.constrain import TokenTrie

NT, KMAX = 256, 8
GAP = 1e-3                    # tests/test_beam_gpu.py::GAP (asserted equal in the CPU tests)
NEG = float("-inf")
NAN = float("nan")
EOS = 2
S_E, D_E = 8, 36              # (36 elements: 16-bit rows that are no multiple of 16 bytes, fp32 rows that are)
V_TRIE = 4096


# ------------------------------------------------------------------------------------------------ the yardstick
def _step_ref(logits, score, done, pos, ids, n_generated, node, trie, eos_id, stop_at_eos):
    logits = torch.as_tensor(logits, dtype=torch.float64)
    score = torch.as_tensor(score, dtype=torch.float64)
    ids = torch.as_tensor(ids, dtype=torch.int64)
    K, V = logits.shape
    S = ids.shape[1]
    pos = [int(p) for p in pos]
    fin = [bool(d) or p < -1 or p + 1 >= S for d, p in zip(done, pos)]       # no room (or no position): finished first
    offers = [None] * K
    if trie is not None:
        node = [int(n) for n in node]
        for j in range(K):
            if fin[j] or node[j] == -1:
                continue
            if not 0 <= node[j] < trie.n_nodes:
                fin[j] = True
                continue
            toks, kids = (np.asarray(a).astype(np.int64) for a in trie.children(node[j]))
            keep = (toks >= 0) & (toks < V)
            if not keep.any():
                fin[j] = True
                continue
            kids = np.where((kids < 0) | (kids >= trie.n_nodes), trie.n_nodes, kids)
            offers[j] = (torch.from_numpy(toks[keep]), torch.from_numpy(kids[keep]))
    vals, pars, toks, kids = [], [], [], []
    for j in range(K):
        if fin[j]:
            vals.append(score[j:j + 1]); pars.append(torch.tensor([j])); toks.append(torch.tensor([-1]))
            kids.append(torch.tensor([node[j] if trie is not None else -1]))
            continue
        l = logits[j]
        m = l.max()
        lse = m + torch.log(torch.exp(l - m).sum())
        t, c = (torch.arange(V), torch.full((V,), -1)) if offers[j] is None else offers[j]
        vals.append(score[j] + (l[t] - lse)); pars.append(torch.full((t.numel(),), j)); toks.append(t); kids.append(c)
    vals, pars, toks, kids = torch.cat(vals), torch.cat(pars), torch.cat(toks), torch.cat(kids)
    keep = ~torch.isnan(vals)                                                  # a NaN takes part nowhere
    vals, pars, toks, kids = vals[keep], pars[keep], toks[keep], kids[keep]
    by_c = torch.sort(pars * V + toks.clamp(min=0), stable=True).indices       # candidate number ascending ...
    vals, pars, toks, kids = vals[by_c], pars[by_c], toks[by_c], kids[by_c]
    order = torch.sort(vals, descending=True, stable=True).indices[:K + 1]     # ... kept among equal values
    ranked = [(float(vals[o]), int(pars[o]), int(toks[o])) for o in order]
    out = {"parent": [], "token": [], "ids": [], "pos": [], "score": [], "done": [], "n_generated": [], "node": [],
           "ranked": ranked, "n_comparable": int(vals.numel())}
    for i in range(K):
        if i < len(order):
            o = order[i]
            val, j, v, kid = float(vals[o]), int(pars[o]), int(toks[o]), int(kids[o])
        else:                                                                  # the missing tail: old slot i, carried
            val, j, v, kid = float(score[i]), i, -1, (node[i] if trie is not None else -1)
        row = ids[j].clone()
        if v < 0:
            out["pos"].append(pos[j]); out["done"].append(1); out["n_generated"].append(int(n_generated[j]))
        else:
            row[pos[j] + 1] = v
            out["pos"].append(pos[j] + 1)
            out["done"].append(1 if stop_at_eos and v == eos_id else 0)
            out["n_generated"].append(int(n_generated[j]) + 1)
        out["parent"].append(j); out["token"].append(v); out["ids"].append(row); out["score"].append(val)
        out["node"].append(kid)
    out["ids"] = torch.stack(out["ids"])
    clamp = lambda x, hi: min(max(int(x), 0), hi)                               # noqa: E731
    out["x_src"] = [v if v >= 0 else clamp(ids[j, clamp(pos[j], S - 1)], V - 1) for j, v in zip(out["parent"], out["token"])]
    out["pos64"] = [clamp(p, S - 1) for p in out["pos"]]
    out["running"] = (int(out["done"][0] == 0), int(0 in out["done"]))
    if trie is None:
        del out["node"]
    return out


def beam_step_ref(logits, score, done, pos, ids, n_generated, *, eos_id=EOS, stop_at_eos=True):
    """tests/test_beam_cpu.py::beam_step_ref, extended (module docstring). ONE sample, fp64. -> its dict, plus x_src, pos64,
    running and n_comparable."""
    return _step_ref(logits, score, done, pos, ids, n_generated, None, None, eos_id, stop_at_eos)


def beam_step_trie_ref(logits, score, done, pos, ids, n_generated, node, trie, *, eos_id=EOS, stop_at_eos=True):
    """tests/test_constrained_cpu.py::beam_step_trie_ref, extended (module docstring). -> beam_step_ref's dict plus "node"."""
    return _step_ref(logits, score, done, pos, ids, n_generated, node, trie, eos_id, stop_at_eos)


def reference(case):
    """The yardstick on every sample of a case -> list of dicts."""
    K = case["K"]
    out = []
    for b in range(case["logits"].shape[0] // K):
        sl = slice(b * K, (b + 1) * K)
        a = (case["logits"][sl].double(), case["score"][sl].double(), case["done"][sl].tolist(), case["pos"][sl].tolist(),
             case["ids"][sl], case["ngen"][sl].tolist())
        kw = dict(eos_id=case["eos"], stop_at_eos=case["stop"])
        out.append(beam_step_ref(*a, **kw) if case["trie"] is None else
                   beam_step_trie_ref(*a, case["node"][sl], case["trie"], **kw))
    return out


def score_bound(logits):
    """-> (bound, dev32): 4 x what torch's own fp32 log_softmax deviates from fp64 on these logits (floor 1e-6), the bound of
    tests/test_beam_gpu.py::test_beam_step_follows_the_rule_in_fp64; entries that are not finite in fp64 (rows with a NaN,
    logits of -inf) do not count."""
    ref = torch.log_softmax(logits.double(), -1)
    dev = (torch.log_softmax(logits, -1).double() - ref).abs()
    dev = dev[torch.isfinite(ref) & torch.isfinite(dev)]
    dev32 = float(dev.max()) if dev.numel() else 0.0
    return max(4.0 * dev32, 1e-6), dev32


def assert_decidable(case, refs):
    """Among the best K + 1 candidates of every sample two neighbours are a planted exact tie — both named in the sample's
    `ties`, or both at -inf (the candidates of empty slots and of -inf logits, planted as such) — or at least GAP apart."""
    for b, (r, ties) in enumerate(zip(refs, case["ties"])):
        for (v0, p0, t0), (v1, p1, t1) in zip(r["ranked"][:-1], r["ranked"][1:]):
            if v0 == v1:
                assert v0 == NEG or ((p0, t0) in ties and (p1, t1) in ties), (case["name"], b, (v0, p0, t0), (v1, p1, t1))
            else:
                assert v0 - v1 >= GAP, (case["name"], b, (v0, p0, t0), (v1, p1, t1))


def owner(case, b, parent, token):
    """The thread whose list holds candidate (parent, token) of sample b."""
    if token < 0:
        return 0
    if case["trie"] is not None and case["node"][b * case["K"] + parent] != -1:
        toks = np.asarray(case["trie"].children(case["node"][b * case["K"] + parent])[0])
        return int(np.nonzero(toks == token)[0][0]) % NT
    return token % NT


def assert_premises(case, refs):
    """What each sample's builder says of it (`expect`): the winners in order, candidates that must not appear, the threads
    that own the winners, the number of slots of the missing tail, the new done flags."""
    for b, (r, e) in enumerate(zip(refs, case["expect"])):
        got = list(zip(r["parent"], r["token"]))
        where = (case["name"], b, got)
        if "winners" in e:
            assert got == e["winners"], where
        for c in e.get("absent", ()):
            assert c not in got, where
        if "owners" in e:
            assert [owner(case, b, p, t) for p, t in got] == e["owners"], where
        if "tail" in e:
            assert case["K"] - min(r["n_comparable"], case["K"]) == e["tail"], where
        if "done" in e:
            assert r["done"] == e["done"], where
        if "node" in e:
            assert r["node"] == e["node"], where
        if "running" in e:
            assert r["running"] == e["running"], where


# ------------------------------------------------------------------------------------------------ samples and launches
def blank(K, V, seed, live=(0,), S=S_E, sd=1.0):
    """One sample: rows of N(0, sd) logits, the slots of `live` at score 0 and the others empty (-inf), positions with room."""
    g = torch.Generator().manual_seed(seed)
    pos = torch.randint(1, S - 3, (K,), generator=g).to(torch.int32)
    s = {"logits": (sd * torch.randn(K, V, generator=g)).float(), "score": torch.full((K,), NEG),
         "done": torch.zeros(K, dtype=torch.int32), "pos": pos, "ngen": pos.clone(), "ids": torch.randint(min(3, V - 1), V, (K, S), generator=g), "node": [-1] * K,
         "ties": set(), "expect": {}}
    for j in live:
        s["score"][j] = 0.0
    return s


def launch(name, K, samples, *, eos=EOS, stop=True, trie=None, D=D_E, emb_offset=0):
    """Samples of one K and V -> a case: the operands of one launch, host tensors."""
    cat = lambda k: torch.cat([s[k] for s in samples])                          # noqa: E731
    return {"name": name, "K": K, "logits": cat("logits"), "score": cat("score").float(), "done": cat("done"), "pos": cat("pos"),
            "ngen": cat("ngen"), "ids": cat("ids"), "node": [n for s in samples for n in s["node"]], "trie": trie, "eos": eos,
            "stop": stop, "ties": [s["ties"] for s in samples], "expect": [s["expect"] for s in samples], "D": D,
            "emb_offset": emb_offset}


def follow(case, refs, name):
    """The launch that follows: every slot as the yardstick left it (scores rounded to fp32), fresh logits."""
    g = torch.Generator().manual_seed(len(name))
    nxt = dict(case, name=name, logits=torch.randn(case["logits"].shape, generator=g).float(),
               score=torch.tensor([v for r in refs for v in r["score"]]).float(),
               done=torch.tensor([v for r in refs for v in r["done"]], dtype=torch.int32),
               pos=torch.tensor([v for r in refs for v in r["pos"]], dtype=torch.int32),
               ngen=torch.tensor([v for r in refs for v in r["n_generated"]], dtype=torch.int32),
               ids=torch.cat([r["ids"] for r in refs]), ties=[set() for _ in refs], expect=[{} for _ in refs])
    if case["trie"] is not None:
        nxt["node"] = [n for r in refs for n in r["node"]]
    return nxt


def make_emb(case, dtype):
    """The embedding table of a case, host: V rows of D values; with emb_offset the rows are a view that starts that many
    elements into its storage (whole 16-byte rows off a 16-byte boundary: copy_row's element-by-element branch)."""
    V, D, off = case["logits"].shape[1], case["D"], case["emb_offset"]
    flat = torch.randn(V * D + off, generator=torch.Generator().manual_seed(1)).to(dtype)
    return flat, off


# ---- 1: all winners in one thread's slice, one parent
def one_slice_sample(K, r, order, seed, others="empty"):
    """Slot 0 live; K + 1 logits planted at tokens r, r + 256, ..., r + 256 K, from 12 upwards in steps of 0.5 — `order`: rising
    along the token index (every insertion goes to the front of thread r's list), falling (every insertion appends) or
    shuffled. The lowest planted value is rank K + 1 and must not appear."""
    V = NT * (K + 2) + 3
    s = blank(K, V, seed)
    if others == "behind":
        s["score"][1:] = -50.0
    steps = {"rising": list(range(K + 1)), "falling": list(range(K, -1, -1)),
             "shuffled": torch.randperm(K + 1, generator=torch.Generator().manual_seed(seed)).tolist()}[order]
    for i, h in enumerate(steps):
        s["logits"][0, r + NT * i] = 12.0 + 0.5 * h
    by_value = sorted(range(K + 1), key=lambda i: -steps[i])
    s["expect"] = {"winners": [(0, r + NT * i) for i in by_value[:K]], "absent": [(0, r + NT * by_value[K])], "owners": [r] * K}
    return s


def one_slice_case(K):
    samples = [one_slice_sample(K, r, order, 10 * K + i, "behind" if order == "falling" else "empty")
               for i, (r, order) in enumerate((r, o) for r in (0, 255, 2) for o in ("rising", "falling", "shuffled"))]
    return launch(f"one slice, one parent, K={K}", K, samples)


def nine_and_one_case():
    """K = 8: nine planted in thread 2's slice (nine of the eleven tokens of the parent that thread 2 owns) and one in
    thread 77 that ranks 5th: seven winners from thread 2, the 5th from thread 77, the two lowest of the nine absent.
    Twice: the nine rising and falling along the token index."""
    K, r = 8, 2
    V = NT * (K + 2) + 3
    samples = []
    for order in ("rising", "falling"):
        s = blank(K, V, 90 + len(order))
        hs = list(range(9)) if order == "rising" else list(range(8, -1, -1))
        for i, h in enumerate(hs):
            s["logits"][0, r + NT * i] = 12.0 + 0.5 * h                       # values 12 .. 16
        s["logits"][0, 77 + NT * 3] = 14.25                                    # between the 4th (14.5) and the 5th (14.0) of them
        nine = sorted(range(9), key=lambda i: -hs[i])
        win = [(0, r + NT * i) for i in nine[:4]] + [(0, 77 + NT * 3)] + [(0, r + NT * i) for i in nine[4:7]]
        s["expect"] = {"winners": win, "absent": [(0, r + NT * i) for i in nine[7:]], "owners": [2] * 4 + [77] + [2] * 3}
        samples.append(s)
    return launch("nine in one slice and one elsewhere", K, samples)


# ---- 2: all winners in one slice, one per parent
def one_per_parent_case():
    """K = 8, eight live parents; row j peaks (15 above a unit row) at token r + 256 j, the scores staggered by 0.5 in an order
    that is not the slots'. Sample 0: r = 7. Sample 1: r = 7, parents 2 and 5 exact twins (same score, same row: two candidates
    of thread 7's list that only their number tells apart). Sample 2: r = 0 with slot 3 finished and slot 6 out of room — their
    one candidate j * V sits in thread 0's list beside the six peaks."""
    K, V = 8, NT * 9 + 5
    stagger = [3, 6, 1, 4, 7, 0, 5, 2]                                         # rank of parent j among the eight

    def sample(r, seed):
        s = blank(K, V, seed, live=range(K))
        for j in range(K):
            s["logits"][j, r + NT * j] = 15.0
            s["score"][j] = -0.5 * stagger[j]
        return s
    by_rank = sorted(range(K), key=lambda j: stagger[j])
    a = sample(7, 21)
    a["expect"] = {"winners": [(j, 7 + NT * j) for j in by_rank], "owners": [7] * K}
    b = sample(7, 22)
    b["logits"][5] = b["logits"][2]
    b["score"][5] = b["score"][2] = -1.25                                      # twins between the first and the second of the rest
    t = 7 + NT * 2
    b["ties"] = {(2, t), (5, t)}
    rest = [j for j in by_rank if j not in (2, 5)]
    b["expect"] = {"winners": [(rest[0], 7 + NT * rest[0]), (2, t), (5, t)] + [(j, 7 + NT * j) for j in rest[1:]], "owners": [7] * K}
    c = sample(0, 23)
    c["done"][3] = 1                                                           # (score -2.0: rank 4)
    c["pos"][6] = S_E - 1                                                      # (score -2.5: rank 5)
    c["expect"] = {"winners": [(j, -1 if j in (3, 6) else NT * j) for j in by_rank], "owners": [0] * K}
    return launch("one slice, one winner per parent", K, [a, b, c])


# ---- 3: a tie group wider than K
TIE_TOKENS = (5, 64 + 40, 128 + 3, 192 + 60)        # threads of all four waves, lanes below and above 32


def wide_tie_case(K):
    """2K exactly equal values straddle rank K: K / 2 twin parents (one score, one row) times the four tokens of TIE_TOKENS, all
    at one logit — the candidates (j, t) of the twins share thread t. One strictly better candidate of another parent leads.
    The winners are that one and the K - 1 lowest candidate numbers of the group."""
    V = 700
    twins = (0, 3) if K == 4 else (1, 4, 6, 7)
    other = 1 if K == 4 else 0
    s = blank(K, V, 30 + K, live=twins + (other,))
    for t in TIE_TOKENS:
        s["logits"][twins[0], t] = 12.0
    for j in twins:
        s["logits"][j] = s["logits"][twins[0]]
        s["score"][j] = -1.0
    s["logits"][other, 300] = 14.0
    s["score"][other] = -0.25
    group = [(j, t) for j in twins for t in TIE_TOKENS]
    s["ties"] = set(group)
    s["expect"] = {"winners": [(other, 300)] + group[:K - 1], "owners": [300 % NT] + [t for _, t in group[:K - 1]]}
    return launch(f"a tie group of {2 * K} around rank K={K}", K, [s])


# ---- 4: vocabulary edges
def spaced_rows(K, V, seed, step=0.25):
    """Rows whose logits are a permutation of 0, step, 2 step, ...: every gap inside a row is at least `step`."""
    g = torch.Generator().manual_seed(seed)
    return torch.stack([step * torch.randperm(V, generator=g).float() for _ in range(K)])


def small_vocab_cases():
    out = []
    s = blank(8, 8, 41)                                                        # V = K = 8, one live slot: every token wins
    s["logits"] = spaced_rows(8, 8, 41)
    by_value = sorted(range(8), key=lambda v: -float(s["logits"][0, v]))
    s["expect"] = {"winners": [(0, v) for v in by_value], "owners": by_value}
    out.append(launch("V = K = 8", 8, [s]))
    s = blank(1, 1, 42)                                                        # V = 1, K = 1
    s["expect"] = {"winners": [(0, 0)]}
    out.append(launch("V = 1, K = 1", 1, [s, blank(1, 1, 43)]))
    for V in (255, 256, 257):                                                  # around the workgroup's width; the last token leads
        s = blank(3, V, 44 + V, live=(0, 1, 2), sd=0.25)
        s["score"][1], s["score"][2] = -0.5, -7.0
        s["logits"][0, V - 1], s["logits"][0, 0], s["logits"][1, V - 2], s["logits"][1, 3] = 9.0, 8.0, 9.0, 6.0
        s["expect"] = {"winners": [(0, V - 1), (1, V - 2), (0, 0)], "absent": [(1, 3)]}
        out.append(launch(f"V = {V}, K = 3", 3, [s]))
    s = blank(8, 8, 47, live=range(8))                                         # 64 candidates in the first eight threads
    s["logits"] = spaced_rows(8, 8, 47, step=1.0)
    s["score"] = -torch.tensor([0.0, 0.3, 0.6, 0.1, 0.4, 0.7, 0.2, 0.5])
    out.append(launch("V = 8, eight live parents", 8, [s]))
    return out


# ---- 5: NaN, -inf and the missing tail
def nan_case():
    K, V = 4, 300
    a = blank(K, V, 51, live=range(K))                                         # a live slot whose row holds one NaN: offers nothing
    a["score"] = torch.tensor([-1.0, -0.1, -2.0, -3.0])
    a["logits"][1, 17] = NAN
    for j in (0, 2, 3):
        a["logits"][j, 40 + j] = 10.0
    a["expect"] = {"tail": 0, "absent": [(1, t) for t in range(V)]}
    b = blank(K, V, 52, live=range(K))                                         # every row NaN: every slot is itself, carried
    b["logits"][:] = NAN
    b["score"] = torch.tensor([-1.0, NAN, NEG, -0.5])
    b["expect"] = {"winners": [(i, -1) for i in range(K)], "tail": K, "done": [1] * K, "running": (0, 0)}
    c = blank(K, V, 53, live=range(K))                                         # a finished slot with a NaN score: offers nothing
    c["score"] = torch.tensor([-1.0, NAN, -2.0, -0.7])
    c["done"][1] = 1
    c["logits"][0, 9] = c["logits"][2, 270] = c["logits"][3, 100] = 11.0
    c["expect"] = {"tail": 0, "absent": [(1, -1)]}
    d = blank(K, V, 54, live=range(K))                                         # exactly K - 2 comparable candidates
    d["logits"][0, 200] = NAN                                                  # slot 0 live on a NaN row; 1 and 3 finished;
    d["done"][1] = d["done"][2] = d["done"][3] = 1                             # 2 finished with a NaN score
    d["score"] = torch.tensor([-0.2, -3.0, NAN, -1.5])
    d["expect"] = {"winners": [(3, -1), (1, -1), (2, -1), (3, -1)], "tail": 2, "done": [1] * K}
    e = blank(K, V, 55)                                                        # -inf on half of a live row
    e["logits"][0, ::2] = NEG
    e["logits"][0, 1], e["logits"][0, 257], e["logits"][0, 299] = 9.0, 8.0, 7.0
    e["expect"] = {"tail": 0, "absent": [(0, t) for t in range(0, V, 2)]}
    f = blank(K, V, 56)                                                        # two finite logits, the rest -inf: the -inf
    f["logits"][0] = NEG                                                       # candidates follow in candidate order
    f["logits"][0, 150], f["logits"][0, 3] = 1.0, 0.0
    f["expect"] = {"winners": [(0, 150), (0, 3), (0, 0), (0, 1)], "tail": 0}
    return launch("NaN, -inf and the missing tail", K, [a, b, c, d, e, f])


# ---- 6: row bookkeeping
def bookkeeping_samples():
    K, V, S = 4, 300, S_E

    def peaked(seed, live=range(K)):
        s = blank(K, V, seed, live=live)
        s["score"] = torch.tensor([-0.1, -0.6, -1.1, -1.6])
        for j in range(K):
            s["logits"][j, 20 + 70 * j] = 14.0                                 # each live parent's child keeps its parent's rank
        return s
    a = peaked(61)                                                             # pos -1: column 0; pos -2: finished first, x_next
    a["pos"] = torch.tensor([-1, -2, S - 2, S - 1], dtype=torch.int32)         # from column 0; the last column; no room
    a["expect"] = {"winners": [(0, 20), (1, -1), (2, 160), (3, -1)]}
    b = peaked(62)                                                             # carried slots whose current id is outside [0, V)
    b["done"][0] = b["done"][2] = 1
    b["ids"][0, int(b["pos"][0])] = -5
    b["ids"][2, int(b["pos"][2])] = V + 3
    b["expect"] = {"winners": [(0, -1), (1, 90), (2, -1), (3, 230)]}
    c = peaked(63)                                                             # the EOS among the winners, at slot 0 and slot 2;
    c["logits"][0, EOS] = c["logits"][2, EOS] = 16.0                           # slot 3 stays live
    c["score"] = torch.tensor([-0.1, -9.0, -1.1, -1.6])
    c["expect"] = {"winners": [(0, EOS), (2, EOS), (3, 230), (0, 20)]}
    return [a, b, c]


def bookkeeping_cases():
    K, V = 4, 300
    first = launch("row bookkeeping, stop at the EOS", K, bookkeeping_samples())
    first["expect"][2].update(done=[1, 1, 0, 0], running=(0, 1))               # new slot 0 finished while slot 3 is live
    free = launch("row bookkeeping, stop_at_eos = 0", K, bookkeeping_samples(), stop=False)
    free["expect"][2].update(done=[0, 0, 0, 0], running=(1, 1))
    none = launch("row bookkeeping, eos_id = -1", K, bookkeeping_samples(), eos=-1)
    past = launch("row bookkeeping, eos_id = V", K, bookkeeping_samples(), eos=V)
    for c in (none, past):
        c["expect"][2].update(done=[0, 0, 0, 0])
    return [first, free, none, past]


# ---- 7: the ticket
def ticket_case(B):
    """K = 1, V = 4, S = 4, D = 4: B samples, every third finished; each row a permutation of (0, 1, 2, 3)."""
    g = torch.Generator().manual_seed(B)
    lg = torch.argsort(torch.rand(B, 4, generator=g), dim=1).float()
    done = (torch.arange(B) % 3 == 2).to(torch.int32)
    pos = torch.randint(0, 2, (B,), generator=g).to(torch.int32)
    c = {"name": f"the ticket at {B} samples", "K": 1, "logits": lg, "score": -torch.rand(B, generator=g).float(), "done": done,
         "pos": pos, "ngen": pos.clone(), "ids": torch.randint(0, 4, (B, 4), generator=g), "node": [-1] * B, "trie": None,
         "eos": -1, "stop": True, "D": 4, "emb_offset": 0}
    return c


def ticket_ref(c):
    """The rule at K = 1 on every sample at once, fp64 (checked against the yardstick on a stride of samples in the CPU tests):
    a finished sample is carried; a live one takes the largest logit's token. -> dict of tensors."""
    lg = c["logits"].double()
    B = lg.shape[0]
    live = c["done"] == 0
    tok = lg.argmax(1)
    lp = torch.log_softmax(lg, -1).gather(1, tok[:, None])[:, 0]
    ids = c["ids"].clone()
    rows = torch.arange(B)[live]
    ids[rows, (c["pos"][live] + 1).long()] = tok[live]
    cur = c["ids"][torch.arange(B), c["pos"].long()]
    return {"parent": torch.zeros(B, dtype=torch.int64), "token": torch.where(live, tok, torch.tensor(-1)), "ids": ids,
            "pos": c["pos"] + live.to(torch.int32), "done": c["done"].clone(), "ngen": c["ngen"] + live.to(torch.int32),
            "score": torch.where(live, c["score"].double() + lp, c["score"].double()), "x_src": torch.where(live, tok, cur),
            "n_active": int(live.sum())}


def wide_launch_case():
    """257 samples at K = 2: more workgroups than a workgroup has threads; every third sample with both slots finished."""
    K, V = 2, 40
    samples = []
    for b in range(257):
        s = blank(K, V, 700 + b, live=(0, 1))
        s["logits"] = spaced_rows(K, V, 700 + b)
        s["score"][1] = -0.125
        if b % 3 == 2:
            s["done"][:] = 1
        samples.append(s)
    return launch("257 samples at K = 2", K, samples)


# ---- 8: embedding rows
def emb_cases():
    out = []
    for name, D, off in (("D = 1", 1, 0), ("D = 8", 8, 0), ("D = 8, whole 16-byte words off their boundary", 8, 1),
                         ("D = 16, whole 16-byte words off their boundary", 16, 3)):
        c = launch("embedding rows: " + name, 4, bookkeeping_samples()[:2], D=D, emb_offset=off)
        out.append(c)
    return out


# ------------------------------------------------------------------------------------------------ tries by hand
def hand_trie(nodes, V=V_TRIE):
    """nodes: per node a list of (token, child) -> a TokenTrie around the CSR arrays as given (no check: some are meant to be
    broken)."""
    first = np.cumsum([0] + [len(n) for n in nodes]).astype(np.int32)
    et = np.array([t for n in nodes for t, _ in n], dtype=np.int64).astype(np.int32)
    ec = np.array([c for n in nodes for _, c in n], dtype=np.int64).astype(np.int32)
    return TokenTrie(first, et, ec, np.zeros(1, dtype=np.int32), {}, True, EOS, V, [0], [0])


def is_valid_csr(trie, V=V_TRIE):
    """What fvqa/constrain.py promises of a trie: node_first ascends from 0 to n_edges, every token in [0, V), every child a
    node, the tokens of a node strictly ascending."""
    nf, et, ec = (np.asarray(a).astype(np.int64) for a in (trie.node_first, trie.edge_token, trie.edge_child))
    ok = nf[0] == 0 and nf[-1] == et.size == ec.size and bool((np.diff(nf) >= 0).all())
    ok = ok and bool(((et >= 0) & (et < V)).all()) and bool(((ec >= 0) & (ec < trie.n_nodes)).all())
    return ok and all(bool((np.diff(et[a:b]) > 0).all()) for a, b in zip(nf[:-1], nf[1:]))


def fan(n, seed, leaf, V=V_TRIE, low=3):
    """n edges with distinct ascending tokens of [low, V), each to the node `leaf`."""
    rng = np.random.default_rng(seed)
    return [(int(t), leaf) for t in np.sort(rng.choice(np.arange(low, V), size=n, replace=False))]


def trie_sample(K, seed, nodes, live=(0,)):
    s = blank(K, V_TRIE, seed, live=live)
    s["node"] = list(nodes)
    return s


def long_list_cases():
    """Node 1: 600 edges; node 2: 2305 = 9 * 256 + 1 edges (thread 0 owns ten of them, the others nine); node 0 a leaf. The
    model's favourite token (logit 30) is on no list."""
    e600, e2305 = fan(600, 1, 0), fan(2305, 2, 0)
    trie = hand_trie([[], e600, e2305])
    free = sorted(set(range(3, V_TRIE)) - {t for t, _ in e600 + e2305})[0]
    out = []
    samples = []
    for i in (7, 87):                                                          # K = 3: edge indices i, i + 256, i + 512
        s = trie_sample(3, 80 + i, [1, 1, 1])
        s["logits"][0, free] = 30.0
        idx = [i + 256, i + 512, i]
        for h, at in enumerate(idx):
            s["logits"][0, e600[at][0]] = 14.0 - 0.5 * h
        s["expect"] = {"winners": [(0, e600[at][0]) for at in idx], "owners": [i] * 3, "node": [0, 0, 0], "absent": [(0, free)]}
        samples.append(s)
    out.append(launch("a node with 600 edges", 3, samples, trie=trie))
    samples = []
    for tid, n_planted, seed in ((0, 8, 83), (3, 9, 84), (0, 9, 85)):          # K = 8: eight, then nine, in one thread's slice
        s = trie_sample(8, seed, [2] * 8)
        s["logits"][0, free] = 30.0
        mine = list(range(tid, 2305, NT))
        hs = torch.randperm(n_planted, generator=torch.Generator().manual_seed(seed)).tolist()
        at = mine[len(mine) - n_planted:]                                      # (the thread's last entries: the ragged one included)
        for a, h in zip(at, hs):
            s["logits"][0, e2305[a][0]] = 12.0 + 0.5 * h
        by_value = [a for _, a in sorted(zip(hs, at), reverse=True)]
        s["expect"] = {"winners": [(0, e2305[a][0]) for a in by_value[:8]], "owners": [tid] * 8, "node": [0] * 8,
                       "absent": [(0, free)] + [(0, e2305[a][0]) for a in by_value[8:]]}
        samples.append(s)
    out.append(launch("a node with 2305 edges", 8, samples, trie=trie))
    return out


BAD_TOKENS = (-1, V_TRIE, 2 ** 31 - 1)


def unusable_token_case():
    """Node 1: 300 edges with tokens -1, V and 2^31 - 1 mixed in at indices on both sides of 256 (never offered: their children
    are node 3, which no new slot may take); node 2: only such tokens (its slot is finished first and carried with its node)."""
    edges = fan(300, 3, 0)
    bad_at = {0: -1, 130: V_TRIE, 255: 2 ** 31 - 1, 256: -1, 299: V_TRIE}
    for at, t in bad_at.items():
        edges[at] = (t, 3)
    trie = hand_trie([[], edges, [(t, 3) for t in BAD_TOKENS], []])
    K = 4
    s = trie_sample(K, 86, [1, 2, 1, 1], live=(0, 1))
    s["score"][1] = -5.0
    good = [at for at in (1, 257, 298) if at not in bad_at]
    for h, at in enumerate(good):
        s["logits"][0, edges[at][0]] = 14.0 - h
    s["expect"] = {"winners": [(0, edges[good[0]][0]), (0, edges[good[1]][0]), (0, edges[good[2]][0]), (1, -1)],
                   "node": [0, 0, 0, 2], "done": [0, 0, 0, 1]}
    return launch("unusable edge tokens", K, [s], trie=trie), bad_at


def child_lookup_cases():
    """Node 1: 700 edges; the winners sit at edge indices 300 and 600, whose children are -3 and n_nodes + 7 (both stored as
    n_nodes; the launch that follows finishes those slots). Node 2: the winning token stands twice, at indices 300 and 556 —
    one thread's second and third entry — with children 4 and 5: the lower index's child is taken (K = 1: one winner)."""
    e700 = fan(700, 4, 0)
    dup = fan(700, 5, 0)
    n_nodes = 6
    e700[300], e700[600] = (e700[300][0], -3), (e700[600][0], n_nodes + 7)
    dup[300], dup[556] = (dup[300][0], 4), (dup[300][0], 5)
    trie = hand_trie([[], e700, dup, [], [], []])
    s = trie_sample(2, 87, [1, 1])
    s["logits"][0, e700[600][0]], s["logits"][0, e700[300][0]] = 14.0, 13.0
    s["expect"] = {"winners": [(0, e700[600][0]), (0, e700[300][0])], "node": [n_nodes, n_nodes], "owners": [600 % NT, 300 % NT]}
    first = launch("child lookup at edge indices 300 and 600", 2, [s], trie=trie)
    a, b = trie_sample(1, 88, [2]), trie_sample(1, 89, [1])
    a["logits"][0, dup[300][0]] = 14.0
    a["ties"] = {(0, dup[300][0])}                                             # (the one candidate, offered twice)
    a["expect"] = {"winners": [(0, dup[300][0])], "node": [4]}
    b["logits"][0, e700[44][0]] = 14.0                                         # (K = 1 beside it: an edge of the first trip)
    b["expect"] = {"winners": [(0, e700[44][0])], "node": [0]}
    return first, launch("child lookup of a token that stands twice", 1, [a, b], trie=trie)


def node_cases():
    """Node values -2, n_nodes and n_nodes + 5 (finished first, carried with their node); a slot at -1 beside slots at nodes,
    one token offered by two parents; a parent swap under which the nodes move with the slots."""
    e1, e2 = [(50, 3), (900, 4)], [(50, 5), (2000, 3)]
    trie = hand_trie([[], e1, e2, [], [], []])
    n = trie.n_nodes
    K = 4
    a = trie_sample(K, 91, [-2, n, n + 5, 1], live=range(K))
    a["score"] = torch.tensor([-0.5, -1.0, -1.5, -2.0])
    a["logits"][3, 900] = 14.0
    a["expect"] = {"winners": [(0, -1), (1, -1), (2, -1), (3, 900)], "node": [-2, n, n + 5, 4], "done": [1, 1, 1, 0]}
    b = trie_sample(K, 92, [-1, 1, 2, 0], live=(0, 1, 2))                      # slot 0 unconstrained: its favourite is on no list;
    b["score"] = torch.tensor([-0.1, -0.6, -1.1, NEG])                         # token 50 from parents 0, 1 and 2
    b["logits"][0, 3000], b["logits"][0, 50], b["logits"][1, 50], b["logits"][2, 50] = 15.0, 14.0, 14.0, 14.0
    b["expect"] = {"winners": [(0, 3000), (1, 50), (2, 50), (0, 50)], "node": [-1, 3, 5, -1]}
    c = trie_sample(K, 93, [1, 2, 4, 2], live=range(K))                        # new slot 0 from old slot 1 and the reverse; a
    c["score"] = torch.tensor([-3.0, -0.1, -2.0, -9.0])                        # finished slot between them keeps its node
    c["done"][2] = 1
    c["logits"][0, 900], c["logits"][1, 2000], c["logits"][3, 50] = 14.0, 14.0, 14.0
    c["expect"] = {"winners": [(1, 2000), (2, -1), (0, 900), (3, 50)], "node": [3, 4, 4, 5]}
    return launch("node values, a free slot, a parent swap", K, [a, b, c], trie=trie)


# ------------------------------------------------------------------------------------------------ every case, by name
def step_cases():
    cases = [one_slice_case(K) for K in (2, 5, 8)] + [nine_and_one_case(), one_per_parent_case(), wide_tie_case(4), wide_tie_case(8)]
    cases += small_vocab_cases() + [nan_case()] + bookkeeping_cases() + [wide_launch_case()] + emb_cases()
    return {c["name"]: c for c in cases}


def trie_cases():
    first, twice = child_lookup_cases()
    after = follow(first, reference(first), "the launch after the lost children")
    after["expect"] = [{"winners": [(0, -1), (1, -1)], "done": [1, 1], "node": [6, 6]}]      # node n_nodes: finished first
    cases = long_list_cases() + [unusable_token_case()[0], first, after, twice, node_cases()]
    return {c["name"]: c for c in cases}


STEP_NAMES = list(step_cases())
TRIE_NAMES = list(trie_cases())
# the families that run in two storage types only (fp16 among them); every other one runs in all three
LARGE = ("257 samples at K = 2", "one slice, one parent, K=8", "nine in one slice and one elsewhere")


# ------------------------------------------------------------------------------------------------ the cache move
def move_ref(dst, src, src_seq, lo, hi, *, S, A, group=0, window_rows=None):
    """fvqa_kv_beam_move by torch indexing on host tensors, as include/fvqa.h and the head of csrc/beam.hip state it: for
    destination sequence n the k and v thirds of rows [max(lo, 0), min(hi, S)) come from sequence src_seq[n] (+ the first slot of
    n's group when group > 0); a source outside [0, n_src) moves nothing. window_rows None: the direct form, adapter rows go
    along. Otherwise the move inside one cache (src is dst as it was): a slot that is its own source moves nothing, "rows beyond
    the window are not moved" — at most the first window_rows rows from lo —, adapter rows stay. -> the new dst."""
    D = dst.shape[2] // 3
    n_dst, n_src = (dst.shape[1] - A) // S, (src.shape[1] - A) // S
    out = dst.clone()
    for n in range(n_dst):
        sq = int(src_seq[n]) + (n // group * group if group > 0 else 0)
        if not 0 <= sq < n_src or (window_rows is not None and sq == n):
            continue
        a, b = max(int(lo[n]), 0), min(int(hi[n]), S)
        if window_rows is not None:
            b = min(b, a + window_rows)
        if b > a:
            out[:, n * S + a:n * S + b, D:] = src[:, sq * S + a:sq * S + b, D:]
    if window_rows is None and A:
        out[:, n_dst * S:, D:] = src[:, n_src * S:, D:]
    return out


def poison(L, n_seq, S, A, D, dtype, seed):
    """A cache (L, n_seq * S + A, 3 * D) of random values (tests/test_beam_gpu.py::poison), host."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-30000, 30000, (L, n_seq * S + A, 3 * D), generator=g).to(dtype)


def row_dims(dtype):
    """D with rows of one third of exactly 16 bytes and of 48 bytes."""
    per16 = 16 // torch.empty(0, dtype=dtype).element_size()
    return per16, 3 * per16


# name -> dict(L, S, A, n_src, n_dst (direct) | N (window), D or "D16"/"D48", src_seq, lo, hi, group, window)
def move_cases():
    c = {}
    # ---- direct (dst is another buffer than src)
    c["direct: ranges past both ends, empty ranges, sources outside"] = dict(
        L=2, S=6, A=3, n_src=2, n_dst=7, D=40, group=0,
        src_seq=[0, 1, 1, -1, 2, 0, 1], lo=[-3, 0, 4, 0, 0, 2, -9], hi=[4, 9, 2, 6, 6, 2, 99])
    c["direct: sources relative to a group"] = dict(
        L=2, S=5, A=3, n_src=6, n_dst=6, D=40, group=3, src_seq=[2, 0, 1, 1, 3, 0], lo=[0, 1, 2, 0, -1, 3], hi=[5, 4, 3, 6, 5, 5])
    c["direct: no adapter rows"] = dict(L=3, S=4, A=0, n_src=1, n_dst=3, D=40, group=0, src_seq=[0, 0, 0], lo=[0, 1, 3], hi=[4, 3, 4])
    c["direct: L = 1, S = 1, 16 adapter rows of 16 bytes"] = dict(L=1, S=1, A=16, n_src=1, n_dst=2, D="D16", group=0, src_seq=[0, 0],
                                                                  lo=[0, 0], hi=[1, 0])
    c["direct: L = 1, S = 1, rows of 48 bytes, no adapter"] = dict(L=1, S=1, A=0, n_src=2, n_dst=3, D="D48", group=0,
                                                                   src_seq=[1, 2, 0], lo=[0, 0, -1], hi=[1, 1, 2])
    # ---- through the window (inside one cache)
    c["window: wider than the sequence"] = dict(L=2, S=6, A=16, N=6, D=40, group=3, window=11, src_seq=[1, 2, 0, 1, 0, 2],
                                                lo=[0, 2, -4, 1, 0, 0], hi=[6, 9, 6, 5, 6, 6])
    c["window: one row"] = dict(L=2, S=6, A=2, N=4, D=40, group=2, window=1, src_seq=[1, 0, 1, 1], lo=[2, 5, 0, 4], hi=[6, 6, 1, 4])
    c["window: ranges longer than the window, lo < 0"] = dict(
        L=2, S=9, A=2, N=6, D="D16", group=3, window=3, src_seq=[1, 2, 0, 2, 2, 0], lo=[2, 0, -2, 5, 7, 3], hi=[7, 9, 6, 9, 9, 6])
    c["window: every slot its own parent"] = dict(L=2, S=6, A=2, N=6, D=40, group=3, window=4, src_seq=[0, 1, 2, 0, 1, 2],
                                                  lo=[0] * 6, hi=[4] * 6)
    c["window: an 8-cycle and a permutation at K = 8"] = dict(
        L=1, S=4, A=16, N=16, D="D48", group=8, window=4, src_seq=[1, 2, 3, 4, 5, 6, 7, 0, 3, 0, 1, 2, 7, 4, 5, 6], lo=[0] * 16,
        hi=[4, 3, 4, 2, 4, 1, 4, 4] * 2)
    c["window: absolute sources"] = dict(L=2, S=5, A=3, N=6, D=40, group=0, window=5, src_seq=[5, 0, 1, 3, 2, 4],
                                         lo=[0, 1, 0, 2, 0, 0], hi=[5, 5, 3, 4, 5, 1])
    c["window: sources outside the cache"] = dict(L=2, S=5, A=3, N=6, D=40, group=3, window=5, src_seq=[-1, 0, 3, 3, 2, -4],
                                                  lo=[0] * 6, hi=[5] * 6)
    c["window: L = 1, S = 1"] = dict(L=1, S=1, A=0, N=2, D="D16", group=2, window=1, src_seq=[1, 0], lo=[0, -5], hi=[1, 7])
    return c


MOVE_NAMES = list(move_cases())


def move_tensors(spec, dtype, seed=0):
    """-> (dst before, src or None for the move inside dst, D)."""
    D = spec["D"] if isinstance(spec["D"], int) else row_dims(dtype)[0 if spec["D"] == "D16" else 1]
    if "window" in spec:
        return poison(spec["L"], spec["N"], spec["S"], spec["A"], D, dtype, seed + 3), None, D
    return (poison(spec["L"], spec["n_dst"], spec["S"], spec["A"], D, dtype, seed + 2),
            poison(spec["L"], spec["n_src"], spec["S"], spec["A"], D, dtype, seed + 1), D)


def move_want(spec, dst, src):
    kw = dict(S=spec["S"], A=spec["A"], group=spec["group"])
    if "window" in spec:
        return move_ref(dst, dst, spec["src_seq"], spec["lo"], spec["hi"], window_rows=spec["window"], **kw)
    return move_ref(dst, src, spec["src_seq"], spec["lo"], spec["hi"], **kw)
