"""What the nine token-step wrappers of fvqa/ops.py refuse, on the GPU with real device tensors: one table of (entry, operand,
defect), each damaging a single operand of an otherwise valid call. Every case must raise a ValueError that names the entry and
must leave ids, pos and done with the bits they had — nothing was launched. Per entry the undamaged call succeeds: a wrapper that
refused everything would not pass. (A CPU tensor and a non-contiguous operand are refused by the check every wrapper of ops
shares, whose message names no entry: "fvqa ops need ..."; those two defects are held to that text.)"""
import types

import pytest
import torch

from fvqa import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROWS, V, D, S, T, K = 2, 32, 16, 8, 2, 2
N_REQ, WIDTH, MAX_NEW = 2, 4, 4
STATE = ("ids", "ids_in", "ids_out", "pos", "done")


def trie3(dev):
    """Three nodes: the root offers token 5 (-> node 1) and token 7 (-> node 2); both children are leaves."""
    t = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)   # noqa: E731
    return types.SimpleNamespace(node_first=t([0, 2, 2, 2]), edge_token=t([5, 7]), edge_child=t([1, 2]))


def valid(entry, T=T, dev=DEV):
    """The operands of a call of `entry` that succeeds, by name (every parameter of the wrappers can be passed by keyword)."""
    g = torch.Generator().manual_seed(0)
    i32 = lambda *shape, fill=0: torch.full(shape, fill, dtype=torch.int32, device=dev)   # noqa: E731
    f32 = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=dev)              # noqa: E731
    i64 = lambda n: torch.zeros(n, dtype=torch.int64, device=dev)                         # noqa: E731

    def rows_of(rows, n_logits):
        return dict(logits=torch.randn(n_logits, V, generator=g).to(dev), emb=torch.randn(V, D, generator=g).to(dev),
                    x_next=f32(n_logits, D), n_active=i32(1), pos=i32(rows, fill=3), done=i32(rows), pos64=i64(rows),
                    ids=torch.randint(3, V, (rows, S), generator=g, dtype=torch.int64).to(dev))

    if entry.startswith("decode_next"):
        pairs = entry == "decode_next_pair"
        rows = 2 * ROWS if pairs else ROWS                           # (2 pairs: the positive rows, then their twins)
        o = dict(rows_of(rows, rows), token=i32(ROWS), n_kept=i32(ROWS), u=torch.rand(ROWS, generator=g).to(dev), temperature=0.0)
        if entry != "decode_next":
            o.update(gen_start=i32(ROWS, fill=4), logprob=f32(ROWS), counter=i32(1), top_k=0, repetition_penalty=1.0)
        if entry not in ("decode_next", "decode_next_ex"):
            o.update(node=i32(ROWS), trie=trie3(dev))
        if pairs:
            o.update(n_plausible=i32(ROWS), alpha=0.5, beta=0.1)
        if entry == "decode_next_stream":
            o.update(req=torch.arange(ROWS, dtype=torch.int32, device=dev), budget=i32(N_REQ, fill=WIDTH),
                     out_tokens=i32(N_REQ, WIDTH, fill=-1), out_n_generated=i32(N_REQ), out_logprob=f32(N_REQ, WIDTH),
                     u=torch.rand(WIDTH, N_REQ, generator=g).to(dev))
        return o
    if entry in ("spec_step", "trie_jump_step"):
        o = dict(rows_of(ROWS, ROWS * T), n_generated=i32(ROWS), w=i32(ROWS, T, fill=-1), length=i32(ROWS, fill=1),
                 start=i32(ROWS), token=i32(ROWS, T), n_committed=i32(ROWS), counter=i32(1), max_new_tokens=MAX_NEW)
        o["w"][:, 0] = o["ids"][:, 3].int()                          # (the last committed token: the one at pos)
        if entry == "spec_step":
            o.update(logprob=f32(ROWS, T), n_drafted=i32(ROWS), draft_tokens=i32(ROWS, MAX_NEW, fill=-1), lookup_ngram=2)
        else:
            o.update(logprob_pick=f32(ROWS), logprob_fed=f32(ROWS, T), node=i32(ROWS), trie=trie3(dev))
        return o
    o = rows_of(ROWS, ROWS)                                          # beam_step, beam_step_trie: one sample of K = 2 slots
    o.update(ids_in=o.pop("ids"), ids_out=torch.zeros(ROWS, S, dtype=torch.int64, device=dev), score=f32(ROWS),
             n_generated=i32(ROWS), parent=i32(ROWS), token=i32(ROWS), counter=i32(1), num_beams=K)
    if entry == "beam_step_trie":
        o.update(node=i32(ROWS), trie=trie3(dev))
    return o


ENTRIES = ("decode_next", "decode_next_ex", "decode_next_trie", "decode_next_pair", "decode_next_stream", "spec_step",
           "trie_jump_step", "beam_step", "beam_step_trie")
EX = ENTRIES[1:5]
OTHER = {torch.int32: torch.int64, torch.int64: torch.int32, torch.float32: torch.float64}
SHORTER = {("decode_next_pair", "gen_start"), ("decode_next_pair", "u")}     # (read as their first B entries: longer is legal)


def get(o, name):
    return getattr(o["trie"], name[5:]) if name.startswith("trie.") else o[name]


def put(o, name, t):
    if name.startswith("trie."):
        o["trie"] = types.SimpleNamespace(**{**vars(o["trie"]), name[5:]: t})
    else:
        o[name] = t


def damage(entry, o, name, defect):
    if defect == "T17":
        o.clear()
        o.update(valid(entry, T=17))
    elif defect == "dtype":
        put(o, name, get(o, name).to(OTHER[get(o, name).dtype]))
    elif defect == "numel":                                          # one element, or one row, too many (or too few)
        t = get(o, name)
        if name == "trie.node_first":
            put(o, name, t[:1].clone())                              # (any length >= 2 is some trie's)
        elif (entry, name) in SHORTER:
            put(o, name, t[:-1].clone())
        else:
            put(o, name, torch.cat([t, torch.zeros_like(t[:1])]))
    elif defect == "noncontig":
        t = get(o, name)
        put(o, name, t.t().contiguous().t() if t.dim() == 2 else t.repeat_interleave(2)[::2])
        assert not get(o, name).is_contiguous() and get(o, name).shape == t.shape
    elif defect == "cpu":
        put(o, name, get(o, name).cpu())
    elif defect == "alias":
        o[name] = o["ids_in"]
    else:                                                            # a value: a keyword, or None in place of an operand
        o[name] = defect[1]
    if name == "u":
        o["temperature"] = 0.8                                       # (u is read, and so checked, only when sampling)
    if name == "lookup_ngram":
        o["draft_tokens"] = None                                     # (... and the n-gram only without given drafts)


def cases():
    out = []
    for e in ENTRIES:
        o = valid(e, dev="cpu")                                      # (collection touches no GPU)
        names = [k for k, v in o.items() if torch.is_tensor(v)] + (["trie." + k for k in vars(o["trie"])] if "trie" in o else [])
        for n in names:                                              # every tensor operand: its dtype and its size
            out += [(e, n, "dtype"), (e, n, "numel")]
        out += [(e, "logits", "noncontig"), (e, "pos", "cpu")]
        if "trie" in o:
            out.append((e, "trie.edge_token", "noncontig"))
        if e.startswith("decode_next"):
            out.append((e, "u", ("set", None)))                      # temperature > 0 without u
        if e in EX:
            out += [(e, "top_k", ("set", -1)), (e, "repetition_penalty", ("set", 0.5))]
        if e in ("trie_jump_step", "decode_next_pair", "decode_next_stream"):
            out += [(e, "trie", ("set", None)), (e, "node", ("set", None))]       # node without trie, and the reverse
        if e in ("spec_step", "trie_jump_step"):
            out.append((e, "w", "T17"))
        if e.startswith("beam_step"):
            out += [(e, "num_beams", ("set", 9)), (e, "ids_out", "alias")]
    out += [("spec_step", "lookup_ngram", ("set", 5)), ("decode_next_pair", "alpha", ("set", -0.5)),
            ("decode_next_pair", "beta", ("set", 1.5))]
    return out


def case_id(c):
    e, n, d = c
    return f"{e}-{n}-{d if isinstance(d, str) else d[1]}"


def test_the_table_reaches_every_check_the_issue_names():
    table = cases()
    assert len(set(map(case_id, table))) == len(table)
    for e in ENTRIES:
        mine = {(n, d) for x, n, d in table if x == e}
        assert ("emb", "numel") in mine and ("x_next", "numel") in mine and ("logits", "noncontig") in mine and ("pos", "cpu") in mine
    assert ("decode_next_stream", "out_logprob", "numel") in table and ("spec_step", "draft_tokens", "numel") in table


@pytest.mark.parametrize("entry,sampling", [(e, False) for e in ENTRIES] + [(e, True) for e in ENTRIES[:5]])
def test_the_undamaged_call_succeeds(entry, sampling):
    o = valid(entry)
    if sampling:
        o["temperature"] = 0.8
    getattr(ops, entry)(**o)
    torch.cuda.synchronize()
    n_active = int(o["n_active"][0])
    assert 0 <= n_active <= ROWS and int(o["counter"][0] if "counter" in o else 0) == 0
    pos = o["pos"][:ROWS].tolist()
    assert all(p >= 4 for p in pos), pos                             # every row took a token
    if "trie" in o and not sampling and entry != "trie_jump_step":
        assert set(o["token"].flatten().tolist()) <= {5, 7}          # ... from the root's two edges


@pytest.mark.parametrize("case", cases(), ids=case_id)
def test_a_damaged_operand_is_refused_before_any_launch(case):
    entry, name, defect = case
    o = valid(entry)
    damage(entry, o, name, defect)
    before = {k: (o[k], o[k].clone()) for k in STATE if k in o}
    shared = {"noncontig": "fvqa ops need contiguous tensors", "cpu": "fvqa ops need device tensors"}
    what = entry + ":" if name.startswith("trie.") or defect not in shared else shared[defect]
    with pytest.raises(ValueError, match=what):
        getattr(ops, entry)(**o)
    torch.cuda.synchronize()
    for k, (t, was) in before.items():
        assert torch.equal(t, was), k
