#!/usr/bin/env python3
"""The bits of every token-step entry that picks a row, as one line per case that two trees can be diffed by: no model, seeded
synthetic operands, the public fvqa.ops API only (so the tool runs unchanged in any tree that has these entries), and per case

  case | sha256 over every operand after the launch (outputs and in/out state, in a fixed order)

Entries: decode_next (greedy, sampled), decode_next_ex, _trie, _pair (with and without a trie), _stream (with and without a trie),
_rules (min-p alone, a unigram ban with top-k's count, a bigram ban with a minimum length and min-p; its lines come last in each
group and are new beside a tree without the entry: compare the others), spec_step, spec_step_sample, tree_spec_step, tree_spec_step_sample, trie_jump_step. Shapes: V = 509 (ragged strided tails), 32000
(the row of e_i in LDS), 40003 (recomputed); 3 sequences or pairs, D = 32; T = 4 and 16 rows per pass for the chain and the jump
step, R = 4 and 64 for the tree; fp32 and both 16-bit storage types. Rows: one with planted tie groups (a group of equal logits
across rank k = 6, a larger one where the nucleus cuts), one of NaNs, peaked rows that let a chain or a walk run deep. The hand-made
trie has a node with 300 edges (more than a workgroup has threads), nodes with 3, 1 and 0 edges, edge tokens outside [0, V) on both
sides, a child outside the trie; rows sit at those nodes, at -1 and at a node outside the trie. Parameter sets: nucleus and
top-k-with-penalty (P_NUCLEUS, P_TOPK of tests/test_specsample_gpu.py), a penalty alone, greedy where the entry has it.

  python tools/pick_hashes.py [--out FILE] [--only TEXT] [--repeat N]
  (--only: the cases whose name holds TEXT; --repeat: launch every case N times — for a kernel trace, the hashes are the last run's)"""
import argparse
import hashlib
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "flipped-vqa_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from fvqa import constrain, ops, vocab  # noqa: E402

DEV = "cuda"
EOS, B, D, S, MAX_NEW, WALK, TILE = 2, 3, 32, 24, 40, 32, 32
VOCABS = {509: 3.0, 32000: 6.0, 40003: 6.0}
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
PARAMS = {"nucleus": dict(temperature=0.8, top_p=0.9, top_k=0, repetition_penalty=1.0),
          "topk_penalty": dict(temperature=1.3, top_p=1.0, top_k=6, repetition_penalty=1.5),
          "penalty": dict(temperature=1.0, top_p=1.0, top_k=0, repetition_penalty=1.3)}
RULES = {"min_p": dict(min_p=0.1, no_repeat_ngram=0, min_new_tokens=0),
         "ngram1": dict(min_p=0.0, no_repeat_ngram=1, min_new_tokens=0),
         "ngram2_minlen_min_p": dict(min_p=0.05, no_repeat_ngram=2, min_new_tokens=9)}
GREEDY = dict(temperature=0.0, top_p=1.0, top_k=0, repetition_penalty=1.0)
GREEDY_PENALTY = dict(GREEDY, repetition_penalty=1.3)
ANSWERS = [[10, 11, 12], [10, 11, 13, 14], [10, 15, 16, 17, 18], [20, 21, 22, 23, 24, 25], [20, 26, 27]]
POS, G0 = [5, 9, 7], [2, 3, 0]
T_ = lambda a, dt: torch.as_tensor(np.asarray(a), dtype=dt, device=DEV).contiguous()   # noqa: E731
I32 = lambda *s: torch.full(s, -7, dtype=torch.int32, device=DEV)                      # noqa: E731
F32 = lambda *s: torch.full(s, float("nan"), dtype=torch.float32, device=DEV)          # noqa: E731


def rows_of(V, n, seed):
    """n logits rows: random; row 0 of every three with the planted tie groups, row 1 of every three NaN (when nan), the others
    peaked at one token so that drafts built from the arg-max are accepted some rows deep."""
    rng = np.random.default_rng(seed)
    lg = (VOCABS[V] * rng.standard_normal((n, V))).astype(np.float32)
    for r in range(n):
        order = np.argsort(-lg[r])
        if r % 3 == 0:
            lg[r, order[4:9]] = lg[r, order[4]]                      # equal logits across rank 6
            lg[r, order[12:60]] = lg[r, order[12]]                   # ... and where a nucleus of 0.9 cuts
        elif r % 3 == 2:
            lg[r, order[0]] += 6.0
    return lg


def ids_of(V, lg, seed):
    rng = np.random.default_rng(seed)
    ids = rng.integers(3, V, (lg.shape[0], S)).astype(np.int64)
    ids[:, 3:7] = np.argsort(-np.nan_to_num(lg), axis=1)[:, :4]      # the most likely tokens sit in the penalised span
    ids[0, 4] = V + 11                                               # ... beside an id outside the vocabulary
    return ids


def make_trie(V):
    """node 0: 300 edges (a token below 0 in front, one beyond V behind); node 1: 3 edges (one token beyond V, one child outside
    the trie); nodes 2, 3: one edge each (a chain for the jump step); node 4: a leaf; node 5: one edge, the EOS."""
    t0 = np.concatenate([[-4], np.linspace(3, V - 1, 298).astype(np.int64), [V + 5]])
    et = np.concatenate([t0, [10, 11, V + 7], [12], [13], [EOS]]).astype(np.int32)
    ec = np.concatenate([1 + np.arange(300) % 5, [2, 99, 3], [3], [4], [4]]).astype(np.int32)
    nf = np.array([0, 300, 303, 304, 305, 305, 306], dtype=np.int32)
    return types.SimpleNamespace(node_first=T_(nf, torch.int32), edge_token=T_(et, torch.int32), edge_child=T_(ec, torch.int32))


def emb_of(V, dtype):
    return torch.randn(V, D, generator=torch.Generator().manual_seed(1)).to(dtype).to(DEV)


def digest(st):
    sha = hashlib.sha256()
    for k in sorted(st):
        if torch.is_tensor(st[k]):
            sha.update(k.encode())
            sha.update(st[k].detach().contiguous().view(torch.uint8).cpu().numpy().tobytes())
    return sha.hexdigest()


def state(V, dtype, lg, n_rows, seed, x_rows=None, **more):
    """The in/out operands every entry has, fresh: n_rows id rows; row 1 of every three is done in the second half of a pair."""
    ids = ids_of(V, lg[:n_rows], seed)
    return dict(logits=T_(lg, torch.float32), ids=T_(ids, torch.int64), pos=T_((POS * 2)[:n_rows], torch.int32),
                done=torch.zeros(n_rows, dtype=torch.int32, device=DEV),
                x=torch.full((x_rows or lg.shape[0], D), float("nan"), dtype=dtype, device=DEV), n_active=I32(1),
                pos64=torch.full((n_rows,), -7, dtype=torch.int64, device=DEV), **more)


def decode_cases(V, dtype, emb, trie):
    lg = rows_of(V, B, 10 + V)
    lg_nan = lg.copy()
    lg_nan[1] = np.nan
    lg2 = np.concatenate([lg, rows_of(V, B, 20 + V)[::-1]])          # the pairs' twins
    lg2_nan = np.concatenate([lg_nan, lg2[B:]])
    rng = np.random.default_rng(V)
    u = T_(rng.random(B), torch.float32)
    g0 = T_(G0, torch.int32)
    ex = lambda: dict(token=I32(B), n_kept=I32(B), logprob=F32(B), counter=torch.zeros(1, dtype=torch.int32, device=DEV))   # noqa: E731
    for name, prm in [("greedy", GREEDY), ("greedy_penalty", GREEDY_PENALTY)] + list(PARAMS.items()):
        kw = dict(u=u if prm["temperature"] > 0 else None, eos_id=EOS, stop_at_eos=True, **prm)
        for rows, tag in ((lg, ""), (lg_nan, "_nan")):
            if prm["repetition_penalty"] == 1.0 and prm["top_k"] == 0:
                def plain(rows=rows, kw=kw):
                    st = state(V, dtype, rows, B, V, token=I32(B), n_kept=I32(B))
                    ops.decode_next(st["logits"], emb, st["ids"], st["pos"], st["done"], st["x"], st["token"], st["n_kept"],
                                    st["n_active"], u=kw["u"], pos64=st["pos64"], temperature=kw["temperature"], top_p=kw["top_p"],
                                    eos_id=EOS, stop_at_eos=True)
                    return st
                yield f"decode_next/{name}{tag}", plain

            def ex_(rows=rows, kw=kw):
                st = state(V, dtype, rows, B, V, **ex())
                ops.decode_next_ex(st["logits"], emb, st["ids"], st["pos"], st["done"], g0, st["x"], st["token"], st["n_kept"],
                                   st["logprob"], st["n_active"], st["counter"], pos64=st["pos64"], **kw)
                return st
            yield f"decode_next_ex/{name}{tag}", ex_
            for nodes in ([0, 1, -1], [4, 7, 2], [1, 0, 5]):
                def trie_(rows=rows, kw=kw, nodes=nodes):
                    st = state(V, dtype, rows, B, V, node=T_(nodes, torch.int32), **ex())
                    ops.decode_next_trie(st["logits"], emb, st["ids"], st["pos"], st["done"], g0, st["x"], st["token"],
                                         st["n_kept"], st["logprob"], st["n_active"], st["counter"], st["node"], trie,
                                         pos64=st["pos64"], **kw)
                    return st
                yield f"decode_next_trie/{name}{tag}/nodes{nodes}", trie_
            for nodes in (None, [0, 1, -1]):
                for alpha, beta in ((0.5, 0.1), (1.0, 0.0)):
                    def pair_(rows=lg2 if rows is lg else lg2_nan, kw=kw, nodes=nodes, alpha=alpha, beta=beta):
                        st = state(V, dtype, rows, 2 * B, V, n_plausible=I32(B), **ex())
                        if nodes is not None:
                            st["node"] = T_(nodes, torch.int32)
                        ops.decode_next_pair(st["logits"], emb, st["ids"], st["pos"], st["done"], g0, st["x"], st["token"],
                                             st["n_kept"], st["n_plausible"], st["logprob"], st["n_active"], st["counter"],
                                             alpha=alpha, beta=beta, node=st.get("node"), trie=None if nodes is None else trie,
                                             pos64=st["pos64"], **kw)
                        return st
                    yield f"decode_next_pair/{name}{tag}/nodes{nodes}/a{alpha}b{beta}", pair_
            for nodes in (None, [0, 1, -1]):
                def stream_(rows=rows, kw=kw, nodes=nodes):
                    N, W = 3, 12
                    st = state(V, dtype, rows, B, V, out_tokens=I32(N, W), out_n_generated=I32(N), out_logprob=F32(N, W), **ex())
                    if nodes is not None:
                        st["node"] = T_(nodes, torch.int32)
                    uw = T_(np.random.default_rng(V + 1).random((W, N)), torch.float32) if kw["u"] is not None else None
                    ops.decode_next_stream(st["logits"], emb, st["ids"], st["pos"], st["done"], g0, st["x"], st["token"],
                                           st["n_kept"], st["logprob"], st["n_active"], st["counter"], T_([2, 0, 1], torch.int32),
                                           T_([12, 8, 20], torch.int32), st["out_tokens"], st["out_n_generated"],
                                           out_logprob=st["out_logprob"], node=st.get("node"), trie=None if nodes is None else trie,
                                           pos64=st["pos64"], **dict(kw, u=uw))
                    return st
                yield f"decode_next_stream/{name}{tag}/nodes{nodes}", stream_
            for rname, rules in RULES.items() if hasattr(ops, "decode_next_rules") else ():
                def rules_(rows=rows, kw=kw, rules=rules):
                    st = state(V, dtype, rows, B, V, **ex())
                    st["ids"][:, 7] = st["ids"][:, 5]                # (rows 0 and 2: the token at pos occurred before — a bigram to ban)
                    ops.decode_next_rules(st["logits"], emb, st["ids"], st["pos"], st["done"], g0, st["x"], st["token"],
                                          st["n_kept"], st["logprob"], st["n_active"], st["counter"], pos64=st["pos64"], **kw, **rules)
                    return st
                yield f"decode_next_rules/{name}{tag}/{rname}", rules_


def chain_cases(V, dtype, emb, trie):
    for T in (4, 16):
        lg = rows_of(V, B * T, 30 + V + T)
        lg[T + 1] = np.nan                                           # sequence 1, row 1: reached only behind an accepted draft
        arg = np.argmax(np.nan_to_num(lg, nan=-1e30), axis=1).reshape(B, T)
        w = np.full((B, T), -1, dtype=np.int32)
        w[:, 0] = 7
        w[:, 1:] = arg[:, :-1]                                       # drafts: the arg-max of the row in front ...
        w[0, min(3, T - 1)] = 8                                      # ... but one
        common = lambda: dict(ngen=T_([0, 2, 1], torch.int32), w=T_(w, torch.int32), len=T_([T, max(1, T // 2), 1], torch.int32),   # noqa: E731
                              start=I32(B), token=I32(B, T), logprob=F32(B, T), n_committed=I32(B), n_drafted=I32(B),
                              counter=torch.zeros(1, dtype=torch.int32, device=DEV))
        drafts = T_(np.random.default_rng(V + T).integers(0, V, (B, MAX_NEW)), torch.int32)
        for src in ("given", "lookup"):
            dkw = dict(max_new_tokens=MAX_NEW, draft_tokens=drafts if src == "given" else None, lookup_ngram=2, eos_id=EOS,
                       stop_at_eos=True)

            def greedy(dkw=dkw):
                st = state(V, dtype, lg, B, V, **common())
                ops.spec_step(st["logits"], emb, st["ids"], st["pos"], st["done"], st["ngen"], st["w"], st["len"], st["start"],
                              st["x"], st["token"], st["logprob"], st["n_committed"], st["n_drafted"], st["n_active"],
                              st["counter"], pos64=st["pos64"], **dkw)
                return st
            yield f"spec_step/T{T}/{src}", greedy
            for name, prm in PARAMS.items():
                def sampled(dkw=dkw, prm=prm):
                    st = state(V, dtype, lg, B, V, n_kept=I32(B, T), **common())
                    u = T_(np.random.default_rng(V + 2).random((MAX_NEW, B)), torch.float32)
                    ops.spec_step_sample(st["logits"], emb, st["ids"], st["pos"], st["done"], st["ngen"], T_(G0, torch.int32),
                                         st["w"], st["len"], st["start"], st["x"], st["token"], st["n_kept"], st["logprob"],
                                         st["n_committed"], st["n_drafted"], st["n_active"], st["counter"], u=u, pos64=st["pos64"],
                                         **dkw, **prm)
                    return st
                yield f"spec_step_sample/T{T}/{src}/{name}", sampled
        for nodes in (None, [0, 1, 2]):
            for want in (False, True):
                def jump(nodes=nodes, want=want):
                    st = state(V, dtype, lg, B, V, **common())
                    st.update(logprob_pick=F32(B), logprob_fed=F32(B, T))
                    if nodes is not None:
                        st["node"] = T_(nodes, torch.int32)
                    ops.trie_jump_step(st["logits"], emb, st["ids"], st["pos"], st["done"], st["ngen"], st.get("node"), st["w"],
                                       st["len"], st["start"], st["x"], st["token"], st["logprob_pick"], st["logprob_fed"],
                                       st["n_committed"], st["n_active"], st["counter"], None if nodes is None else trie,
                                       max_new_tokens=MAX_NEW, chain_eos=True, want_logprobs=want, pos64=st["pos64"], eos_id=EOS)
                    return st
                yield f"trie_jump_step/T{T}/nodes{nodes}/logprobs{int(want)}", jump


def tree_cases(V, dtype, emb, trie):
    hp = vocab.plan_draft(constrain.compile_constraints(ANSWERS, EOS, V), B)
    plan = {k: torch.as_tensor(hp[k], dtype=torch.int32).to(DEV).contiguous() for k in ("n_plan", "token", "depth", "end", "parent")}
    ptok, ppar = np.asarray(hp["token"]).reshape(-1), np.asarray(hp["parent"]).reshape(-1)
    n_plan = int(np.asarray(hp["n_plan"]).reshape(-1)[0])
    for R in (4, 64):
        lg = rows_of(V, B * R, 40 + V + R)
        for b in range(B):                                           # local row j of sequence b: peaked at a child's token
            for j in range(min(R, n_plan)):
                kids = [r for r in range(n_plan) if ppar[r] == j]
                if kids and (b + j) % 4 != 3:
                    lg[b * R + j, ptok[kids[(b + j) % len(kids)]]] = lg[b * R + j].max() + 7.0
        lg[2 * R] = np.nan
        tiles = (R + TILE - 1) // TILE
        common = lambda: dict(ngen=T_([0, 2, 1], torch.int32), node=T_([0, 0, -1], torch.int32),   # noqa: E731
                              len=T_([R, max(1, R // 2), 1], torch.int32), start=I32(B), depth=I32(B * R), end=I32(B * R),
                              tile_anc=I32(B * tiles * TILE), path=I32(B, WALK), n_path=I32(B), start_old=I32(B), token=I32(B, WALK),
                              logprob=F32(B, WALK), n_committed=I32(B), n_drafted=I32(B), n_on_trie=I32(1),
                              counter=torch.zeros(2, dtype=torch.int32, device=DEV))

        def greedy():
            st = state(V, dtype, lg, B, V, **common())
            ops.tree_spec_step(st["logits"], emb, plan, st["ids"], st["pos"], st["done"], st["ngen"], st["node"], st["len"],
                               st["start"], st["x"], st["depth"], st["end"], st["tile_anc"], st["path"], st["n_path"],
                               st["start_old"], st["token"], st["logprob"], st["n_committed"], st["n_drafted"], st["n_active"],
                               st["n_on_trie"], st["counter"], max_new_tokens=MAX_NEW, pos64=st["pos64"], eos_id=EOS,
                               stop_at_eos=True)
            return st
        yield f"tree_spec_step/R{R}", greedy
        for name, prm in PARAMS.items():
            def sampled(prm=prm):
                st = state(V, dtype, lg, B, V, n_kept=I32(B, WALK), **common())
                u = T_(np.random.default_rng(V + 3).random((MAX_NEW, B)), torch.float32)
                ops.tree_spec_step_sample(st["logits"], emb, plan, st["ids"], st["pos"], st["done"], st["ngen"],
                                          T_(G0, torch.int32), st["node"], st["len"], st["start"], st["x"], st["depth"], st["end"],
                                          st["tile_anc"], st["path"], st["n_path"], st["start_old"], st["token"], st["n_kept"],
                                          st["logprob"], st["n_committed"], st["n_drafted"], st["n_active"], st["n_on_trie"],
                                          st["counter"], u=u, max_new_tokens=MAX_NEW, pos64=st["pos64"], eos_id=EOS,
                                          stop_at_eos=True, **prm)
                return st
            yield f"tree_spec_step_sample/R{R}/{name}", sampled


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--only", default="")
    ap.add_argument("--repeat", type=int, default=1)
    args = ap.parse_args()
    lines = []
    for dname, dtype in DTYPES.items():
        for V in VOCABS:
            emb, trie = emb_of(V, dtype), make_trie(V)
            for family in (decode_cases, chain_cases, tree_cases):
                for name, run in family(V, dtype, emb, trie):
                    case = f"{dname}/V{V}/{name}"
                    if args.only not in case:
                        continue
                    for _ in range(args.repeat):
                        st = run()
                    torch.cuda.synchronize()
                    lines.append(f"{case} {digest(st)}")
                    print(lines[-1], flush=True)
    print(f"{len(lines)} cases", flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
