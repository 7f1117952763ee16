"""Exact answer-vocabulary scoring: the log-probability of EVERY allowed answer behind a prompt, in one pass over a tree.

`generate(constraints=...)` searches the answer set (greedy, or a beam of <= 8 slots) and returns one member; `score_options` is
exact but scores the options written into the sample's own prompt. `score_vocab` is the classifier over an answer vocabulary:
the constraints compile into a trie (fvqa/constrain.py), every distinct prefix of every allowed answer — every INTERNAL node of
the trie — is one row, computed once:

  tree    the prompt is run ONCE (fvqa/score.py's prompt pass: the KV cache), then the rows of all samples go through the layers
          in one pass (rowpass.layers) with fvqa_attn_suffix_tree as the attention — a row sees the cached prompt and its
          ancestors —, the head runs on those rows in blocks of HEAD_BLOCK, and fvqa_trie_score reads each edge's
          log-probability off its parent's logits row and adds them up along every member's path.
  dense   every member is written behind its prompt, (B, M, S) id and label rows, DENSE_CHUNK members at a time through the
          dense option-scoring pass (score._dense_pass: the existing forward); the per-token losses fill the same edge table and
          the same reduction closes it. The fallback for a batch the planner turns down, and the cross-check.

The root's input is the prompt's last token (position prefix - 1), so the cache a row reads is [0, prefix - 1) and every edge's
logits come from a row of this pass: the prefill's logits are not needed.
"""
from __future__ import annotations

import os
from dataclasses import dataclass, field
from typing import Optional

import numpy as np
import torch

from . import constrain, ops, rowpass, score

ROUTES = ("tree", "dense")
DEFAULT_ROUTE = "tree"
HEAD_BLOCK = 1024        # rows of one LM-head call of the tree route: (HEAD_BLOCK + 1, V) fp32 logits, 131 MB at V = 32000
DENSE_CHUNK = 32         # members per dense forward (B * DENSE_CHUNK sequences; fvqa_option_pick takes <= 64 options)
PATH = ops.TREE_DEPTH_MAX + 1


@dataclass
class VocabPlan:
    """What plan_vocab found, host numpy arrays (int32 unless said). Per sample b — a shared trie is planned once and repeated —:
    rows: the trie's internal nodes in pre-order, R = the largest count, n_rows (B,); token (B, R) the row's input token (-1 at the
    root: the prompt's last token), depth, end, parent (B, R; parent -1 at the root), tile_anc (B, ceil(R / 32), 32) the proper
    ancestors of each tile's first row, root first, -1 behind them. Padding rows: token 0, depth 0, end = their own index + 1.
    edges: edge_parent, edge_token, edge_child (B, E) (the row the edge leads to, -1: a leaf), n_edges (B,), in pre-order of the
    parent and ascending token order.
    members (the distinct answers, in ascending order of their index): member_path (B, MU, 32) edges root first, member_len,
    member_index (B, MU) — the LOWEST index of the answer in the caller's list —, member_edge (B, MU) its leaf edge, n_members
    (B,); M: columns of the results = the longest caller's list.
    tree: whether the batch can take the tree route (why_dense says why not)."""
    B: int
    R: int
    E: int
    MU: int
    M: int
    shared: bool
    n_rows: np.ndarray
    token: np.ndarray
    depth: np.ndarray
    end: np.ndarray
    parent: np.ndarray
    tile_anc: np.ndarray
    edge_parent: np.ndarray
    edge_token: np.ndarray
    edge_child: np.ndarray
    n_edges: np.ndarray
    member_path: np.ndarray
    member_len: np.ndarray
    member_index: np.ndarray
    member_edge: np.ndarray
    n_members: np.ndarray
    tree: bool
    why_dense: str
    _dev: dict = field(default_factory=dict, repr=False)

    def members(self, b: int):
        """The token sequences (EOS included) of sample b's distinct members, in the order of the member tables."""
        return [[int(self.edge_token[b, e]) for e in self.member_path[b, m, :self.member_len[b, m]]]
                for m in range(int(self.n_members[b]))]

    def tables(self, device) -> dict:
        """The int32 device tensors the kernels read (made once per device)."""
        key = str(device)
        if key not in self._dev:
            names = ("n_rows", "depth", "end", "tile_anc", "edge_parent", "edge_token", "n_edges", "member_path", "member_len",
                     "member_index", "n_members")
            self._dev[key] = {k: torch.as_tensor(np.ascontiguousarray(getattr(self, k)), dtype=torch.int32).to(device)
                              for k in names}
        return self._dev[key]


def _plan_one(h: constrain.TokenTrie, root: int):
    """One sample's tables as python lists: the pre-order walk of the trie from `root`."""
    nf, et, ec = np.asarray(h.node_first), np.asarray(h.edge_token), np.asarray(h.edge_child)
    internal = lambda v: int(nf[v + 1]) > int(nf[v])                     # noqa: E731
    token, depth, parent, end = [], [], [], []
    e_parent, e_token, e_child, members = [], [], [], []
    # (node, its row's token, parent row, depth, the path of edges to it); children pushed in descending token order
    stack = [("in", root, -1, -1, 0, ())]
    while stack:
        item = stack.pop()
        if item[0] == "out":
            end[item[1]] = len(token)
            continue
        _, v, tok, par, d, path = item
        r = len(token)
        token.append(tok)
        depth.append(d)
        parent.append(par)
        end.append(-1)
        stack.append(("out", r))
        lo, hi = int(nf[v]), int(nf[v + 1])
        first = len(e_parent)
        for i in range(lo, hi):                                          # this row's edges, ascending token order
            e_parent.append(r)
            e_token.append(int(et[i]))
            e_child.append(-1)
        for i in range(hi - 1, lo - 1, -1):
            c, e = int(ec[i]), first + (i - lo)
            if internal(c):
                stack.append(("in", c, int(et[i]), r, d + 1, path + (e,)))
            else:
                members.append((h.leaf_choice[c], path + (e,)))
    # edge_child: the row whose (parent, token) the edge is (a child's row number is only known once it is popped)
    at = {(e_parent[e], e_token[e]): e for e in range(len(e_parent))}
    for r in range(1, len(token)):
        e_child[at[(parent[r], token[r])]] = r
    members.sort()
    return token, depth, parent, end, e_parent, e_token, e_child, members


def plan_draft(trie, B: int) -> dict:
    """The plan of a DRAFT trie (generate(draft_answers=C); include/fvqa.h fvqa_tree_spec_step): `_plan_one`'s pre-order walk
    without plan_vocab's limits — a draft trie may be deeper than 32 tokens and larger than one pass, the token step cuts every
    pass to what fits. -> host int32 arrays: shared (bool); a shared trie is planned ONCE — n_plan (1,), token, depth, end, parent
    (P,): the kernel reads it with a sample stride of 0 —; per-sample tries give n_plan (B,) and (B, P) tables, padded behind a
    sample's rows (token 0, depth 0, end = own index + 1, parent -1; never read: n_plan bounds every index). The root's token
    (-1) is not read: its input is the prompt's last token. The plan is kept on the host trie: a caller that compiles its
    TokenTrie once pays for the walk once."""
    h = trie.host()
    kept = h.__dict__.setdefault("_draft_plans", {})
    if int(B) not in kept:
        kept[int(B)] = _plan_draft(h, int(B))
    return kept[int(B)]


def _plan_draft(h: constrain.TokenTrie, B: int) -> dict:
    roots = [int(r) for r in h.roots(int(B))]
    per = {r: _plan_one(h, r)[:4] for r in set(roots)}
    ones = [per[roots[0]]] if h.shared else [per[r] for r in roots]
    P = max(len(o[0]) for o in ones)
    n = len(ones)
    out = dict(n_plan=np.zeros(n, dtype=np.int32), token=np.zeros((n, P), dtype=np.int32), depth=np.zeros((n, P), dtype=np.int32),
               end=np.tile(np.arange(1, P + 1, dtype=np.int32), (n, 1)), parent=np.full((n, P), -1, dtype=np.int32))
    for b, (token, depth, parent, end) in enumerate(ones):
        k = len(token)
        out["n_plan"][b] = k
        out["token"][b, :k], out["depth"][b, :k], out["end"][b, :k], out["parent"][b, :k] = token, depth, end, parent
    if h.shared:
        out = {k: (v if k == "n_plan" else v[0]) for k, v in out.items()}
    out["shared"] = bool(h.shared)
    return out


def plan_vocab(trie, B: int, prefix=None, S: Optional[int] = None, n_listed=None) -> VocabPlan:
    """Host-only integer work. trie: a constrain.TokenTrie; B: the batch size (a per-sample trie built for another one is a
    ValueError). prefix (one int per sample) and S: where each answer starts and the sequence length — given, the plan checks that
    every row lies inside the sequence (start + depth < S, start = prefix - 1) and every member fits (prefix + length <= S: a
    ValueError, as generate has it). n_listed: the length of each sample's list as the caller gave it (columns of the results;
    default: highest member index + 1).
    The tree route's limits (include/fvqa.h): depth of a row <= 31, rows per sample <= 4096, B * rows <= 65536, members per sample
    <= 4096; a batch outside them takes the dense route whole (tree False, why_dense)."""
    h = trie.host()
    roots = [int(r) for r in h.roots(int(B))]
    if prefix is not None and len(prefix) != B:
        raise ValueError(f"plan_vocab: {len(prefix)} prefix indices for a batch of {B}")
    per = {}
    for r in set(roots):
        per[r] = _plan_one(h, r)
    ones = [per[r] for r in roots]
    R = max(len(o[0]) for o in ones)
    E = max(len(o[4]) for o in ones)
    MU = max(len(o[7]) for o in ones)
    longest = max(len(p) for o in ones for _, p in o[7])
    if longest > PATH:
        # (the member tables hold 32 edges a path: a deeper trie is planned for its limits only)
        return _refused(B, h.shared, f"an answer of {longest} tokens with its EOS (> {PATH})")
    NT = (R + ops.TREE_TILE - 1) // ops.TREE_TILE
    z = lambda *s, fill=0: np.full(s, fill, dtype=np.int32)              # noqa: E731
    p = VocabPlan(B=B, R=R, E=E, MU=MU, M=0, shared=h.shared, n_rows=z(B), token=z(B, R), depth=z(B, R),
                  end=np.tile(np.arange(1, R + 1, dtype=np.int32), (B, 1)), parent=z(B, R, fill=-1),
                  tile_anc=z(B, NT, ops.TREE_TILE, fill=-1), edge_parent=z(B, E), edge_token=z(B, E), edge_child=z(B, E, fill=-1),
                  n_edges=z(B), member_path=z(B, MU, PATH, fill=-1), member_len=z(B, MU, fill=1), member_index=z(B, MU),
                  member_edge=z(B, MU), n_members=z(B), tree=True, why_dense="")
    for b, (token, depth, parent, end, e_parent, e_token, e_child, members) in enumerate(ones):
        n = len(token)
        p.n_rows[b] = n
        p.token[b, :n], p.depth[b, :n], p.parent[b, :n], p.end[b, :n] = token, depth, parent, end
        for t in range((n + ops.TREE_TILE - 1) // ops.TREE_TILE):
            chain, a = [], parent[t * ops.TREE_TILE]
            while a >= 0:
                chain.append(a)
                a = parent[a]
            if len(chain) <= ops.TREE_TILE:
                p.tile_anc[b, t, :len(chain)] = chain[::-1]
        ne = len(e_parent)
        p.n_edges[b] = ne
        p.edge_parent[b, :ne], p.edge_token[b, :ne], p.edge_child[b, :ne] = e_parent, e_token, e_child
        p.n_members[b] = len(members)
        for m, (idx, path) in enumerate(members):
            p.member_path[b, m, :len(path)] = path
            p.member_len[b, m], p.member_index[b, m], p.member_edge[b, m] = len(path), idx, path[-1]
    if n_listed is None:
        p.M = int(max(p.member_index[b, :p.n_members[b]].max() for b in range(B))) + 1
    else:
        listed = [int(n_listed)] * B if isinstance(n_listed, (int, np.integer)) else [int(x) for x in n_listed]
        if len(listed) != B or any(int(p.member_index[b, :p.n_members[b]].max()) >= listed[b] for b in range(B)):
            raise ValueError("plan_vocab: n_listed does not cover the members' indices")
        p.M = max(listed)
    why = ""
    deepest = int(max(p.depth[b, :p.n_rows[b]].max() for b in range(B)))
    if deepest > ops.TREE_DEPTH_MAX:
        why = f"a row of depth {deepest} (> {ops.TREE_DEPTH_MAX})"
    elif R > ops.TREE_ROWS_MAX:
        why = f"{R} rows in a sample (> {ops.TREE_ROWS_MAX})"
    elif B * R > ops.TREE_TOTAL_ROWS_MAX:
        why = f"{B} x {R} rows (> {ops.TREE_TOTAL_ROWS_MAX})"
    elif MU > ops.TREE_ROWS_MAX:
        why = f"{MU} members in a sample (> {ops.TREE_ROWS_MAX})"
    if prefix is not None:
        if S is None:
            raise ValueError("plan_vocab: prefix comes with S")
        for b in range(B):
            pre, n_tok = int(prefix[b]), int(p.member_len[b, :p.n_members[b]].max())
            if pre < 1:
                raise ValueError(f"plan_vocab: sample {b}: prefix index {pre} leaves no prompt token for the root row")
            if pre + n_tok > S:
                raise ValueError(f"plan_vocab: sample {b}: an allowed answer of {n_tok} tokens (EOS included) does not fit behind "
                                 f"the prompt of {pre} tokens inside max_seq_len = {S}")
            # (a row of depth d sits at prefix - 1 + d <= prefix + n_tok - 2 < S: every row lies inside the sequence)
    p.tree, p.why_dense = not why, why
    return p


def _refused(B, shared, why):
    z = np.zeros((B, 1), dtype=np.int32)
    return VocabPlan(B=B, R=0, E=0, MU=0, M=0, shared=shared, n_rows=z[:, 0], token=z, depth=z, end=z, parent=z,
                     tile_anc=np.zeros((B, 1, ops.TREE_TILE), dtype=np.int32), edge_parent=z, edge_token=z, edge_child=z,
                     n_edges=z[:, 0], member_path=np.zeros((B, 1, PATH), dtype=np.int32), member_len=z, member_index=z,
                     member_edge=z, n_members=z[:, 0], tree=False, why_dense=why)


def route_of(plan: VocabPlan) -> str:
    """FVQA_SCORE_VOCAB=tree|dense picks the route; a batch the planner turns down goes dense whatever was asked."""
    want = os.environ.get("FVQA_SCORE_VOCAB", "") or DEFAULT_ROUTE
    if want not in ROUTES:
        raise ValueError(f"FVQA_SCORE_VOCAB={want!r}: expected one of {ROUTES}")
    return want if plan.tree else "dense"


def _listed(constraints, B: int):
    """How long each sample's list is, as the caller wrote it (None for a compiled trie: the plan takes the highest index)."""
    if isinstance(constraints, constrain.TokenTrie):
        return None
    seqs = constraints.tolist() if isinstance(constraints, np.ndarray) else list(constraints)
    if all(constrain._is_seq_of_ints(constrain._plain(s)) for s in seqs):
        return [len(seqs)] * B
    return [len(s) for s in seqs]


def _tree(eng, data, ids_h, vs_list, prefix, plan: VocabPlan, events, top: int, by_mean: bool):
    dev = eng.device
    B, _, S = ids_h.shape
    R = plan.R
    t = plan.tables(dev)
    tok = torch.as_tensor(plan.token, dtype=torch.int64).clone()
    start = torch.as_tensor([p - 1 for p in prefix], dtype=torch.int64)
    tok[:, 0] = ids_h[torch.arange(B), 0, start]                         # the root's input: the prompt's last token
    saved = score._prompt_pass(eng, data, "vqa", ids_h, vs_list, events, "prompt pass")
    done = score._mark(events, "tree pass")
    start_d = start.to(torch.int32).to(dev, non_blocking=True)
    x = eng.pack.emb[tok.reshape(-1).to(dev, non_blocking=True)].contiguous()
    ar, m_ = saved["ar"], eng.model
    b = rowpass.buffers(eng, B * R, xin=False, lg=False)
    rotated = rowpass.cache_rotated(eng)

    def attn(i, qkv, o):
        ops.attn_suffix_tree(qkv, ar.qkv[i], o, *m_.gate_views(i), saved["vstart"], start_d, t["n_rows"], t["depth"], t["end"],
                             t["tile_anc"], (eng.cos, eng.sin), B, R, S, eng.H, eng.Dh, eng.A, eng.F, cache_rotated=rotated)
    x = rowpass.layers(eng, b, attn, x)
    done()
    done = score._mark(events, "tree head")
    e = lambda *s, dtype=eng.dtype: torch.empty(*s, dtype=dtype, device=dev)  # noqa: E731
    rows = B * R
    blk = min(HEAD_BLOCK, rows)
    xf, lg = e(blk, eng.D), e(blk + 1, eng.V, dtype=torch.float32)
    lse, rowloss = e(blk + 1, dtype=torch.float32), e(blk + 1, dtype=torch.float32)
    loss_sum = torch.zeros(2, dtype=torch.float32, device=dev)
    ones = torch.ones(blk + 1, dtype=torch.int64, device=dev)            # (every row has a label: fvqa_ce_fwd writes its lse)
    edge_lp = torch.zeros(B, plan.E, dtype=torch.float32, device=dev)
    out = None
    for r0 in range(0, rows, blk):
        n = min(blk, rows - r0)
        rowpass.head(eng, x[r0:r0 + n], xf[:n], lg[:n])
        ops.ce_fwd(lg[:n + 1], ones[:n + 1], lse, rowloss, loss_sum, 1, n + 1, eng.V, 0)
        out = ops.trie_score(t, edge_lp, B, R, eng.V, logits=lg, lse=lse, row0=r0, n_block_rows=n, reduce=r0 + n >= rows,
                             n_columns=plan.M, top=top, by_mean=by_mean)
    done()
    out["edge_logprob"] = edge_lp
    return out


def dense_rows(plan: VocabPlan, ids_h: torch.Tensor, prefix, m0: int, m1: int):
    """The dense route's host integers for the members [m0, m1) of every sample (a sample with fewer members repeats its first):
    ids, label (B, m1 - m0, S) — the member behind the prompt, its tokens as labels —, and where each edge's loss is read, once
    per edge: (b, e, c, t) int64 lists — edge e of sample b from column c, row t of this chunk's individual_losses."""
    B, _, S = ids_h.shape
    O = m1 - m0
    ids = ids_h[:, 0:1].repeat(1, O, 1)
    lab = torch.zeros(B, O, S, dtype=torch.int64)
    take = [[], [], [], []]
    seen = set()
    for b in range(B):
        nm, pre = int(plan.n_members[b]), int(prefix[b])
        ids[b, :, pre:] = 0                                               # (a reader's row holds its own answer there)
        for c in range(O):
            live = m0 + c < nm
            m = m0 + c if live else 0
            ln = int(plan.member_len[b, m])
            path = plan.member_path[b, m, :ln]
            toks = torch.as_tensor(plan.edge_token[b, path].astype(np.int64))
            if int(toks.min()) <= 0:
                raise ValueError("score_vocab: the dense route cannot score token 0 (the loss's ignore_index)")
            ids[b, c, pre:pre + ln] = toks
            lab[b, c, pre:pre + ln] = toks
            for i, e in enumerate(path.tolist() if live else []):
                if (b, e) not in seen:
                    seen.add((b, e))
                    for lst, v in zip(take, (b, e, c, pre - 1 + i)):
                        lst.append(v)
    return ids, lab, [torch.as_tensor(v, dtype=torch.int64) for v in take]


def _dense(eng, data, ids_h, vs_list, prefix, plan: VocabPlan, events, top: int, by_mean: bool):
    dev = eng.device
    B, _, S = ids_h.shape
    edge_lp = torch.zeros(B, plan.E, dtype=torch.float32, device=dev)
    done = score._mark(events, "dense forward")
    for m0 in range(0, plan.MU, DENSE_CHUNK):
        m1 = min(plan.MU, m0 + DENSE_CHUNK)
        ids, lab, (tb, te, tc, tt) = dense_rows(plan, ids_h, prefix, m0, m1)
        op = score.plan_options(ids, lab)
        tl, ar = score._dense_pass(eng, data, "vqa", ids, lab, vs_list)
        il = score._dense_pick(eng, tl, ar, op, B, m1 - m0, S)[0]
        mv = lambda v: v.to(dev, non_blocking=True)                      # noqa: E731
        edge_lp[mv(tb), mv(te)] = -il[mv(tb), mv(tc), mv(tt)]
    done()
    out = ops.trie_score(plan.tables(dev), edge_lp, B, max(plan.R, 1), eng.V, reduce=True, n_columns=plan.M, top=top,
                         by_mean=by_mean)
    out["edge_logprob"] = edge_lp
    return out


@torch.no_grad()
def score_vocab(eng, data: dict, constraints, *, route: Optional[str] = None, top: int = 5, length_penalty: float = 1.0,
                contrast=None, contrast_alpha: float = 1.0, events: Optional[list] = None):
    """data: a generation prompt batch (generate.prompt_batch, or a reader's generation batch: text_id['vqa'] (B, 1, S),
    prefix_index); constraints: as generate takes them — token sequences, one list for the batch or one per sample, or a TokenTrie.
    -> dict, all tensors on the device, M = the longest list as the caller gave it, padded with -inf / 0 behind a sample's last
    member (and at the later copies of a duplicate, which is scored at its lowest index):
      logprob_sum (B, M) fp32   log p(member | prompt): its tokens and its EOS, teacher-forced;
      count (B, M) int64        its length, EOS included;  mean = logprob_sum / count;
      log_posterior (B, M)      logprob_sum - logsumexp over the sample's members;
      ranking (B, top) int64    the best `top` <= 8 members, best first, by mean (length_penalty = 1: the criterion of score_options
                                and of the constrained beam) or by logprob_sum (length_penalty = 0); -1 behind the last member;
      prediction (B,) int64     ranking[:, 0];
      edge_logprob (B, E) fp32  the log-probability of every edge of the trie (plan.edge_parent / edge_token name them);
      route, plan.
    route: None = route_of(plan) (FVQA_SCORE_VOCAB, "tree" unless the planner turns the batch down); "tree" on such a batch is a
    ValueError. contrast ("blind" or a dict of replacement features, generate's keyword): the twin batch is scored by the same
    route; "prediction" becomes score.contrast_pick's rule on the means (as losses: argmin of -mean+ - alpha * (mean+ - mean-)),
    the result gains "mean_blind", "prediction_blind" and "prediction_plain"."""
    if length_penalty not in (0, 1, 0.0, 1.0):
        raise ValueError("score_vocab: length_penalty is 1 (rank by the mean) or 0 (rank by the sum)")
    if not 1 <= int(top) <= ops.TREE_TOP_MAX:
        raise ValueError(f"score_vocab: 1 <= top <= {ops.TREE_TOP_MAX}")
    if route is not None and route not in ROUTES:
        raise ValueError(f"score_vocab: route {route!r}: expected one of {ROUTES}")
    from .generate import _need_prefix, _twin
    _need_prefix(data)
    twin = None if contrast is None else _twin(data, contrast, contrast_alpha, 0.0)
    ids_h = data["text_id"]["vqa"].cpu()
    if ids_h.dim() != 3:
        raise ValueError("score_vocab: text_id['vqa'] must be (B, 1, S): a generation prompt batch")
    ids_h = ids_h[:, 0:1]                                 # (a reader's batch: option 0's row; only its prompt is read)
    B, _, S = ids_h.shape
    if int(ids_h.min()) < 0 or int(ids_h.max()) >= eng.V:
        raise ValueError(f"text_id[vqa] outside [0, {eng.V})")
    prefix = [int(p) for p in data["prefix_index"]["vqa"]]
    trie = constrain.compile_constraints(constraints, eng.model.tokenizer.eos_id, eng.V)
    plan = plan_vocab(trie, B, prefix, S, n_listed=_listed(constraints, B))
    if plan.R == 0:
        raise ValueError(f"score_vocab: {plan.why_dense}")               # (no table holds such a path: neither route serves it)
    route = route or route_of(plan)
    if route == "tree" and not plan.tree:
        raise ValueError(f"score_vocab: this batch cannot take the tree route ({plan.why_dense})")
    vs_list = [int(v) for v in data["video_start"]["vqa"]]
    fn = _tree if route == "tree" else _dense
    by_mean = float(length_penalty) == 1.0
    out = fn(eng, data, ids_h, vs_list, prefix, plan, events, int(top), by_mean)
    out.update(route=route, plan=plan)
    if twin is not None:
        blind = dict(data)
        blind.update(twin)
        ob = fn(eng, blind, ids_h, vs_list, prefix, plan, events, int(top), by_mean)
        key = "mean" if by_mean else "logprob_sum"
        out.update(mean_blind=ob["mean"], prediction_blind=ob["prediction"], prediction_plain=out["prediction"],
                   prediction=score.contrast_pick(-out[key], -ob[key], out["count"], contrast_alpha))
    return out
