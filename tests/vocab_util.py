"""Helpers of the answer-vocabulary scoring tests (tests/test_vocab_cpu.py, tests/test_vocab_gpu.py), built on the CPU only:
member sets with a wanted number of rows, a brute-force walk of a trie to hold fvqa.vocab.plan_vocab against, the fp64 restatement
of fvqa_trie_score's rule, and inputs and fp64 references for fvqa_attn_suffix_tree (tests/cached_attn_util.py's one_row_ref, with
keys = the cache rows and then the row's ancestors)."""
import math
import os

import numpy as np
import torch

from fvqa import constrain, vocab
from tests import cached_attn_util as U

EOS, V = 2, 512
FP32_RTOL = 1e-3                      # the project's bar for an fp32 build against the reference
# The error of the PARENT's dense teacher-forced pass (score_options' dense route on the members written out as options) on the
# fixtures' means, relative; the 16-bit bound of the end-to-end tests is 4 x this (the margin tests/test_flipped_gpu.py gives the
# shared route). The figure is tests/test_vocab_gpu.py's scale_err — the largest |difference| of a sample's means over the sample's
# largest |mean| —, measured on an MI355X (profiles/score_vocab.log, "errors"), rounded up in the third digit; the fp32 build
# gives 7.1e-7 and 7.3e-7 by the same figure. test_the_parents_dense_error_is_what_the_constants_say measures it again.
DENSE_MEAN_ERR = {
    "vocab_tiny": {torch.bfloat16: 9.43e-4, torch.float16: 6.65e-5},                 # measured 9.4297e-04, 6.6427e-05
    "vocab_7b_l2_peakedperm": {torch.bfloat16: 8.44e-4, torch.float16: 2.88e-5},     # measured 8.4334e-04, 2.8724e-05
}


# ------------------------------------------------------------------------------------------------ the reference's fixtures
FIXTURES = ("vocab_tiny", "vocab_7b_l2_peakedperm")
MODEL_OF = {"vocab_tiny": "tiny_peakedperm", "vocab_7b_l2_peakedperm": "7b_l2_peakedperm"}      # tests/test_generate_gpu.model_of


def load(name):
    return dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name + ".npz")))


def fixture_sets(g):
    """The member lists as the generator wrote them, one per sample (duplicates included)."""
    return [[g["members"][b, m, :g["member_len"][b, m]].tolist() for m in range(int(g["n_listed"][b]))]
            for b in range(g["members"].shape[0])]


def fixture_batch(g, blind=False):
    """The prompt batch, as generate.prompt_batch makes one."""
    ids = torch.from_numpy(g["text_id_vqa"])
    prefix = g["prefix_vqa"].tolist()
    label = torch.zeros_like(ids)
    for b, p in enumerate(prefix):
        label[b, 0, p] = 1
    video = torch.from_numpy(g["video"])
    return {"video": torch.zeros_like(video) if blind else video, "text_id": {"vqa": ids}, "label": {"vqa": label},
            "video_start": {"vqa": g["vstart_vqa"].tolist()}, "prefix_index": {"vqa": prefix}, "vid": [None] * len(prefix)}


def first_columns(g):
    """(B, M) bool: the columns score_vocab fills — the first copy of every distinct member."""
    sets = fixture_sets(g)
    out = np.zeros(g["mean"].shape, dtype=bool)
    for b, s in enumerate(sets):
        seen = set()
        for m, seq in enumerate(s):
            if tuple(seq) not in seen:
                seen.add(tuple(seq))
                out[b, m] = True
    return out


def option_batch(g):
    """The members written out as the answer options of a multiple-choice batch, (B, M, S) ids and labels — what the PARENT's
    dense teacher-forced pass (score.score_options(route="dense")) scores; a sample with a shorter list repeats its member 0."""
    b = fixture_batch(g)
    sets = fixture_sets(g)
    B, _, S = b["text_id"]["vqa"].shape
    M = g["mean"].shape[1]
    ids = b["text_id"]["vqa"].repeat(1, M, 1)
    lab = torch.zeros_like(ids)
    for n, s in enumerate(sets):
        p = b["prefix_index"]["vqa"][n]
        for m in range(M):
            seq = torch.tensor(list(s[m] if m < len(s) else s[0]) + [EOS])
            ids[n, m, p:p + len(seq)] = seq
            lab[n, m, p:p + len(seq)] = seq
    b["text_id"], b["label"] = {"vqa": ids}, {"vqa": lab}
    return b


def rel_err(got, want, mask):
    got, want = np.asarray(got, dtype=np.float64)[mask], np.asarray(want, dtype=np.float64)[mask]
    return float((np.abs(got - want) / np.abs(want)).max())


# ------------------------------------------------------------------------------------------------ member sets
def random_members(n_rows, seed, max_depth=31, extra_prefix_members=0.3):
    """A member set whose trie has exactly n_rows internal nodes: a random tree of n_rows nodes (node i > 0 hangs under a random
    earlier node of depth < max_depth, its edge token is 3 + i), every leaf of it is a member, and so is some of the inner nodes
    (a member that is a proper prefix of another). Shuffled, with one duplicate when there is more than one member."""
    g = np.random.default_rng(seed)
    parent, depth = [-1], [0]
    for i in range(1, n_rows):
        ok = [j for j in range(i) if depth[j] < max_depth]
        p = int(g.choice(ok))
        parent.append(p)
        depth.append(depth[p] + 1)
    kids = [0] * n_rows
    for p in parent[1:]:
        kids[p] += 1

    def path(i):
        out = []
        while i > 0:
            out.append(3 + i)
            i = parent[i]
        return out[::-1]
    members = [path(i) for i in range(n_rows) if kids[i] == 0 or g.random() < extra_prefix_members]
    order = g.permutation(len(members))
    members = [members[i] for i in order]
    if len(members) > 1:
        members.append(list(members[0]))
    return members


def chain_members(depth):
    """One member of `depth` tokens: rows 0..depth, a chain."""
    return [[3 + i for i in range(depth)]]


def crossing_members():
    """46 rows: the root, a chain of five down to X (row 5), under X a bushy subtree of 30 rows (rows 6..35: it runs over the tile
    edge at row 32) and BEHIND it X's other child with a chain of ten (rows 36..45, all in tile 1). The chain of tile 1's first
    row (32, inside the subtree) holds X's ancestors, X, and subtree rows that are NO ancestors of rows 36..45."""
    stem = [10, 11, 12, 13, 14]
    sub = [stem + [20] + m for m in random_members(30, 5, max_depth=8)]
    tail = [stem + [30] + [40 + i for i in range(9)]]
    return sub + tail


def trie_of(members):
    return constrain.TokenTrie.from_sequences(members, EOS, V)


# ------------------------------------------------------------------------------------------------ brute force over a trie
def brute(trie, b, B):
    """Sample b's rows by a recursive walk of the CSR arrays, nothing shared with plan_vocab: dict(token, depth, parent, end
    (lists, pre-order), anc (per row the set of its ancestors-or-self), edges [(parent row, token, child row or -1)], members
    {lowest index: [edge indices]})."""
    h = trie.host()
    root = int(h.roots(B)[b])
    rows = dict(token=[], depth=[], parent=[], end=[], anc=[], edges=[], members={})

    def walk(v, tok, par, d, path):
        r = len(rows["token"])
        rows["token"].append(tok)
        rows["depth"].append(d)
        rows["parent"].append(par)
        rows["end"].append(None)
        rows["anc"].append(({r} | rows["anc"][par]) if par >= 0 else {r})
        toks, kids = h.children(v)
        first = len(rows["edges"])
        for t in toks:
            rows["edges"].append([r, int(t), -1])
        for i, (t, c) in enumerate(zip(toks.tolist(), kids.tolist())):
            e = first + i
            if len(h.children(c)[0]):
                rows["edges"][e][2] = len(rows["token"])
                walk(c, t, r, d + 1, path + [e])
            else:
                rows["members"][h.leaf_choice[c]] = path + [e]
        rows["end"][r] = len(rows["token"])
    walk(root, -1, -1, 0, [])
    return rows


# ------------------------------------------------------------------------------------------------ fvqa_trie_score in fp64
def in_front(ka, a, kb, b):
    if math.isnan(ka) != math.isnan(kb):
        return math.isnan(ka)
    if not math.isnan(ka) and ka != kb:
        return ka > kb
    return a < b


def score_ref(plan, edge_lp, top, by_mean):
    """include/fvqa.h fvqa_trie_score, members step, in fp64 numpy. edge_lp (B, E). -> dict of numpy arrays, and `gap` (B,): the
    distance between the keys of the first and the second of the ranking (inf with one member, nan if either is nan)."""
    B, M = plan.B, plan.M
    lp = np.asarray(edge_lp, dtype=np.float64)
    out = dict(logprob_sum=np.full((B, M), -np.inf), mean=np.full((B, M), -np.inf), log_posterior=np.full((B, M), -np.inf),
               count=np.zeros((B, M), dtype=np.int64), ranking=np.full((B, top), -1, dtype=np.int64),
               prediction=np.zeros(B, dtype=np.int64), gap=np.full(B, np.inf), keys=[])
    for b in range(B):
        nm = int(plan.n_members[b])
        sums, keys, cols = [], [], []
        for m in range(nm):
            ln = int(plan.member_len[b, m])
            s = 0.0
            for e in plan.member_path[b, m, :ln]:
                s += lp[b, e]
            c = int(plan.member_index[b, m])
            sums.append(s)
            keys.append(s / ln if by_mean else s)
            cols.append(c)
            out["logprob_sum"][b, c], out["mean"][b, c], out["count"][b, c] = s, s / ln, ln
        sums = np.asarray(sums)
        with np.errstate(all="ignore"):
            mx = np.nanmax(sums) if not np.isnan(sums).all() else -np.inf
            lz = mx + np.log(np.exp(sums - mx).sum())
        for m in range(nm):
            out["log_posterior"][b, cols[m]] = sums[m] - lz
        order = []
        for m in range(nm):
            at = 0
            while at < len(order) and not in_front(keys[m], m, keys[order[at]], order[at]):
                at += 1
            order.insert(at, m)
        for r, m in enumerate(order[:top]):
            out["ranking"][b, r] = cols[m]
        out["prediction"][b] = cols[order[0]]
        if nm > 1:
            out["gap"][b] = keys[order[0]] - keys[order[1]]
        out["keys"].append({cols[m]: keys[m] for m in range(nm)})
    return out


# ------------------------------------------------------------------------------------------------ fvqa_attn_suffix_tree
DEFECTS = ("sibling", "descendant", "no_chain", "row_position")


def tree_case(dtype, cache_rotated, member_sets, start, vstart, S=160, H=2, A=10, F=10, seed=0, plant=None):
    """N = len(member_sets) samples of length S; sample n's rows are the internal nodes of trie_of(member_sets[n]) (planned per
    sample: R = the largest count), row r at position start[n] + depth[r] against the cache rows [0, start[n]). The cache rows
    from start[n] on and the padding rows of qkv_suf are NaN. want (N * R, D) fp64 by one_row_ref, valid (N * R,).
    plant = (n, q, key row, sibling row, descendant row): the query q of sample n gets a planted key on `key row` (an ancestor,
    score 16) and decoys (score 30) on a sibling's and a descendant's row."""
    N, D = len(member_sets), H * U.DH
    plan = vocab.plan_vocab(trie_of(member_sets), N, [s + 1 for s in start], S)
    R = plan.R
    base = U.rnd(N * S + A, 3 * D, dtype=dtype, seed=seed)
    own = U.rnd(N * R, 3 * D, dtype=dtype, seed=seed + 3)
    g1, g2 = U.gates(H, seed)
    cos, sin, c64, s64 = U.tables(S)
    pos = torch.as_tensor(start, dtype=torch.int64)[:, None] + torch.as_tensor(plan.depth.astype(np.int64))          # (N, R)
    o5 = own.view(N, R, 3, H, U.DH)
    q, k, v = o5[:, :, 0], o5[:, :, 1], o5[:, :, 2]                        # views: a planted raw key lands in `own`
    if plant is not None:
        n, qr, key_row, sib, desc = plant
        qhat = U.rot_rows(q[n, qr].double(), int(pos[n, qr]), c64, s64).to(dtype).double()
        for r, score in ((key_row, U.PLANT), (sib, U.DECOY), (desc, U.DECOY)):
            k[n, r] = U.rot_rows(U.planted(qhat, score), int(pos[n, r]), c64, s64, inverse=True).to(dtype)
    ck = base[: N * S].view(N, S, 3, H, U.DH)[:, :, 1]
    ckr = U.rotated_rounded(ck, c64, s64, dtype)                           # the prompt's keys as the prefill holds them
    cv = base[: N * S].view(N, S, 3, H, U.DH)[:, :, 2].double()
    ak = base[N * S:, D:2 * D].double().view(A, H, U.DH)
    av = base[N * S:, 2 * D:].double().view(A, H, U.DH)
    cache = base.clone()
    if cache_rotated:
        cache[: N * S].view(N, S, 3, H, U.DH)[:, :, 1] = ckr.to(dtype)
    for n in range(N):
        cache[n * S + start[n]:(n + 1) * S] = U.NAN
    suf = own.clone().view(N, R, 3 * D)
    valid = torch.zeros(N, R, dtype=torch.bool)
    for n in range(N):
        suf[n, plan.n_rows[n]:] = U.NAN
        valid[n, :plan.n_rows[n]] = True
    case = dict(plan=plan, suf=suf.reshape(N * R, 3 * D), cache=cache, g1=g1, g2=g2, cos=cos, sin=sin, valid=valid.reshape(-1),
                vstart=torch.tensor(vstart, dtype=torch.int32), start=torch.tensor(start, dtype=torch.int32), N=N, R=R, S=S, H=H,
                A=A, F=F, D=D, dtype=dtype, _ref=dict(q=q, k=k, v=v, ckr=ckr, cv=cv, ak=ak, av=av, c64=c64, s64=s64, pos=pos))
    want = torch.zeros(N, R, D, dtype=torch.float64)
    for n in range(N):
        for r in range(int(plan.n_rows[n])):
            want[n, r] = tree_row_ref(case, n, r)[0]
    case["want"] = want.reshape(N * R, D)
    return case


def tree_row_ref(case, n, r, defect=None):
    """Row r of sample n in fp64 -> (o (D,), the text weights (H, keys)). The keys are the cache rows [0, start) and then the row's
    ancestors, root first, the row itself last, each rotated at start + its depth and rounded. defect (None: the contract):
      "sibling"       the rows with r's parent are keys as well;   "descendant"  so are r's children;
      "no_chain"      the ancestors in front of r's tile are dropped;
      "row_position"  every suffix row sits at start + its row INDEX."""
    plan, f = case["plan"], case["_ref"]
    dtype, st, vs = case["dtype"], int(case["start"][n]), int(case["vstart"][n])
    parent = plan.parent[n]
    keys, a = [], r
    while a >= 0:
        keys.append(int(a))
        a = parent[a]
    keys = keys[::-1]
    nr = int(plan.n_rows[n])
    if defect == "sibling":
        keys = sorted(set(keys) | {x for x in range(nr) if parent[x] == parent[r] and r > 0})
    elif defect == "descendant":
        keys = sorted(set(keys) | {x for x in range(nr) if parent[x] == r})
    elif defect == "no_chain":
        keys = [x for x in keys if x >= (r // 32) * 32]
    where = (lambda x: st + x) if defect == "row_position" else (lambda x: int(f["pos"][n, x]))
    rot = lambda t, p: U.rot_rows(t.double(), min(p, case["S"] - 1), f["c64"], f["s64"]).to(dtype).double()   # noqa: E731
    qhat = rot(f["q"][n, r], where(r))
    kr = torch.cat([f["ckr"][n, :st]] + [rot(f["k"][n, x], where(x))[None] for x in keys])
    vv = torch.cat([f["cv"][n, :st]] + [f["v"][n, x].double()[None] for x in keys])
    # one_row_ref's row p sees keys 0..p and applies gate2 when p >= vs + F: the keys behind the cache sit at positions start +
    # depth, one per position along a chain, so with the contract's keys p = start + depth[r] = the last key's index
    p = kr.shape[0] - 1
    if defect is None:
        assert p == where(r)
    o, pt = one_row(qhat, kr, vv, f["ak"], f["av"], case["g1"].double(), case["g2"].double(), vs, case["F"], where(r),
                    [*range(st)] + [where(x) for x in keys])
    return o.reshape(-1), pt


def one_row(qhat, kr, v, ak, av, g1, g2, vs, F, p, kpos):
    """cached_attn_util.one_row_ref for keys at the positions kpos (a list; the contract's keys are at 0..p and this IS
    one_row_ref — asserted by the callers' tests; a defect's keys may share a position or skip one)."""
    if kpos == list(range(p + 1)):
        return U.one_row_ref(qhat, kr, v, ak, av, g1, g2, vs, F, p)
    sc = 1.0 / math.sqrt(U.DH)
    s_a = torch.einsum("hd,ahd->ha", qhat, ak) * sc
    s_t = torch.einsum("hd,thd->ht", qhat, kr) * sc
    if vs >= 0 and p >= vs + F:
        win = torch.as_tensor([vs <= x < vs + F for x in kpos])
        s_t[:, win] += g2[:, None]
    pa, pt = torch.softmax(s_a, -1), torch.softmax(s_t, -1)
    return torch.tanh(g1)[:, None] * torch.einsum("ha,ahd->hd", pa, av) + torch.einsum("ht,thd->hd", pt, v), pt
