"""Answer-vocabulary scoring without a GPU: fvqa.vocab.plan_vocab against a brute-force walk of the trie, the two facts about
pre-order numbering the tree attention rests on, every refusal (planner, parser, operand checks), the fp64 restatement of
fvqa_trie_score's rule on hand-made numbers, the dense route's host integers and the fixtures' own premises."""
import math
import types

import numpy as np
import pytest
import torch

import engine
import train
from fvqa import constrain, ops, vocab
from tests import vocab_util as VU


def plan_of(sets, B, **kw):
    return vocab.plan_vocab(VU.trie_of(sets), B, **kw)


SETS = {
    "mixed": [[5, 6, 7], [5, 6], [5], [9], [], [5, 6, 7], [5, 8, 3, 4]],          # prefixes, one-token, empty, a duplicate
    "empty_only": [[]],
    "rows65": VU.random_members(65, 4, max_depth=12),
    "crossing": VU.crossing_members(),
    "deep": VU.chain_members(31),
}


# ------------------------------------------------------------------------------------------------ the plan against brute force
@pytest.mark.parametrize("name", sorted(SETS))
def test_plan_is_the_brute_force_walk(name):
    sets = SETS[name]
    trie = VU.trie_of(sets)
    p = vocab.plan_vocab(trie, 2)
    want = VU.brute(trie, 0, 2)
    n = len(want["token"])
    assert p.shared and list(p.n_rows) == [n, n] and p.R == n and p.tree
    for b in range(2):                                                          # a shared trie: planned once, repeated
        assert p.token[b].tolist() == want["token"] and p.depth[b].tolist() == want["depth"]
        assert p.parent[b].tolist() == want["parent"] and p.end[b].tolist() == want["end"]
        ne = len(want["edges"])
        assert int(p.n_edges[b]) == ne
        got_edges = list(zip(p.edge_parent[b, :ne].tolist(), p.edge_token[b, :ne].tolist(), p.edge_child[b, :ne].tolist()))
        assert got_edges == [tuple(e) for e in want["edges"]]
        cols = sorted(want["members"])
        assert p.member_index[b, :p.n_members[b]].tolist() == cols              # ascending; duplicates at their lowest index
        for m, c in enumerate(cols):
            path = want["members"][c]
            assert p.member_path[b, m, :len(path)].tolist() == path and (p.member_path[b, m, len(path):] == -1).all()
            assert int(p.member_len[b, m]) == len(path) == len(sets[c]) + 1 and int(p.member_edge[b, m]) == path[-1]
            assert p.members(b)[m] == list(sets[c]) + [VU.EOS]
        for t in range((n + 31) // 32):
            chain = sorted(want["anc"][32 * t] - {32 * t})
            assert p.tile_anc[b, t, :len(chain)].tolist() == chain and (p.tile_anc[b, t, len(chain):] == -1).all()
    assert p.M == max(want["members"]) + 1                                      # without n_listed: the highest index + 1


def test_duplicates_the_empty_member_and_a_prefix_member():
    p = plan_of(SETS["mixed"], 1, n_listed=7)
    assert p.M == 7 and int(p.n_members[0]) == 6 and p.member_index[0, :6].tolist() == [0, 1, 2, 3, 4, 6]      # 5 = a copy of 0
    members = p.members(0)
    assert members[4] == [VU.EOS] and int(p.member_len[0, 4]) == 1              # the empty member: the root's EOS edge alone
    e = int(p.member_edge[0, 4])
    assert int(p.member_path[0, 4, 0]) == e and int(p.edge_parent[0, e]) == 0 and int(p.edge_token[0, e]) == VU.EOS
    assert members[1] == members[0][:2] + [VU.EOS]                              # [5, 6] ends where [5, 6, 7] goes on
    assert p.member_path[0, 1, :2].tolist() == p.member_path[0, 0, :2].tolist()
    with pytest.raises(ValueError):
        plan_of(SETS["mixed"], 1, n_listed=6)                                   # does not cover index 6


def test_per_sample_tries_are_padded_to_the_largest():
    sets = [SETS["mixed"], SETS["empty_only"], SETS["rows65"]]
    p = plan_of(sets, 3)
    assert not p.shared and list(p.n_rows) == [8, 1, 65] and p.R == 65           # mixed: root, 5, 56, 567, 58, 583, 5834, 9
    for b, s in enumerate(sets):
        one = plan_of(s, 1)
        n, ne, nm = int(one.n_rows[0]), int(one.n_edges[0]), int(one.n_members[0])
        for k in ("token", "depth", "end", "parent"):
            assert np.array_equal(getattr(p, k)[b, :n], getattr(one, k)[0]), k
        assert (p.token[b, n:] == 0).all() and (p.depth[b, n:] == 0).all() and (p.end[b, n:] == np.arange(n + 1, 66)).all()
        assert np.array_equal(p.edge_parent[b, :ne], one.edge_parent[0]) and np.array_equal(p.edge_token[b, :ne], one.edge_token[0])
        assert np.array_equal(p.member_path[b, :nm], one.member_path[0]) and int(p.n_members[b]) == nm
        assert np.array_equal(p.tile_anc[b, :one.tile_anc.shape[1]], one.tile_anc[0]) and (p.tile_anc[b, one.tile_anc.shape[1]:] == -1).all()
    shared, one = plan_of(SETS["mixed"], 3), plan_of(SETS["mixed"], 1)
    assert shared.shared and shared.R == one.R
    for k in ("token", "depth", "end", "parent", "tile_anc", "edge_parent", "edge_token", "member_path", "member_index"):
        for b in range(3):
            assert np.array_equal(getattr(shared, k)[b], getattr(one, k)[0]), k


@pytest.mark.parametrize("seed", range(12))
def test_the_two_facts_about_pre_order(seed):
    """a is an ancestor-or-self of q iff a <= q < end[a]; and every ancestor of a row of the tile from q0 lies in the tile or is
    an ancestor of q0 — so the tile's keys are tile_anc(q0) and the tile's own rows."""
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, 140))
    sets = VU.random_members(n, 50 + seed, max_depth=int(rng.integers(1, 32)))
    trie = VU.trie_of(sets)
    p, want = vocab.plan_vocab(trie, 1), VU.brute(trie, 0, 1)
    assert int(p.n_rows[0]) == n
    end = p.end[0]
    for q in range(n):
        anc = {a for a in range(n) if a <= q < end[a]}
        assert anc == want["anc"][q]
        q0 = (q // 32) * 32
        chain = {int(a) for a in p.tile_anc[0, q // 32] if a >= 0}
        assert chain == want["anc"][q0] - {q0}
        assert all(a >= q0 or a in chain for a in anc)


# ------------------------------------------------------------------------------------------------ refusals
def test_planner_refusals():
    deep = plan_of(VU.chain_members(32), 1)                                     # rows of depth 0..32
    assert not deep.tree and "32" in deep.why_dense
    assert plan_of(VU.chain_members(31), 1).tree
    with pytest.raises(ValueError, match="does not fit"):
        plan_of(SETS["mixed"], 1, prefix=[60], S=64)                            # 60 + 5 tokens > 64
    assert plan_of(SETS["mixed"], 1, prefix=[59], S=64).tree
    with pytest.raises(ValueError, match="built for 2 samples"):
        plan_of([SETS["mixed"], SETS["empty_only"]], 3)
    with pytest.raises(ValueError, match="prefix"):
        plan_of(SETS["mixed"], 2, prefix=[10], S=64)
    with pytest.raises(ValueError, match="no prompt token"):
        plan_of(SETS["mixed"], 1, prefix=[0], S=64)
    wide = plan_of([[3 + i] for i in range(20)], 1)                             # twenty one-token members: the root and a row each
    assert wide.tree and wide.R == 21 and int(wide.n_members[0]) == 20 and int(wide.depth.max()) == 1


def test_limits_send_the_whole_batch_dense(monkeypatch):
    sets = SETS["rows65"]
    monkeypatch.setattr(ops, "TREE_ROWS_MAX", 64)
    p = plan_of(sets, 2)
    assert not p.tree and "65 rows" in p.why_dense and vocab.route_of(p) == "dense"
    monkeypatch.setattr(ops, "TREE_ROWS_MAX", 4096)
    monkeypatch.setattr(ops, "TREE_TOTAL_ROWS_MAX", 129)
    assert not plan_of(sets, 2).tree and plan_of(sets, 1).tree
    monkeypatch.setattr(ops, "TREE_TOTAL_ROWS_MAX", 65536)
    p = plan_of(sets, 2)
    assert vocab.route_of(p) == "tree"
    monkeypatch.setenv("FVQA_SCORE_VOCAB", "dense")
    assert vocab.route_of(p) == "dense"
    monkeypatch.setenv("FVQA_SCORE_VOCAB", "fast")
    with pytest.raises(ValueError):
        vocab.route_of(p)


def test_the_limits_are_the_headers():
    import os
    import re
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fvqa.h")).read()
    macro = lambda n: int(re.search(rf"#define {n} (\d+)", text).group(1))     # noqa: E731
    assert (ops.TREE_DEPTH_MAX, ops.TREE_ROWS_MAX, ops.TREE_TOTAL_ROWS_MAX) == (
        macro("FVQA_TREE_DEPTH_MAX"), macro("FVQA_TREE_ROWS_MAX"), macro("FVQA_TREE_TOTAL_ROWS_MAX"))
    assert ops.TREE_DEPTH_MAX + 1 == ops.TREE_TILE == vocab.PATH


def test_score_vocab_refuses_before_any_launch(monkeypatch):
    eng = types.SimpleNamespace(V=VU.V, model=types.SimpleNamespace(tokenizer=types.SimpleNamespace(eos_id=VU.EOS)))
    ids = torch.ones(2, 1, 64, dtype=torch.int64)
    data = {"text_id": {"vqa": ids}, "video_start": {"vqa": [0, 0]}, "prefix_index": {"vqa": [10, 12]}}
    for kw, msg in ((dict(length_penalty=0.5), "length_penalty"), (dict(top=9), "top"), (dict(route="shared"), "route"),
                    (dict(contrast="blind"), "video")):
        with pytest.raises(ValueError, match=msg):
            vocab.score_vocab(eng, data, SETS["mixed"], **kw)
    with pytest.raises(ValueError, match="prefix_index"):
        vocab.score_vocab(eng, {"text_id": {"vqa": ids}}, SETS["mixed"])
    with pytest.raises(ValueError, match="built for 3 samples"):
        vocab.score_vocab(eng, data, [SETS["mixed"]] * 3)
    with pytest.raises(ValueError, match="does not fit"):
        vocab.score_vocab(eng, dict(data, prefix_index={"vqa": [10, 61]}), SETS["mixed"])
    with pytest.raises(ValueError, match="32"):
        vocab.score_vocab(eng, data, VU.chain_members(32))                      # a row of depth 32: no table holds its path
    monkeypatch.setattr(ops, "TREE_ROWS_MAX", 2)
    with pytest.raises(ValueError, match="tree route"):
        vocab.score_vocab(eng, data, SETS["mixed"], route="tree")               # the planner turned it down: dense or nothing


PARSER_CONFLICTS = [
    ["--val_vocab"], ["--val_vocab", "--answer_vocab", "f.txt"], ["--val_vocab", "--is_generation_task"],
    ["--val_vocab", "--answer_vocab", "f.txt", "--is_generation_task", "--num_beams", "2"],
    ["--val_vocab", "--answer_vocab", "f.txt", "--is_generation_task", "--lookahead", "4"],
    ["--val_vocab", "--answer_vocab", "f.txt", "--is_generation_task", "--gen_constrain", "vocab", "--gen_jump_forward", "4"],
    ["--val_vocab", "--answer_vocab", "f.txt", "--is_generation_task", "--gen_stream", "4"],
    ["--val_vocab", "--answer_vocab", "f.txt", "--is_generation_task", "--gen_stop_eos", "--gen_frame_attention"],
]


@pytest.mark.parametrize("argv", PARSER_CONFLICTS)
def test_parser_conflicts(argv, capsys):
    with pytest.raises(SystemExit):
        train.get_args_parser().parse_args(argv)
    assert "--val_vocab" in capsys.readouterr().err


def test_parser_accepts_the_flag():
    a = train.get_args_parser().parse_args(["--val_vocab", "--answer_vocab", "f.txt", "--is_generation_task", "--contrast", "blind"])
    assert a.val_vocab and a.answer_vocab == "f.txt"
    assert not train.get_args_parser().parse_args([]).val_vocab


def tree_operands(R=33, n_seq=2, S=64, H=2, A=10, dtype=torch.float32):
    D = H * 128
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32)                         # noqa: E731
    return dict(qkv_suf=torch.zeros(n_seq * R, 3 * D, dtype=dtype), qkv_cache=torch.zeros(n_seq * S + A, 3 * D, dtype=dtype),
                o_suf=torch.zeros(n_seq * R, D, dtype=dtype), gate1=torch.zeros(H), gate2=torch.zeros(H), vstart=i32(n_seq),
                start=i32(n_seq), n_rows=i32(n_seq), depth=i32(n_seq * R), end=i32(n_seq * R),
                tile_anc=i32(n_seq * ((R + 31) // 32) * 32))


def call_tree(t, R=33, n_seq=2, S=64, H=2, A=10, F=10, Dh=128, rope="ok"):
    if rope == "ok":
        rope = (torch.zeros(S, 64), torch.zeros(S, 64))
    return ops.attn_suffix_tree(t["qkv_suf"], t["qkv_cache"], t["o_suf"], t["gate1"], t["gate2"], t["vstart"], t["start"],
                                t["n_rows"], t["depth"], t["end"], t["tile_anc"], rope, n_seq, R, S, H, Dh, A, F, cache_rotated=True)


def test_tree_attention_operand_checks_need_no_device():
    with pytest.raises(ValueError, match="device tensors"):                     # every shape right: the device check is the last
        call_tree(tree_operands())
    bad = [
        (dict(depth=torch.zeros(65, dtype=torch.int32)), {}, "depth"),
        (dict(end=torch.zeros(66, dtype=torch.int64)), {}, "end"),
        (dict(tile_anc=torch.zeros(2 * 33, dtype=torch.int32)), {}, "tile_anc"),
        (dict(n_rows=torch.zeros(3, dtype=torch.int32)), {}, "n_rows"),
        (dict(start=torch.zeros(2, dtype=torch.int64)), {}, "start"),
        (dict(gate1=torch.zeros(3)), {}, "gate1"),
        (dict(o_suf=torch.zeros(66, 128)), {}, "row shapes"),
        (dict(qkv_suf=torch.zeros(65, 768)), {}, "row shapes"),
        (dict(qkv_cache=torch.zeros(2 * 64, 768)), {}, "qkv_cache"),
        (dict(o_suf=torch.zeros(66, 256, dtype=torch.bfloat16)), {}, "dtype"),
        ({}, dict(Dh=64), "head_dim"),
        ({}, dict(A=17), "adapter_len"),
        ({}, dict(S=4097), "seq_len"),
        ({}, dict(R=0), "rows per sample"),
        ({}, dict(R=ops.TREE_ROWS_MAX + 1), "rows per sample"),
        ({}, dict(R=33, n_seq=ops.TREE_TOTAL_ROWS_MAX // 33 + 1), "rows per sample"),
    ]
    for over, kw, msg in bad:
        t = tree_operands()
        t.update(over)
        with pytest.raises(ValueError, match=msg):
            call_tree(t, **kw)
    t = tree_operands()
    t["qkv_suf"] = torch.zeros(66 * 768 + 1)[1:].view(66, 768)                  # 4 bytes off a 16-byte boundary
    with pytest.raises(ValueError, match="16-byte"):
        call_tree(t)


def test_trie_score_operand_checks_need_no_device():
    p = plan_of(SETS["mixed"], 2)
    t = {k: torch.as_tensor(getattr(p, k)) for k in ("edge_parent", "edge_token", "n_edges", "member_path", "member_len",
                                                     "member_index", "n_members")}
    lp = torch.zeros(2, p.E)
    with pytest.raises(ValueError, match="device tensors"):
        ops.trie_score(t, lp, 2, p.R, 64, reduce=True, n_columns=p.M, top=3)
    for kw, msg in ((dict(reduce=True, n_columns=p.M, top=9), "top"), (dict(), "nothing to do"),
                    (dict(logits=torch.zeros(4, 64), lse=torch.zeros(4), row0=2 * p.R - 3, n_block_rows=4), "block inside")):
        with pytest.raises(ValueError, match=msg):
            ops.trie_score(t, lp, 2, p.R, 64, **kw)
    with pytest.raises(ValueError, match="edge_lp"):
        ops.trie_score(t, torch.zeros(2, p.E + 1), 2, p.R, 64, reduce=True, n_columns=p.M)
    with pytest.raises(ValueError, match="member_path"):
        ops.trie_score(dict(t, member_path=t["member_path"][:, :, :31]), lp, 2, p.R, 64, reduce=True, n_columns=p.M)


# ------------------------------------------------------------------------------------------------ the rule of fvqa_trie_score
def hand_plan():
    """members 0: [5, 6], 1: [5], 2: [9], 3: [] (EOS alone), 4: [5, 6] again."""
    return plan_of([[5, 6], [5], [9], [], [5, 6]], 1, n_listed=5)


def hand_lp(p, values):
    """edge_lp from {(parent row, token): log-probability}."""
    lp = np.zeros((1, p.E))
    for e in range(int(p.n_edges[0])):
        lp[0, e] = values[(int(p.edge_parent[0, e]), int(p.edge_token[0, e]))]
    return lp


def test_score_rule_on_hand_made_numbers():
    p = hand_plan()
    # rows: 0 root, 1 = [5], 2 = [5, 6], 3 = [9]
    assert p.token[0].tolist() == [-1, 5, 6, 9]
    v = {(0, 2): math.log(0.1), (0, 5): math.log(0.6), (0, 9): math.log(0.3), (1, 2): math.log(0.5), (1, 6): math.log(0.5),
         (2, 2): math.log(1.0), (3, 2): math.log(0.2)}
    r = VU.score_ref(p, hand_lp(p, v), top=3, by_mean=False)
    want = {0: 0.6 * 0.5 * 1.0, 1: 0.6 * 0.5, 2: 0.3 * 0.2, 3: 0.1}
    for c, pr in want.items():
        assert math.isclose(r["logprob_sum"][0, c], math.log(pr), rel_tol=1e-12)
    assert r["count"][0].tolist() == [3, 2, 2, 1, 0] and np.isneginf(r["logprob_sum"][0, 4]) and np.isneginf(r["log_posterior"][0, 4])
    z = sum(want.values())
    assert math.isclose(r["log_posterior"][0, 2], math.log(0.06 / z), rel_tol=1e-12)
    assert r["ranking"][0].tolist() == [0, 1, 3] and r["prediction"][0] == 0    # sums 0.3 = 0.3 (a tie: the lower index), 0.1, 0.06
    m = VU.score_ref(p, hand_lp(p, v), top=5, by_mean=True)
    means = {c: math.log(pr) / n for (c, pr), n in zip(want.items(), (3, 2, 2, 1))}
    order = sorted(means, key=lambda c: (-means[c], c))
    assert m["ranking"][0].tolist() == order + [-1] and m["prediction"][0] == order[0] == 0
    assert math.isclose(m["gap"][0], means[order[0]] - means[order[1]], rel_tol=1e-12)


def test_score_rule_ties_and_nan():
    p = hand_plan()
    flat = {k: -1.0 for k in ((0, 2), (0, 5), (0, 9), (1, 2), (1, 6), (2, 2), (3, 2))}
    r = VU.score_ref(p, hand_lp(p, flat), top=4, by_mean=True)                  # every mean is -1: ascending columns
    assert r["ranking"][0].tolist() == [0, 1, 2, 3] and r["gap"][0] == 0
    r = VU.score_ref(p, hand_lp(p, flat), top=2, by_mean=False)                 # sums -1 (col 3), -2, -2, -3
    assert r["ranking"][0].tolist() == [3, 1]
    nan = dict(flat)
    nan[(1, 2)] = float("nan")                                                  # the EOS behind [5]: member 1 alone
    r = VU.score_ref(p, hand_lp(p, nan), top=3, by_mean=True)
    assert r["ranking"][0].tolist() == [1, 0, 2] and r["prediction"][0] == 1    # torch's rule: a NaN beats every number
    assert np.isnan(r["log_posterior"][0, :4]).all() and np.isneginf(r["log_posterior"][0, 4])
    nan[(0, 9)] = float("nan")                                                  # two NaNs: the lower column first
    assert VU.score_ref(p, hand_lp(p, nan), top=3, by_mean=False)["ranking"][0].tolist() == [1, 2, 3]


# ------------------------------------------------------------------------------------------------ the dense route's integers
def test_dense_rows_write_each_member_behind_its_prompt():
    sets = [SETS["mixed"], [[9, 9, 9]]]
    p = plan_of(sets, 2, prefix=[10, 12], S=32)
    ids_h = torch.arange(2 * 32).view(2, 1, 32) + 100
    ids, lab, (tb, te, tc, tt) = vocab.dense_rows(p, ids_h, [10, 12], 0, p.MU)
    assert tuple(ids.shape) == (2, p.MU, 32)
    for b, pre in enumerate((10, 12)):
        members = p.members(b)
        for c in range(p.MU):
            seq = members[c] if c < len(members) else members[0]
            assert ids[b, c, :pre].tolist() == ids_h[b, 0, :pre].tolist()
            assert ids[b, c, pre:pre + len(seq)].tolist() == seq and not ids[b, c, pre + len(seq):].any()
            assert lab[b, c, pre:pre + len(seq)].tolist() == seq and int((lab[b, c] != 0).sum()) == len(seq)
    seen = sorted(zip(tb.tolist(), te.tolist()))
    assert seen == [(b, e) for b in range(2) for e in range(int(p.n_edges[b]))]                         # every edge once
    for b, e, c, t in zip(tb.tolist(), te.tolist(), tc.tolist(), tt.tolist()):
        pre = (10, 12)[b]
        assert int(lab[b, c, t + 1]) == int(p.edge_token[b, e]) and t == pre - 1 + int(p.depth[b, p.edge_parent[b, e]])
    with pytest.raises(ValueError, match="token 0"):
        q = plan_of([[0, 5]], 1)
        vocab.dense_rows(q, ids_h[:1], [10], 0, 1)


def test_vocab_gold_reads_the_batchs_answer_text():
    data = {"text": [{"options": ["piano"]}, {"options": ["a", "two", "c"]}, {"options": ["tuba"]}],
            "answer": torch.tensor([0, 1, 0])}
    assert engine.vocab_gold(data, ["one", "two", "piano", "two"]) == [2, 1, -1]


# ------------------------------------------------------------------------------------------------ the fixtures' premises
@pytest.mark.parametrize("name", VU.FIXTURES)
def test_fixture_premises(name):
    g = VU.load(name)
    sets = VU.fixture_sets(g)
    assert len(sets) == 3 and all(v > 0 for d in VU.DENSE_MEAN_ERR.values() for v in d.values())
    p = vocab.plan_vocab(constrain.compile_constraints(sets, VU.EOS, 32000), 3, g["prefix_vqa"].tolist(), 128,
                         n_listed=g["n_listed"].tolist())
    assert p.tree and not p.shared
    cols = VU.first_columns(g)
    for b, s in enumerate(sets):
        assert [] in s and len({tuple(m) for m in s}) < len(s)                                # the empty member, a duplicate
        assert any(len(m) == 1 for m in s)
        assert any(a != c and a[:len(c)] == c and c for a in s for c in s)                    # a proper prefix of another
        assert np.array_equal(g["count"][b, :len(s)], [len(m) + 1 for m in s])
        assert np.allclose(g["token_logprob"][b].sum(-1)[:len(s)], g["logprob_sum"][b, :len(s)], rtol=1e-5, atol=1e-6)
        best = max((m for m in range(len(s)) if cols[b, m]), key=lambda m: (g["mean"][b, m], -m))
        assert best == g["prediction"][b]
    if name == "vocab_tiny":
        assert int(p.n_rows.min()) >= 40 and any(len(m) == 31 for s in sets for m in s)
    worst = max(4 * v for v in VU.DENSE_MEAN_ERR[name].values())
    assert int((g["gap"] > 4 * max(worst, VU.FP32_RTOL)).sum()) >= 3
