"""The vote over the samples of a prompt on the GPU: fvqa_sample_vote against its numpy restatement (tests/test_vote_cpu.py),
exactly, and `generate(vote=True)` end to end."""
import numpy as np
import pytest
import torch

from fvqa import generate, ops
from tests.test_beam_gpu import tiny  # noqa: F401  (the fixture)
from tests.test_generate_gpu import DEV
from tests.test_vote_cpu import vote_rule

pytestmark = pytest.mark.gpu

KEYS = ("group", "votes", "winner", "n_groups", "share")


def vote(tokens, score):
    """One launch on host arrays -> dict of host arrays."""
    out = ops.sample_vote(torch.as_tensor(np.asarray(tokens), dtype=torch.int32, device=DEV).contiguous(),
                          torch.as_tensor(np.asarray(score), dtype=torch.float32, device=DEV).contiguous())
    torch.cuda.synchronize()
    assert set(out) == set(KEYS)
    return {k: v.cpu().numpy() for k, v in out.items()}


def assert_is_the_rule(tokens, score):
    got, want = vote(tokens, score), vote_rule(tokens, score)
    for k in KEYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert np.array_equal(got[k].view(np.uint32) if k == "share" else got[k], want[k].view(np.uint32) if k == "share" else want[k]), k
    return got


@pytest.mark.parametrize("steps", [1, 31])
@pytest.mark.parametrize("n", [1, 2, 5, 64])
@pytest.mark.parametrize("B", [1, 20])
def test_vote_is_the_rule_exactly(B, n, steps):
    """Rows drawn from a few answers per prompt (groups of every size), scores with exact ties and NaNs among them."""
    rng = np.random.default_rng(1000 * B + 10 * n + steps)
    answers = rng.integers(3, 9, (B, 4, steps))
    answers[:, :, steps // 2:][rng.random((B, 4, steps - steps // 2)) < 0.5] = -1
    pick = rng.integers(0, 4, (B, n))
    tokens = np.take_along_axis(answers, pick[:, :, None], 1)
    score = rng.integers(-4, 0, (B, n)).astype(np.float32) / 2           # few values: exact ties
    score[rng.random((B, n)) < 0.1] = np.nan
    got = assert_is_the_rule(tokens, score)
    again = vote(tokens, score)
    for k in KEYS:
        assert np.array_equal(got[k].view(np.uint32) if k == "share" else got[k],
                              again[k].view(np.uint32) if k == "share" else again[k]), k
    assert (got["votes"].sum(1) == n).all() and ((got["votes"] > 0).sum(1) == got["n_groups"]).all()


def test_vote_edges():
    a, b, c = [5, 6, -1], [5, 7, -1], [5, 6, 2]
    # all equal, all distinct, a difference in the padding alone
    r = assert_is_the_rule([[a] * 64], [np.linspace(-3, -1, 64)])
    assert r["winner"][0] == 0 and r["n_groups"][0] == 1 and r["share"][0] == 1.0 and r["votes"][0, 0] == 64
    distinct = np.arange(64 * 3).reshape(1, 64, 3)
    r = assert_is_the_rule(distinct, [np.concatenate([np.linspace(-3, -1, 40), np.linspace(-1.01, -2, 24)])])
    assert r["n_groups"][0] == 64 and r["winner"][0] == 39 and r["share"][0] == np.float32(1) / np.float32(64)
    r = assert_is_the_rule([[[5, 6, -1], [5, 6, 6], [5, 6, -1]]], [[0.0, 0.0, 0.0]])
    assert r["group"][0].tolist() == [0, 1, 0] and r["winner"][0] == 0
    # tied on votes: the representative's score; tied on score too: the lower index; a NaN is -inf
    assert assert_is_the_rule([[a, b, b, a]], [[-2.0, -1.0, -9.0, -0.1]])["winner"][0] == 1
    assert assert_is_the_rule([[a, b, b, a]], [[-1.0, -2.0, -0.1, -9.0]])["winner"][0] == 0
    assert assert_is_the_rule([[a, b, b, a]], [[-1.0, -1.0, 0.0, 0.0]])["winner"][0] == 0
    assert assert_is_the_rule([[b, a, a, b]], [[-1.0, -1.0, 0.0, 0.0]])["winner"][0] == 0
    assert assert_is_the_rule([[a, b, b, a]], [[float("nan"), -50.0, 0.0, 0.0]])["winner"][0] == 1
    assert assert_is_the_rule([[a, b, b, a]], [[-50.0, float("nan"), 0.0, 0.0]])["winner"][0] == 0
    assert assert_is_the_rule([[a, b]], [[float("nan"), float("-inf")]])["winner"][0] == 0
    assert assert_is_the_rule([[a, b, b]], [[0.0, float("nan"), 0.0]])["winner"][0] == 1
    assert assert_is_the_rule([[c, a, b, a, c, c]], [[-1.0, 0.0, 0.0, 0.0, 0.0, 0.0]])["votes"][0].tolist() == [3, 2, 1, 0, 0, 0]


def test_ops_sample_vote_checks_its_tensors():
    tok = torch.zeros(2, 3, 4, dtype=torch.int32, device=DEV)
    sc = torch.zeros(2, 3, device=DEV)
    ops.sample_vote(tok, sc)
    for bad_tok, bad_sc in ((tok.long(), sc), (tok[:, :, :0], sc), (tok, sc.double()), (tok, sc[:, :2].contiguous()), (tok[0], sc),
                            (torch.zeros(1, 65, 2, dtype=torch.int32, device=DEV), torch.zeros(1, 65, device=DEV)),
                            (tok.transpose(1, 2), sc), (tok.cpu(), sc)):
        with pytest.raises(ValueError):
            ops.sample_vote(bad_tok, bad_sc)


# ------------------------------------------------------------------------------------------------ end to end
def rule_on(out):
    """The numpy rule on a result's own tokens, scored by the mean raw log-probability per generated token."""
    lp = out["logprobs"]
    score = lp.sum(-1) / (out["tokens"] != -1).sum(-1).clamp(min=1).to(torch.float32)
    return vote_rule(out["tokens"].cpu().numpy(), score.cpu().numpy())


def assert_vote(out, want):
    for k in KEYS:
        got = out["vote"][k].cpu().numpy()
        assert got.dtype == want[k].dtype and np.array_equal(got, want[k]), (k, got, want[k])


def test_vote_end_to_end(tiny):  # noqa: F811
    eng, batch = tiny.eng, tiny.batch
    B = len(tiny.prefix)
    kw = dict(num_return_sequences=5, min_p=0.05, vote=True, seed=7, stop_at_eos=True, max_new_tokens=6, return_logprobs=True)
    out = generate.generate(eng, batch, temperature=3.0, **kw)
    assert tuple(out["tokens"].shape) == (B, 5, out["steps"]) and set(out["vote"]) == set(KEYS)
    assert_vote(out, rule_on(out))
    print("temperature 3:", {k: v.tolist() for k, v in out["vote"].items()})
    plain = generate.generate(eng, batch, temperature=3.0, **dict(kw, vote=False))
    assert "vote" not in plain and set(out) == set(plain) | {"vote"}
    for k in ("ids", "tokens", "logprobs", "n_generated"):
        assert torch.equal(out[k], plain[k]), k       # the vote reads the samples, it does not change them
    quiet = generate.generate(eng, batch, temperature=3.0, **dict(kw, return_logprobs=False))
    assert "logprobs" not in quiet and "sum_logprob" not in quiet                 # collected for the score, returned on request
    for k in KEYS:
        assert torch.equal(quiet["vote"][k], out["vote"][k]), k
    # a peaked row: all five samples agree
    out = generate.generate(eng, batch, temperature=0.05, **kw)
    assert_vote(out, rule_on(out))
    assert out["vote"]["share"].tolist() == [1.0] * B and out["vote"]["n_groups"].tolist() == [1] * B
    assert out["vote"]["winner"].tolist() == [0] * B and out["vote"]["votes"][:, 0].tolist() == [5] * B
    greedy = generate.generate(eng, batch, temperature=0.0, stop_at_eos=True, max_new_tokens=6)
    assert torch.equal(out["ids"][:, 0], greedy["ids"])


def test_vote_under_constraints_groups_by_choice(tiny):  # noqa: F811
    eng, batch = tiny.eng, tiny.batch
    B = len(tiny.prefix)
    greedy = generate.generate(eng, batch, temperature=0.0, stop_at_eos=True, max_new_tokens=6)["tokens"].cpu().numpy()
    first = int(greedy[1, 0])                         # members that share prefixes, one of them listed twice
    members = [[first], [first, 77], [first, 77, 78], [9000, 77], [first, 77], [9001]]
    out = generate.generate(eng, batch, temperature=3.0, num_return_sequences=5, vote=True, seed=3, constraints=members,
                            max_new_tokens=6, return_logprobs=True)
    assert_vote(out, rule_on(out))
    choice, group, winner = out["choice"].cpu().numpy(), out["vote"]["group"].cpu().numpy(), out["vote"]["winner"].cpu().numpy()
    assert (choice >= 0).all()
    print("choices", choice.tolist(), "groups", group.tolist(), "winner", winner.tolist())
    for b in range(B):
        for i in range(5):
            for j in range(5):
                assert (group[b, i] == group[b, j]) == (choice[b, i] == choice[b, j]), (b, i, j)
        assert choice[b, winner[b]] == choice[b, group[b, winner[b]]]
    with pytest.raises(ValueError):
        generate.generate(eng, batch, temperature=3.0, num_return_sequences=1, vote=True, seed=3)


def test_model_generate_returns_the_winner(tiny):  # noqa: F811
    from tests.test_generate_gpu import model_of
    m = model_of("tiny_peakedperm", torch.float32)
    kw = dict(temperature=3.0, min_p=0.05, num_return_sequences=5, seed=7, max_new_tokens=6)
    every = m.generate(tiny.batch, **kw)
    best = m.generate(tiny.batch, vote=True, **kw)
    g = m.last_generation
    assert set(g["vote"]) == set(KEYS) and g["answers"] == every
    assert best == [every[b][int(k)] for b, k in enumerate(g["vote"]["winner"].cpu())]
