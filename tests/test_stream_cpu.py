"""In-flight batching without a GPU: `fvqa.stream.simulate` against an independent restatement of the policy (the issue's, written
here a second time and differently: per-request events on a timeline instead of per-slot state), the step counts the policy
implies for the streams of tests/golden/gen_eos_*, every refusal, and header / bindings / exports."""
import ctypes as C
import random
import re
import os
import types

import pytest
import torch

from fvqa import _lib, ops, stream

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A = C.c_void_p(256)
BUILDS = [("bf16", _lib.BF16), ("f16", _lib.F16)]
EOS_K = [1, 3, 6, 12]                               # the greedy answer lengths of gen_eos_*_peakedperm's four samples


# ------------------------------------------------------------------------------------------------ the policy, restated
def restated(lengths, slots, admit):
    """The policy told from the requests' side. free_from[s] = the first iteration at which the host may know slot s free:
    a tenant seated at t0 that generates n tokens raises `done` in step t0 + max(n, 1) - 1, the snapshot of step x is read before
    step x + 2. -> (steps, prefills, seatings, the iteration each seating's slot became known free)."""
    free_from = [0] * slots
    waiting = list(range(len(lengths)))
    t = prefills = 0
    seatings, known = [], []
    while True:
        free = [s for s in range(slots) if free_from[s] <= t]
        if waiting and len(free) >= min(admit, len(waiting)):
            m = min(admit, len(free), len(waiting))
            prefills += 1
            for s in free[:m]:
                r = waiting.pop(0)
                known.append(free_from[s])
                seatings.append((t, s, r))
                free_from[s] = max(t + max(lengths[r], 1) - 1, t) + 2
        if not waiting and all(f <= t for f in free_from):
            return t, prefills, seatings, known
        t += 1
        assert t < 10 ** 6


def check(lengths, slots, admit):
    steps, prefills, seated = stream.simulate(lengths, slots, admit)
    want = restated(lengths, slots, admit)
    assert (steps, prefills, seated) == want[:3], (lengths, slots, admit)
    assert sorted(r for _, _, r in seated) == list(range(len(lengths)))                 # every request seated once
    assert [r for _, _, r in seated] == list(range(len(lengths)))                       # ... and in order
    assert all(k <= t for (t, _, _), k in zip(seated, want[3]))                         # never before a snapshot showed it free
    busy = {}
    for t, s, r in seated:                                                              # no slot holds two running requests
        assert busy.get(s, -1) < t
        busy[s] = t + max(lengths[r], 1) - 1
    assert steps <= stream.step_cap([max(n, 1) for n in lengths])
    return steps, prefills, seated


def test_the_streams_of_the_fixtures():
    L = EOS_K * 3
    steps, prefills, seated = check(L, 4, 2)
    assert (steps, prefills, sum(L)) == (29, 6, 66)                                     # 66 running slot-steps of 4 * 29
    assert check(L[::-1], 3, 1)[:2] == (30, 12)
    assert check([min(n, 4) for n in L], 4, 2)[:2] == (16, 6)
    assert check(L, 4, 4)[:2] == (39, 3)                                                # admit == slots: the rectangular batches
    assert 3 * check(EOS_K, 4, 4)[0] == 39                                              # three plain batches of four
    assert seated[:4] == [(0, 0, 0), (0, 1, 1), (1, 2, 2), (1, 3, 3)]                   # one admission per iteration
    assert check([3, 6, 12, 24] * 16, 8, 4)[:2] == (127, 16)                            # the measurement's stream
    assert stream.simulate(L, 4) == stream.simulate(L, 4, 2)                            # admit defaults to slots // 2
    assert stream.simulate([5], 1) == (6, 1, [(0, 0, 0)])                               # ... and to 1 at one slot


def test_simulate_against_the_restatement_on_random_streams():
    rng = random.Random(7)
    for _ in range(400):
        slots = rng.randint(1, 9)
        admit = rng.randint(1, slots)
        lengths = [rng.choice([0, 1, 1, 2, 3, 5, 8, 13, 31]) for _ in range(rng.randint(1, 40))]
        check(lengths, slots, admit)


def test_admission_is_the_one_decision():
    assert stream.admission({3, 1, 2}, 5, 2) == [1, 2]
    assert stream.admission({3}, 5, 2) == []                                            # fewer free than a group
    assert stream.admission({3}, 1, 2) == [3]                                           # ... unless nobody else waits
    assert stream.admission({0, 1, 2, 3}, 0, 2) == []
    assert stream.admission(set(), 4, 1) == []
    assert stream.admission({5, 0}, 9, 4) == []
    assert stream.admission({5, 0, 7, 2, 1}, 9, 4) == [0, 1, 2, 5]


# ------------------------------------------------------------------------------------------------ refusals
def test_slots_and_admit_are_checked_before_anything_else():
    for slots, admit in ((0, None), (-1, None), (65536, None), (4, 0), (4, 5), (1, 2), (2.5, None), (4, 1.5)):
        with pytest.raises(ValueError, match="slots|admit"):
            stream.simulate([1, 2], slots, admit)
        with pytest.raises(ValueError, match="slots|admit"):
            stream.generate_stream(None, {}, slots=slots, admit=admit)                  # (before the batch or the engine is read)
    assert stream.check_slots(65535, None) == (65535, 32767) and stream.check_slots(1, None) == (1, 1)


def test_generate_stream_has_no_keyword_for_what_it_does_not_run():
    import inspect
    kw = set(inspect.signature(stream.generate_stream).parameters)
    assert kw == {"eng", "batches", "slots", "admit", "max_new_tokens", "temperature", "top_p", "top_k", "repetition_penalty",
                  "return_logprobs", "constraints", "stop_at_eos", "seed"}
    import llama
    m = types.SimpleNamespace(ensure_engine=lambda: pytest.fail("refused before the engine is built"))
    for k in ("num_beams", "contrast", "lookahead", "jump_forward", "num_return_sequences"):
        with pytest.raises(ValueError, match=k):
            llama.Transformer.generate_stream(m, {}, slots=4, **{k: 2})


def test_budgets_and_sampling_parameters_are_refused_on_the_host():
    ids = torch.zeros(3, 1, 16, dtype=torch.int64)
    batch = {"text_id": {"vqa": ids}, "label": {"vqa": ids}, "video_start": {"vqa": [0, 0, 0]}, "prefix_index": {"vqa": [4, 4, 4]}}
    for kw in (dict(max_new_tokens=0), dict(max_new_tokens=[3, 3]), dict(max_new_tokens=[3, 0, 3]), dict(temperature=-1.0),
               dict(top_p=0.0), dict(top_p=1.5), dict(top_k=-1), dict(repetition_penalty=0.5)):
        with pytest.raises(ValueError, match="generate_stream"):
            stream.generate_stream(None, batch, slots=2, **kw)
    with pytest.raises(ValueError, match="prefix_index"):
        stream.generate_stream(None, {"text_id": {"vqa": ids}}, slots=2)
    with pytest.raises(ValueError, match="no batch"):
        stream.generate_stream(None, [], slots=2)
    other = dict(batch, text_id={"vqa": torch.zeros(3, 1, 32, dtype=torch.int64)})
    with pytest.raises(ValueError, match="max_seq_len"):
        stream.generate_stream(None, [batch, other], slots=2)


def test_the_parsers_accept_the_flags_and_refuse_what_a_stream_does_not_decode(capsys):
    import answer
    import train
    base = ["--is_generation_task"]
    a = train.get_args_parser().parse_args(base + ["--gen_stream", "8", "--gen_stream_admit", "2"])
    assert (a.gen_stream, a.gen_stream_admit) == (8, 2)
    a = train.get_args_parser().parse_args(base)
    assert (a.gen_stream, a.gen_stream_admit) == (0, None)                              # off by default
    assert train.get_args_parser().parse_args(base + ["--gen_stream", "8", "--gen_constrain", "options"]).gen_stream == 8
    for bad in (["--num_beams", "2"], ["--contrast", "blind"], ["--lookahead", "4"],
                ["--gen_constrain", "options", "--gen_jump_forward", "4"]):
        with pytest.raises(SystemExit):
            train.get_args_parser().parse_args(base + ["--gen_stream", "8"] + bad)
        assert "--gen_stream" in capsys.readouterr().err
    for bad in (["--gen_stream", "-1"], ["--gen_stream", "65536"], ["--gen_stream", "4", "--gen_stream_admit", "5"],
                ["--gen_stream", "4", "--gen_stream_admit", "0"], ["--gen_stream_admit", "2"]):
        with pytest.raises(SystemExit):
            train.get_args_parser().parse_args(base + bad)
    q = ["--questions", "q.txt"]
    a = answer.get_args_parser().parse_args(q + ["--slots", "4", "--admit", "1", "--temperature", "0.7", "--top_k", "8"])
    assert (a.questions, a.slots, a.admit, a.question) == ("q.txt", 4, 1, None)
    for bad in (["--num_beams", "2"], ["--contrast", "blind"], ["--lookahead", "4"], ["--constrain", "--jump_forward", "4"],
                ["--temperature", "0.7", "--num_samples", "2"], ["--admit", "5"]):
        with pytest.raises(SystemExit):
            answer.get_args_parser().parse_args(q + ["--slots", "4"] + bad)
        assert "--slots" in capsys.readouterr().err


def test_validation_without_the_flag_never_touches_the_stream():
    import engine
    called = []

    class M(torch.nn.Module):
        def inference_stream(self, *a):
            called.append(a)
            raise AssertionError("not without --gen_stream")

        def forward(self, data, inference=False):
            return torch.tensor([1, 0]), [{"video_id": None, "question": "q", "generated_answer": "a"}] * 2

    data = {"answer": torch.tensor([1, 1]), "qtype": torch.tensor([1, 2]), "text": ["", ""], "vid": [None, None]}
    opt = types.SimpleNamespace(param_groups=[{"lr": 0.25}])
    for a in (types.SimpleNamespace(is_generation_task=True, dataset="nextqa", debug=False, output_dir=None),
              types.SimpleNamespace(is_generation_task=True, dataset="nextqa", debug=False, output_dir=None, gen_stream=0)):
        stats = engine.val_one_epoch(M(), [data, data], opt, epoch=0, args=a)
        assert stats["acc"] == 0.5 and not called


# ------------------------------------------------------------------------------------------------ header, bindings, exports
def _header():
    text = open(os.path.join(ROOT, "include", "fvqa.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def _declared_args(name):
    m = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, _header(), flags=re.S)
    assert m, name
    return [a.strip() for a in m.group(1).split(",")]


def _ctype_of(decl):
    if "*" in decl:
        return C.c_void_p
    return {"int": C.c_int, "float": C.c_float}[decl.split()[0]]


@pytest.mark.parametrize("name", ["fvqa_decode_next_stream", "fvqa_slot_seat"])
def test_header_bindings_and_exports_agree(name):
    want = [_ctype_of(d) for d in _declared_args(name)]
    res, args = _lib.SIGNATURES[name]
    assert res is C.c_int and args == want, name
    for which, _ in BUILDS:
        lib = _lib.load(which)
        assert lib.fvqa_version() == _lib.ABI_VERSION == 18       # entries are only added
        assert callable(getattr(lib, name))
    assert callable(ops.decode_next_stream) and callable(ops.slot_seat)
    # the four older entries of the template keep their declarations
    assert len(_declared_args("fvqa_decode_next_ex")) == 26 and len(_declared_args("fvqa_decode_next_trie")) == 32


def _stream_args(dt, temperature=0.7, trie=True, n_req=5, width=3, n_seq=3):
    t = A if trie else None
    #      logits u emb T        top_p k r   eos stop ids pos done gen x tok kept lp act cnt pos64 node nf et ec nn ne
    return [A, A, A, temperature, 0.9, 8, 1.2, 2, 1, A, A, A, A, A, A, A, A, A, A, A, t, t, t, t, 4, 3,
            A, A, n_req, width, A, A, A, n_seq, 509, 128, 16, dt, None]  # req budget n_req width out_tok out_lp out_n B V D S dt st


@pytest.mark.parametrize("which,h16", BUILDS)
def test_the_stream_entry_checks_its_operands_on_the_host(which, h16):
    """Every call here must be refused: one that passed validation would launch a kernel on fake addresses."""
    fn = _lib.load(which).fvqa_decode_next_stream
    assert len(_stream_args(h16)) == len(_lib.SIGNATURES["fvqa_decode_next_stream"][1])
    for dt in (h16, _lib.F32):
        for trie in (True, False):
            base = _stream_args(dt, trie=trie)
            for at in (0, 1, 2, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 26, 27, 30, 32):   # every required pointer; u when sampling
                a = list(base)
                a[at] = None
                assert fn(*a) == -1, (dt, trie, at)
        for at in (20, 21, 22, 23):                                                        # a trie given in part
            a = _stream_args(dt)
            a[at] = None
            assert fn(*a) == -1, at
        for at, v in ((28, 0), (29, 0), (33, 0), (33, 65536), (34, 0), (35, 0), (36, 0), (24, 0)):
            a = _stream_args(dt)
            a[at] = v
            assert fn(*a) == -2, (at, v)
        for at in (26, 27, 30, 31, 32):                                                    # off a 4-byte boundary
            a = _stream_args(dt)
            a[at] = C.c_void_p(258)
            assert fn(*a) == -3, at
        for bad in (dict(temperature=-1.0), dict(temperature=float("nan"))):
            assert fn(*_stream_args(dt, **bad)) == -1
    other = _lib.F16 if h16 == _lib.BF16 else _lib.BF16
    assert fn(*_stream_args(other)) == -1                                                  # the other build's 16-bit code


def _seat_args(n_admit=2, n_src=3, n_slots=5, S=16, V=509, trie=True):
    t = A if trie else None
    #      slot src request n_admit ids prefix vstart logits root n_src ids pos pos64 done gen vstart req node lg err
    return [A, A, A, n_admit, A, A, A, A, t, n_src, A, A, A, A, A, A, A, t, A, A, n_slots, S, V, None]


def test_the_seating_entry_checks_its_operands_on_the_host():
    fn = _lib.load().fvqa_slot_seat
    assert len(_seat_args()) == len(_lib.SIGNATURES["fvqa_slot_seat"][1])
    for trie in (True, False):
        for at in (0, 1, 2, 4, 5, 6, 7, 10, 11, 12, 13, 14, 15, 16, 18, 19):
            a = _seat_args(trie=trie)
            a[at] = None
            assert fn(*a) == -1, (trie, at)
    for at in (8, 17):                                                                     # root and node: both or neither
        a = _seat_args()
        a[at] = None
        assert fn(*a) == -1, at
    for at, v in ((3, 0), (3, 6), (9, 0), (20, 0), (20, 65536), (21, 0), (22, 0)):
        a = _seat_args()
        a[at] = v
        assert fn(*a) == -2, (at, v)
    for at, p in ((0, 258), (7, 258), (18, 258), (19, 258), (4, 260), (5, 260), (10, 260), (12, 260)):
        a = _seat_args()
        a[at] = C.c_void_p(p)
        assert fn(*a) == -3, (at, p)


def test_the_seating_wrapper_refuses_duplicates_before_it_reads_a_tensor():
    t = None
    for slot, src, request in (([1, 1], [0, 1], [4, 5]), ([1, 2], [0, 1], [4, 4]), ([1], [0, 1], [4, 5]), ([], [], [])):
        with pytest.raises(ValueError, match="slot_seat"):
            ops.slot_seat(slot, src, request, t, t, t, t, t, t, t, t, t, t, t, t, t)
