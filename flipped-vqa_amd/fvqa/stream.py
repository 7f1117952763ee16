"""In-flight batching for offline generation: a decode batch of `slots` rows in which a finished row hands its slot to the next
waiting request, so that the cost of N requests is the sum of their answers over the batch size and not, batch by batch, the
longest answer of each batch (fvqa/generate.py: a rectangular batch runs to the end of its longest row).

`generate_stream` is the loop; `admission` is the ONE decision it takes per token step and `simulate` a host model of the whole
loop without torch that takes the same decision through the same function — what the live loop launches for given answer
lengths is what `simulate` says.

The policy, before token step t = 0, 1, ...:
  1. learn   after every token step the slots' `done` flags and the running count go to pinned host memory behind an event. Before
             step t the host waits for the event of step t - 2 and reads that snapshot: a slot joins the free set when the
             snapshot shows it done and it was seated no later than iteration t - 2. All slots are free at the start. The host
             never waits for the step it has just queued.
  2. admit   if requests are waiting and len(free) >= min(admit, len(waiting)): the next m = min(admit, len(free), len(waiting))
             requests, in order, take the lowest-numbered free slots — one admission per iteration, one prefill per admission,
             always at `admit` sequences (a short last group is padded by repeating its last request; the padding is not
             seated). The prefill is generate._prefill's training forward in its own arena; ops.kv_beam_move carries rows
             [0, prefix) of the admitted prompts into the slots' sequences of the stream's own cache (the next prefill overwrites
             the arena), ops.slot_seat seats them.
  3. end     when nothing waits and every slot is in the free set: the lag costs two token steps at the end, as the lag-one stop
             of `generate` costs its one.
  4. step    ops.decode_next_stream — one launch —, then the layers and the head.
Rows of a slot's previous tenant behind the newcomer's prefix stay in the cache: fvqa_attn_decode reads keys up to `pos` only and
writes position `pos` before anything reads it — the argument that covers rejected drafts in the lookahead pass.
admit == slots is legal and pointless: a group then waits for the whole batch to drain, which is the rectangular batch again
(with its lag, one step more per batch than `generate` runs)."""
from __future__ import annotations

from typing import List, Sequence, Tuple

N_NEW = 31          # generate.N_NEW (kept apart: `simulate` and `admission` import nothing that needs torch)
LAG = 2             # the snapshot read before step t is that of step t - LAG


def admission(free, n_waiting: int, admit: int) -> List[int]:
    """Step 2 of the policy, the one decision of the loop: -> the slots the next requests are seated in, in request order ([]:
    nobody is admitted now)."""
    free = sorted(free)
    if n_waiting < 1 or len(free) < min(admit, n_waiting):
        return []
    return free[:min(admit, len(free), n_waiting)]


def step_cap(budgets: Sequence[int]) -> int:
    """The token steps no run of the loop exceeds: every step but 3 per request (the lag at its end, the wait for its group) and 3
    for the whole run has some request's token in it."""
    return int(sum(budgets)) + 3 * len(budgets) + 3


def check_slots(slots, admit) -> Tuple[int, int]:
    """-> (slots, admit) with admit's default put in, after the refusals."""
    if int(slots) != slots or slots < 1:
        raise ValueError("generate_stream: slots >= 1")
    if slots > 65535:
        raise ValueError("generate_stream: slots <= 65535 (the token step counts its rows in 16 bits)")
    slots = int(slots)
    if admit is None:
        admit = max(1, slots // 2)
    if int(admit) != admit or not 1 <= admit <= slots:
        raise ValueError(f"generate_stream: admit in [1, slots] = [1, {slots}]")
    return slots, int(admit)


def simulate(lengths: Sequence[int], slots: int, admit=None) -> Tuple[int, int, List[Tuple[int, int, int]]]:
    """The loop on the host: lengths[r] = the tokens request r generates (0: a prompt without room) -> (token steps, prefills,
    seatings as (step, slot, request))."""
    slots, admit = check_slots(slots, admit)
    N, cap = len(lengths), step_cap([max(int(n), 1) for n in lengths])
    free, seated_at, done_at = set(range(slots)), [-1] * slots, [-1] * slots
    nxt = n_prefills = t = 0
    seated = []
    while True:
        if t >= LAG:
            free |= {s for s in range(slots) if done_at[s] <= t - LAG and seated_at[s] <= t - LAG}
        took = admission(free, N - nxt, admit)
        if took:
            n_prefills += 1
        for s in took:
            free.discard(s)
            seated_at[s], done_at[s] = t, t + max(int(lengths[nxt]), 1) - 1     # the step that raises its `done`
            seated.append((t, s, nxt))
            nxt += 1
        if nxt == N and len(free) == slots:
            return t, n_prefills, seated
        if t >= cap:
            raise RuntimeError(f"simulate: {t} token steps exceed the cap of {cap}")
        t += 1


# ------------------------------------------------------------------------------------------------------- the live loop
def _rows(batches) -> list:
    """batches -> [(batch, row)] in request order, after the checks generate() makes on each batch."""
    from . import generate
    if isinstance(batches, dict):
        batches = [batches]
    batches = list(batches)
    if not batches:
        raise ValueError("generate_stream: no batch")
    rows = []
    for d in batches:
        generate._need_prefix(d)
        if d["text_id"]["vqa"].shape[2] != batches[0]["text_id"]["vqa"].shape[2]:
            raise ValueError("generate_stream: every batch has the same max_seq_len")
        if [k for k in ("video", "audio") if k in d] != [k for k in ("video", "audio") if k in batches[0]]:
            raise ValueError("generate_stream: every batch carries the same features")
        rows += [(d, b) for b in range(d["text_id"]["vqa"].shape[0])]
    return rows


def _group(rows, group) -> dict:
    """The prefill's batch of the requests `group` (indices into rows)."""
    import torch
    cat = lambda f: torch.cat([f(*rows[r]) for r in group], 0)      # noqa: E731
    first = rows[group[0]][0]
    sub = {k: cat(lambda d, b: d[k][b:b + 1]) for k in ("video", "audio") if k in first}
    sub["text_id"] = {"vqa": cat(lambda d, b: d["text_id"]["vqa"][b:b + 1, 0:1])}
    sub["label"] = {"vqa": cat(lambda d, b: d["label"]["vqa"][b:b + 1, 0:1])}
    sub["video_start"] = {"vqa": [rows[r][0]["video_start"]["vqa"][rows[r][1]] for r in group]}
    sub["prefix_index"] = {"vqa": [rows[r][0]["prefix_index"]["vqa"][rows[r][1]] for r in group]}
    return sub


def generate_stream(eng, batches, *, slots, admit=None, max_new_tokens=N_NEW, temperature: float = 0.0, top_p: float = 1.0,
                    top_k: int = 0, repetition_penalty: float = 1.0, return_logprobs: bool = False, constraints=None,
                    stop_at_eos: bool = True, seed=None) -> dict:
    """N requests through a decode batch of `slots` rows (the module's docstring states the policy). `batches`: one batch dict of
    the kind generate() takes, or a list of them; their N rows are the requests, numbered in order — all known up front.
    max_new_tokens: an int or N ints, a budget per request (W = the largest). temperature, top_p, top_k, repetition_penalty,
    return_logprobs, stop_at_eos, seed: generate()'s — the uniforms are one torch.rand(W, N) from generate()'s generator rule, and
    request r at its token i reads u[i, r] wherever it sits, so the draws are those of the plain call on the same N rows.
    constraints: generate()'s — one list, one list per request, or a TokenTrie over N samples; every member must fit the smallest
    budget.
    -> in request order "tokens" (N, W) int32 (-1: no token), "n_generated" (N,) int64, "ids" (N, S) int64 (each prompt with its
    tokens written from its prefix on: what generate() returns), "steps", "n_prefills", "seated" [(step, slot, request)],
    "occupancy" (running slot-steps over slots * steps); "logprobs" (N, W) / "sum_logprob" (N,) with return_logprobs; "choice"
    (N,) with constraints. A request's tokens, count and log-probabilities do not depend on its neighbours, its slot or its
    time of arrival.
    ValueError: slots < 1, slots > 65535, admit outside [1, slots], and what generate() refuses of the keywords above. Beams,
    contrast, lookahead, jump-forward and several samples per prompt are not built into the stream and are no keywords."""
    import torch

    from . import constrain, generate, ops, rowpass
    with torch.no_grad():
        slots, admit = check_slots(slots, admit)
        rows = _rows(batches)
        N = len(rows)
        budgets = [int(x) for x in max_new_tokens] if hasattr(max_new_tokens, "__len__") else [int(max_new_tokens)] * N
        if len(budgets) != N or min(budgets) < 1:
            raise ValueError(f"generate_stream: max_new_tokens is an int >= 1 or one per request ({N} requests)")
        if not temperature >= 0 or not 0 < top_p <= 1:
            raise ValueError("generate_stream: temperature >= 0, 0 < top_p <= 1")
        if int(top_k) != top_k or top_k < 0 or not repetition_penalty >= 1:
            raise ValueError("generate_stream: top_k >= 0 (0: off), repetition_penalty >= 1")
        W, cap = max(budgets), step_cap(budgets)
        S = int(rows[0][0]["text_id"]["vqa"].shape[2])
        prefix_all = [int(d["prefix_index"]["vqa"][b]) for d, b in rows]
        trie = None
        if constraints is not None:
            shape = {"prefix_index": {"vqa": prefix_all}, "text_id": {"vqa": rows[0][0]["text_id"]["vqa"]}}
            trie = generate._compiled(eng, shape, constraints, stop_at_eos, min(budgets))
        pk, dev, V = eng.pack, eng.device, eng.V
        i32 = dict(dtype=torch.int32, device=dev)
        # ---- the state on the device, allocated once per call
        cache = torch.zeros(eng.L, slots * S + eng.A, 3 * eng.D, dtype=eng.dtype, device=dev)
        ids = torch.zeros(slots, S, dtype=torch.int64, device=dev)
        pos, pos64 = torch.zeros(slots, **i32), torch.zeros(slots, dtype=torch.int64, device=dev)
        flags = torch.ones(slots + 1, **i32)                   # done (slots), then the running count: one snapshot, one copy
        done, n_active = flags[:slots], flags[slots:]
        gen_start, vstart = torch.zeros(slots, **i32), torch.zeros(slots, **i32)
        req = torch.full((slots,), -1, **i32)
        b = rowpass.buffers(eng, slots)
        b.lg.zero_()
        b.xin.zero_()
        token, n_kept = torch.zeros(slots, **i32), torch.zeros(slots, **i32)
        logprob = torch.zeros(slots, dtype=torch.float32, device=dev)
        counter, err = torch.zeros(1, **i32), torch.zeros(1, **i32)
        budget = torch.tensor(budgets, **i32)
        tokens, n_gen = torch.full((N, W), -1, **i32), torch.zeros(N, **i32)
        logprobs = torch.zeros(N, W, dtype=torch.float32, device=dev) if return_logprobs else None
        dtrie = node = roots = None
        if trie is not None:
            dtrie, roots = trie.to(dev), [int(x) for x in trie.roots(N)]
            node = torch.full((slots,), -1, **i32)
        u = None
        if temperature > 0:
            gen = None
            if seed is not None:
                gen = torch.Generator(device=dev)
                gen.manual_seed(int(seed))
            u = torch.rand(W, N, dtype=torch.float32, device=dev, generator=gen)
        kw = dict(out_logprob=logprobs, node=node, trie=dtrie, u=u, pos64=pos64, temperature=temperature, top_p=top_p,
                  top_k=int(top_k), repetition_penalty=float(repetition_penalty), eos_id=eng.model.tokenizer.eos_id,
                  stop_at_eos=stop_at_eos)
        rotated = rowpass.cache_rotated(eng)

        def attn(i, qkv, o):
            ops.attn_decode(qkv, cache[i], o, *eng.model.gate_views(i), vstart, pos64, (eng.cos, eng.sin), slots, S, eng.H,
                            eng.Dh, eng.A, eng.F, cache_rotated=rotated)

        snap = torch.empty(LAG + 1, slots + 1, dtype=torch.int32).pin_memory()      # step t lands in row t % (LAG + 1)
        arrived = [None] * (LAG + 1)
        free, seated_at = set(range(slots)), [-1] * slots
        nxt = n_prefills = t = 0
        seated = []
        while True:
            if t >= LAG:                                        # 1. learn: the snapshot of step t - 2, which left a whole step ago
                arrived[(t - LAG) % (LAG + 1)].synchronize()
                shot = snap[(t - LAG) % (LAG + 1)].tolist()
                free |= {s for s in range(slots) if shot[s] != 0 and seated_at[s] <= t - LAG}
            took = admission(free, N - nxt, admit)              # 2. admit
            if took:
                group = list(range(nxt, nxt + len(took)))
                p = generate._prefill(eng, _group(rows, group + [group[-1]] * (admit - len(group))))
                src_seq, hi = [0] * slots, [0] * slots
                for j, s in enumerate(took):
                    src_seq[s], hi[s] = j, min(max(prefix_all[group[j]], 0), S)
                mv = torch.tensor([src_seq, [0] * slots, hi], dtype=torch.int32).to(dev)
                ops.kv_beam_move(cache, p.ar.qkv, mv[0], mv[1], mv[2], S=S, A=eng.A)
                root = None if trie is None else torch.tensor([roots[r] for r in group] + [0] * (admit - len(group)), **i32)
                ops.slot_seat(took, list(range(len(took))), group, p.ids, p.prefix, p.vstart, p.ar.logits, ids, pos, pos64, done,
                              gen_start, vstart, req, b.lg, err, root=root, node=node)
                n_prefills += 1
                for s, r in zip(took, group):
                    free.discard(s)
                    seated_at[s] = t
                    seated.append((t, s, r))
                nxt += len(took)
            if nxt == N and len(free) == slots:                 # 3. end
                break
            if t >= cap:
                raise RuntimeError(f"generate_stream: {t} token steps exceed the cap of {cap} for these budgets")
            ops.decode_next_stream(b.lg, pk.emb, ids, pos, done, gen_start, b.xin, token, n_kept, logprob, n_active, counter, req,
                                   budget, tokens, n_gen, **kw)            # 4. token step t
            snap[t % (LAG + 1)].copy_(flags, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
            arrived[t % (LAG + 1)] = ev
            rowpass.head(eng, rowpass.layers(eng, b, attn), b.xn, b.lg)
            t += 1
        if int(err) != 0:
            raise RuntimeError("generate_stream: the device refused a seating (an occupied slot or an index outside the arrays)")
        n_generated = n_gen.to(torch.int64)
        prompts = torch.cat([d["text_id"]["vqa"][bb:bb + 1, 0] for d, bb in rows], 0).to(dev).clone()
        prefix = torch.tensor(prefix_all, dtype=torch.int64, device=dev)
        col = torch.arange(W, device=dev).unsqueeze(0)
        at = prefix.unsqueeze(1) + col
        inside = (col < n_generated.unsqueeze(1)) & (at >= 0) & (at < S)
        prompts[torch.arange(N, device=dev).unsqueeze(1).expand(N, W)[inside], at[inside]] = tokens[inside].to(torch.int64)
        out = {"tokens": tokens, "n_generated": n_generated, "ids": prompts, "steps": t, "n_prefills": n_prefills,
               "seated": seated, "occupancy": float(n_generated.sum()) / float(slots * max(t, 1))}
        if return_logprobs:
            out["logprobs"] = logprobs
            out["sum_logprob"] = logprobs.sum(1)
        if trie is not None:
            out["choice"] = torch.as_tensor(constrain.choice_of(trie, tokens), device=dev)
        return out
