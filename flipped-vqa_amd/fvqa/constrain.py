"""Constrained decoding: the set of allowed answers as data (`generate(constraints=...)`, include/fvqa.h fvqa_decode_next_trie /
fvqa_beam_step_trie).

The caller gives the allowed answers as token sequences — one list for the whole batch, or one list per sample. `TokenTrie`
compiles them into ONE trie in CSR form (int32 arrays the token-step kernels read on the device): every token step of a row may
only continue a prefix of one of its answers, and the EOS that `from_sequences` appends to every answer is the only way into a
leaf, so a finished row IS a member of the set. Hugging Face offers the same capability as `prefix_allowed_tokens_fn`.
"""
from __future__ import annotations

from typing import List, Sequence

import numpy as np

A_TEXT = "Answer: The answer is "     # dataloader a_text; the answer starts 5 tokens behind the "Answer" marker (prefix_index)
A_SKIP = 5


def _is_seq_of_ints(s) -> bool:
    return not isinstance(s, (str, bytes)) and hasattr(s, "__len__") and all(isinstance(t, (int, np.integer)) for t in s)


def _plain(s) -> list:
    return s.tolist() if hasattr(s, "tolist") else list(s)


class TokenTrie:
    """node_first (n_nodes + 1,), edge_token (n_edges,), edge_child (n_edges,), root (B,) — int32; the edges of a node are in
    ascending token order. `shared`: one answer set for every row (root then has one entry; `roots(B)` repeats it).
    On the host: `leaf_choice` {leaf node: the lowest index of its answer in the sample's list}, `n_members` and `max_len`
    (tokens of the longest answer, its EOS included) per root, `eos_id`, `vocab`. The arrays are numpy until `.to(device)`."""

    def __init__(self, node_first, edge_token, edge_child, root, leaf_choice, shared, eos_id, vocab, n_members, max_len):
        self.node_first, self.edge_token, self.edge_child, self.root = node_first, edge_token, edge_child, root
        self.leaf_choice, self.shared, self.eos_id, self.vocab = leaf_choice, bool(shared), int(eos_id), int(vocab)
        self.n_members, self.max_len = list(n_members), list(max_len)

    @property
    def n_nodes(self) -> int:
        return int(self.node_first.shape[0]) - 1

    @property
    def n_edges(self) -> int:
        return int(self.edge_token.shape[0])

    @classmethod
    def from_sequences(cls, seqs, eos_id: int, vocab: int) -> "TokenTrie":
        """seqs: one list of token-id sequences for the whole batch, or one such list per sample. The EOS is appended to every
        sequence; duplicates merge (the leaf maps to the lowest index); the empty sequence is legal (the answer is the EOS
        alone). ValueError: an empty set, a token outside [0, vocab), an EOS inside a sequence."""
        eos_id, vocab = int(eos_id), int(vocab)
        if not 0 <= eos_id < vocab:
            raise ValueError(f"TokenTrie: eos_id {eos_id} outside [0, {vocab})")
        if isinstance(seqs, np.ndarray):
            seqs = seqs.tolist()
        seqs = list(seqs)
        if len(seqs) == 0:
            raise ValueError("TokenTrie: an empty set of allowed answers")
        shared = all(_is_seq_of_ints(_plain(s)) for s in seqs)
        samples = [seqs] if shared else seqs
        children: List[dict] = []            # per node: {token: child}
        leaf_choice, roots, n_members, max_len = {}, [], [], []
        for b, members in enumerate(samples):
            members = [_plain(m) for m in members]
            if len(members) == 0:
                raise ValueError(f"TokenTrie: sample {b} has an empty set of allowed answers")
            root = len(children)
            children.append({})
            roots.append(root)
            leaves = set()
            for idx, seq in enumerate(members):
                if not _is_seq_of_ints(seq):
                    raise ValueError(f"TokenTrie: sample {b}, answer {idx}: a sequence of token ids is expected")
                seq = [int(t) for t in seq]
                for t in seq:
                    if not 0 <= t < vocab:
                        raise ValueError(f"TokenTrie: sample {b}, answer {idx}: token {t} outside [0, {vocab})")
                    if t == eos_id:
                        raise ValueError(f"TokenTrie: sample {b}, answer {idx}: the EOS {eos_id} inside a sequence")
                at = root
                for t in seq + [eos_id]:
                    nxt = children[at].get(t)
                    if nxt is None:
                        nxt = len(children)
                        children.append({})
                        children[at][t] = nxt
                    at = nxt
                leaf_choice.setdefault(at, idx)
                leaves.add(at)
            n_members.append(len(leaves))
            max_len.append(max(len(m) for m in members) + 1)
        node_first = np.zeros(len(children) + 1, dtype=np.int32)
        tok, child = [], []
        for n, ch in enumerate(children):
            for t in sorted(ch):
                tok.append(t)
                child.append(ch[t])
            node_first[n + 1] = len(tok)
        return cls(node_first, np.asarray(tok, dtype=np.int32), np.asarray(child, dtype=np.int32),
                   np.asarray(roots, dtype=np.int32), leaf_choice, shared, eos_id, vocab, n_members, max_len)

    def roots(self, B: int) -> np.ndarray:
        """root per row of a batch of B samples, on the host (a shared set: the one root B times)."""
        root = np.asarray(self.host().root)
        if self.shared:
            return np.repeat(root, B)
        if int(root.shape[0]) != B:
            raise ValueError(f"TokenTrie: built for {int(root.shape[0])} samples, the batch has {B}")
        return root

    def children(self, node: int):
        """-> (tokens, child nodes) of `node`, as the CSR arrays hold them (host copies)."""
        h = self.host()
        lo, hi = int(h.node_first[node]), int(h.node_first[node + 1])
        return h.edge_token[lo:hi], h.edge_child[lo:hi]

    def host(self) -> "TokenTrie":
        """The numpy form (a trie moved with .to() keeps it)."""
        return getattr(self, "_host", self)

    def to(self, device) -> "TokenTrie":
        """The same trie with its arrays as int32 tensors on `device` (what ops.decode_next_trie / beam_step_trie take)."""
        import torch
        h = self.host()
        t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.int32).to(device)  # noqa: E731
        out = TokenTrie(t(h.node_first), t(h.edge_token), t(h.edge_child), t(h.root), h.leaf_choice, h.shared, h.eos_id,
                        h.vocab, h.n_members, h.max_len)
        out._host = h
        return out


def compile_constraints(constraints, eos_id: int, vocab: int) -> TokenTrie:
    """A TokenTrie as it is (its host form), raw sequences compiled."""
    if isinstance(constraints, TokenTrie):
        return constraints.host()
    return TokenTrie.from_sequences(constraints, eos_id, vocab)


def choice_of(trie: TokenTrie, tokens) -> np.ndarray:
    """tokens (B, steps) or (B, n, steps): the generated tokens of each row, -1 where none was picked (generate's "tokens") ->
    int64 array (B,) / (B, n): the index of the generated member in the sample's list, or -1 if the row ended before a leaf (the
    sequence had no room)."""
    h = trie.host()
    tk = np.asarray(tokens.cpu() if hasattr(tokens, "cpu") else tokens)
    lead = tk.shape[:-1]
    B = lead[0]
    roots = np.asarray(h.roots(B))
    rows = tk.reshape(B, -1, tk.shape[-1])
    nf, et, ec = np.asarray(h.node_first), np.asarray(h.edge_token), np.asarray(h.edge_child)
    out = np.full(rows.shape[:2], -1, dtype=np.int64)
    for b in range(B):
        for k in range(rows.shape[1]):
            at = int(roots[b])
            for t in rows[b, k].tolist():
                if t < 0:
                    break
                lo, hi = int(nf[at]), int(nf[at + 1])
                i = lo + int(np.searchsorted(et[lo:hi], t))
                if i >= hi or int(et[i]) != t:
                    at = -1
                    break
                at = int(ec[i])
            out[b, k] = h.leaf_choice.get(at, -1)
    return out.reshape(lead)


def options_of(data: dict, tokenizer) -> List[List[List[int]]]:
    """The option token sequences of a validation batch, exactly as generate.match_answers cuts them from
    text_id['vqa'][b, c]: from the index of a_token_id in option 0's row + 5 up to the EOS (or the end of the row)."""
    ids_all = data["text_id"]["vqa"]
    B, n_opt, S = ids_all.shape
    a_id, eos = tokenizer.a_token_id, tokenizer.eos_id
    out = []
    for b in range(B):
        start = ids_all[b, 0].tolist().index(a_id) + A_SKIP
        opts = []
        for c in range(n_opt):
            tail = ids_all[b, c, start:].tolist()
            opts.append(tail[: tail.index(eos)] if eos in tail else tail)
        out.append(opts)
    return out


def encode_answers(tokenizer, answers: Sequence[str]) -> List[List[int]]:
    """answers (strings) -> their token sequences as they stand behind the prompt: enc("Answer: The answer is " + a)[5:], the
    same + 5 that prefix_index uses. ValueError if the first five tokens are not those of the bare a_text (the cut would then
    not fall between the prompt and the answer)."""
    enc = tokenizer._enc
    head = list(enc(A_TEXT))[:A_SKIP]
    out = []
    for a in answers:
        t = list(enc(A_TEXT + str(a)))
        if len(head) != A_SKIP or t[:A_SKIP] != head:
            raise ValueError(f"encode_answers: {a!r} changes the tokens of {A_TEXT!r}: {t[:A_SKIP]} != {head}")
        out.append([int(x) for x in t[A_SKIP:]])
    return out


def read_answer_vocab(path: str) -> List[str]:
    """--answer_vocab FILE: one answer per line; blank lines are skipped."""
    with open(path, encoding="utf-8") as f:
        answers = [ln.strip() for ln in f]
    answers = [a for a in answers if a]
    if not answers:
        raise ValueError(f"{path}: no answer")
    return answers
