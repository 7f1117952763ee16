// The token step of jump-forward constrained greedy decoding (fvqa/generate.py: generate(constraints=C, jump_forward=T)):
// everything between the LM head and the next pass's first RMSNorm in ONE launch, one 256-thread workgroup per sequence. Under a
// trie of allowed answers a row whose node has a single child has nothing to decide: the token is fixed whatever the logits say.
// This step picks the one token that IS a decision from the logits, then walks the trie on while it offers exactly one edge and
// commits those tokens too — up to T per step —, and the next pass feeds ALL of them, so that their k / v join the cache
// (fvqa_attn_suffix_append) without a pass of their own (include/fvqa.h fvqa_trie_jump_step states the rule).
//
//   fed      (want_logprobs) the log-probability of each token w_j, 1 <= j < m, the previous step chained, under the row it
//            was fed behind: l[w_j] - lse of row j - 1, the lse of fvqa_decode_next_ex's rule 5 (maximum, sum of expf in strided
//            order, shuffles, the four waves in order). Without want_logprobs the rows 0 .. m - 2 are never read.
//   pick     on the LAST fed row, m - 1: csrc/row_sample.h's view of the row (RowElems) and its greedy pick, the code
//            decode_next_k<.., TRIE> runs at temperature 0. A row at node == -1: the largest logit over the vocabulary, lowest
//            index on exact ties. A row at a node: the same over the node's edge list — the edge range clamped into
//            [0, n_edges], edges whose token lies outside [0, V) skipped, lowest edge on ties —, the child clamped to n_nodes.
//            The row's lse, for the token's log-probability, in front of it.
//   chain    ONE thread: at most T - 1 dependent steps of "the node's clamped edge range holds exactly one edge, its token is
//            inside the vocabulary". The committed tokens stay in LDS for the embedding gather.
//   outputs  the rows of the next pass (embeddings of the committed tokens; zeros behind), start / len for the suffix attention,
//            the step's tokens and log-probabilities, the count of running rows through the caller's ticket word (an INTEGER
//            atomic; the workgroup that arrives last writes the count and puts the word back to zero: csrc/token_step.h).
// No float atomics, fixed summation orders: two launches on the same inputs give the same bits.
#include "row_sample.h"
#include "token_step.h"

namespace {

constexpr int TMAX = 16;                 // rows of a sequence per pass (fvqa_attn_suffix's suffix_len limit)

template <typename T>
__global__ __launch_bounds__(NT) void trie_jump_step_k(const float* __restrict__ logits, const T* __restrict__ emb, Trie tr,
                                                       int eos_id, int max_new, int chain_eos, int want_logprobs,
                                                       int64_t* __restrict__ ids, int32_t* __restrict__ pos,
                                                       int32_t* __restrict__ done, int32_t* __restrict__ n_generated,
                                                       int32_t* __restrict__ node, int32_t* __restrict__ w,
                                                       int32_t* __restrict__ len_p, int32_t* __restrict__ start_p,
                                                       int64_t* __restrict__ pos64, T* __restrict__ x_next,
                                                       int32_t* __restrict__ token_out, float* __restrict__ logprob_pick,
                                                       float* __restrict__ logprob_fed, int32_t* __restrict__ n_committed,
                                                       int32_t* __restrict__ n_active, unsigned* __restrict__ counter, int B,
                                                       int Tn, int V, int D, int S, int vec16) {
  __shared__ float redf[4];
  __shared__ int redi[4];
  __shared__ int cm[TMAX];               // the tokens committed by this step, in order
  __shared__ int s_nc, s_done, s_src;
  const int b = blockIdx.x, tid = threadIdx.x;
  int64_t* row_ids = ids + (size_t)b * S;
  const int p0 = pos[b];
  const int ngen0 = n_generated[b];
  int m = len_p[b];
  m = m < 1 ? 1 : (m > Tn ? Tn : m);
  // a finished row, one with no room for another token and one whose budget is spent commit nothing
  const bool live0 = done[b] == 0 && p0 >= -1 && p0 + 1 < S && ngen0 < max_new;
  bool live = live0;
  const int nd = node ? node[b] : -1;

  // ---- the log-probabilities of the tokens the previous step chained: w_j under row j - 1
  for (int j = 1; j < Tn; ++j) {
    float lp = 0.f;
    if (want_logprobs && live0 && j < m) {
      const int t = w[(size_t)b * Tn + j];
      if ((unsigned)t < (unsigned)V) {
        const float* lr = logits + ((size_t)b * Tn + j - 1) * V;
        const float lse = row_lse(lr, V, redf);
        lp = lr[t] - lse;
      }
    }
    if (tid == 0) logprob_fed[(size_t)b * Tn + j] = lp;
  }
  if (tid == 0) logprob_fed[(size_t)b * Tn] = 0.f;

  // ---- the pick, on the last fed row: greedy over the row's elements (the vocabulary at node -1, else the node's edge list; a
  // trie that was not given has no nodes)
  const float* lg = logits + ((size_t)b * Tn + m - 1) * V;
  const RowElems<true> el = row_elems<true>(V, tr, live ? nd : -1, redi);
  const bool cons = el.cons;
  if (el.n_ok == 0) live = false;                                  // no children (or a node outside the trie): the row ends
  int tok = -1, child = -1;
  float lse = 0.f;
  if (live) {
    lse = row_lse(lg, V, redf);
    const int sel = row_pick_greedy(el, [&](int t) { return lg[t]; }, redf, redi);
    tok = el.tok(sel);
    if (cons) child = tr.child(el.ec[sel]);
  }
  __syncthreads();                                                 // (every read of pos / done / len / w / node above is over)

  // ---- commit the pick, walk the chain, step the row: one thread
  if (tid == 0) {
    int p = p0, ngen = ngen0, nc = 0, cur = nd;
    int now_done = live ? 0 : 1;
    if (live) {
      p += 1;
      ngen += 1;
      row_ids[p] = tok;                                            // (p <= S - 1: checked before every commit)
      cm[nc++] = tok;
      if (cons) cur = child;
      if (tok == eos_id || ngen >= max_new) now_done = 1;
      while (cons && !now_done && nc < Tn && p + 1 < S && ngen < max_new && cur >= 0 && cur < tr.n_nodes) {
        int e0, e1;
        tr.edges(cur, e0, e1);
        if (e1 - e0 != 1) break;                                   // a decision (or a dead end): the next step's pick
        const int t = tr.edge_token[e0];
        if ((unsigned)t >= (unsigned)V) break;
        if (t == eos_id && !chain_eos) break;                      // the EOS is left to a pick from real logits
        p += 1;
        ngen += 1;
        row_ids[p] = t;
        cm[nc++] = t;
        cur = tr.child(tr.edge_child[e0]);
        if (t == eos_id || ngen >= max_new) now_done = 1;
      }
      pos[b] = p;
      n_generated[b] = ngen;
      if (cons) node[b] = cur;
    }
    if (live0)                                                     // (a row that was not live keeps its w)
      for (int j = 0; j < Tn; ++j) w[(size_t)b * Tn + j] = j < nc ? cm[j] : -1;
    for (int j = 0; j < Tn; ++j) token_out[(size_t)b * Tn + j] = j < nc ? cm[j] : -1;
    logprob_pick[b] = live ? lg[tok] - lse : 0.f;
    n_committed[b] = nc;
    done[b] = now_done;
    // what the next pass feeds: a running row all it committed, from the first one's position on; a done row one valid row
    const int at = valid_pos(p, S);
    const int feed = now_done ? 0 : nc;
    const int st = now_done ? at : p0 + 1;
    len_p[b] = feed;
    start_p[b] = st;
    if (pos64) pos64[b] = st;
    int src = 0;
    if (now_done) src = valid_token(nc > 0 ? (int64_t)cm[nc - 1] : row_ids[at], V);   // (a commit of this step is in LDS)
    s_nc = feed;
    s_done = now_done;
    s_src = src;
    ticket_arrive(counter, n_active, B, !now_done);
  }
  __syncthreads();
  // ---- the next pass's input rows: emb of the committed tokens (a done row: of its current token, one row), zeros behind
  const int n_emb = s_done ? 1 : s_nc;                             // (next_pass_rows costs this kernel two SGPRs and a wave of occupancy)
  for (int j = 0; j < Tn; ++j) {
    T* dst = x_next + ((size_t)b * Tn + j) * D;
    if (j < n_emb) copy_row(dst, emb + (size_t)(s_done ? s_src : cm[j]) * D, D, vec16, tid);
    else zero_row(dst, D, vec16, tid);
  }
}

}  // namespace

extern "C" int fvqa_trie_jump_step(const float* logits, const void* emb, const int32_t* node_first, const int32_t* edge_token,
                                   const int32_t* edge_child, int n_nodes, int n_edges, int eos_id, int max_new_tokens,
                                   int chain_eos, int want_logprobs, int64_t* ids, int32_t* pos, int32_t* done,
                                   int32_t* n_generated, int32_t* node, int32_t* w, int32_t* len, int32_t* start, int64_t* pos64,
                                   void* x_next, int32_t* token, float* logprob_pick, float* logprob_fed, int32_t* n_committed,
                                   int32_t* n_active, uint32_t* counter, int n_seq, int jump_forward, int vocab, int dim,
                                   int seq_len, int dtype, void* stream) {
  if (!logits || !emb || !ids || !pos || !done || !n_generated || !w || !len || !start || !x_next || !token || !logprob_pick ||
      !logprob_fed || !n_committed || !n_active || !counter)
    return FVQA_EINVAL;
  if (!fvqa_dtype_ok(dtype)) return FVQA_EINVAL;
  const int given = fvqa_trie_given(node, node_first, edge_token, edge_child);
  if (given < 0) return FVQA_EINVAL;
  const bool no_trie = given == 0;                                 // every row unconstrained
  if (n_seq <= 0 || jump_forward <= 0 || vocab <= 0 || dim <= 0 || seq_len <= 0 || max_new_tokens <= 0) return FVQA_ESHAPE;
  if (jump_forward > TMAX || n_seq > 65535 || (int64_t)n_seq * jump_forward > 65535) return FVQA_ESHAPE;   // (the ticket counts
                                                                   // arrivals in 16 bits; the pass's rows are a grid dimension)
  if (!no_trie && (n_nodes <= 0 || n_edges < 0)) return FVQA_ESHAPE;
  if (!fvqa_aligned(fvqa_dtype_size(dtype), emb, x_next) ||
      !fvqa_aligned(4, logits, node_first, edge_token, edge_child, pos, done, n_generated, node, w, len, start, token,
                    logprob_pick, logprob_fed, n_committed, n_active, counter) ||
      !fvqa_aligned(8, ids, pos64))
    return FVQA_EALIGN;
  hipStream_t st = (hipStream_t)stream;
  const Trie tr{node_first, edge_token, edge_child, no_trie ? 0 : n_nodes, no_trie ? 0 : n_edges};
  fvqa_by_dtype(dtype, [&](auto* t) {
    using T = std::remove_pointer_t<decltype(t)>;
    hipLaunchKernelGGL(trie_jump_step_k<T>, dim3(n_seq), dim3(NT), 0, st, logits, (const T*)emb, tr, eos_id, max_new_tokens,
                       chain_eos, want_logprobs, ids, pos, done, n_generated, node, w, len, start, pos64, (T*)x_next, token,
                       logprob_pick, logprob_fed, n_committed, n_active, counter, n_seq, jump_forward, vocab, dim, seq_len,
                       fvqa_vec16(dim * sizeof(T), emb, x_next));
  });
  FVQA_CHECK_LAUNCH();
  return FVQA_OK;
}
