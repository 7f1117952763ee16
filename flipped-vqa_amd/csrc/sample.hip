// The token step of the generation API (fvqa/generate.py: generate): everything between the LM head and the next token's first
// RMSNorm in ONE launch, one 256-thread workgroup per sequence — pick the token (greedy, or temperature + nucleus sampling with
// the reference's rule, llama/generation.py:17-68), write it into the id matrix, advance the position, raise the row's `done`
// flag (EOS, or the end of the sequence), gather the next input embedding, count the rows still running.
//
// The pick is not this file's text: the view of a row's elements, the greedy pick and the sampled pick are csrc/row_sample.h's
// (RowElems, row_pick_greedy, row_pick_sampled), which csrc/spec.hip, csrc/treespec.hip and csrc/jump.hip call as well. The kernel
// here decides what a row is (live, its slot, its node, its plausible set), hands the pick the view and the logit it sees
// (l1) and the draw, and steps the row. What follows states the rule the header implements.
//
// Picking with temperature > 0, per row (fp32 throughout, no sort):
//   pass 1   m = max logit
//   pass 2   e_i = __expf((l_i - m) / T), kept in LDS in place of the logits when 4*V bytes fit (else recomputed from the
//            logits, which sit in L2, by every later pass); Z = sum e_i
//   cut      the reference keeps a token iff the mass IN FRONT of it, in the order (p descending, index ascending), is
//            <= top_p. G(t) = sum of the e_i whose bit pattern is > t is a non-increasing step function of the integer t (the
//            bits of a non-negative float order as the float does), so the value of the last kept token is the smallest t
//            with G(t) <= top_p * Z: a bisection over [0, bits(1.0f)], 30 masked sums of the row. Every token above t is
//            kept; of the tokens EQUAL to t (a tie group, ordered by index) the j-th has G(t) + j*t in front of it.
//   walk     in INDEX order (the reference draws with torch.multinomial from the re-normalised kept set; the order of the
//            walk is free): each thread owns a contiguous index range, the kept mass and the tie count of the ranges are
//            scanned across the workgroup, M = the scan's total, and the first kept token whose running kept mass exceeds
//            u * M is the block-wide minimum of the threads' candidates (none exceeds it — u * M rounded up to M —: the last
//            kept token).
// Every sum runs in a fixed order (a thread's strided or contiguous elements, then shuffles, then the four waves in order);
// there are no atomics on floats: two launches on the same inputs give the same bits.
//
// n_active needs a count across workgroups: the ticket word of csrc/token_step.h. The ticket of fvqa_decode_next is a module
// global: launches of this entry on one device must be ordered (one stream, or events), as the decode loop's are.
//
// fvqa_decode_next_ex is the same kernel template with EX = true (the old entry instantiates EX = false, in which none of the
// following exists): a repetition penalty, top-k, the token's log-probability and a ticket word the caller owns.
//   penalty  the distinct ids at positions gen_start .. pos of the row's id matrix are marked in a bitmap of V bits in LDS
//            (behind the row of e_i); every read of a logit goes through l1(): l / r or l * r where the bit is set. The logits
//            are not written.
//   top-k    C(t) = the NUMBER of e_i whose bit pattern is > t is a non-increasing step function like G(t): the value of the
//            token at rank k is the smallest t with C(t) <= k - 1, the same bisection counting instead of summing. Of its tie
//            group the first k - C(t) by index are inside the k. Z_k = G(t) + (k - C(t)) * t replaces Z in the nucleus bound;
//            kept sets are prefixes of one order, so the cut is the shorter of the two prefixes (top_p == 1: the top-k one).
//   logprob  l_tok - (m + logf(sum expf(l - m))) on the RAW logits, two passes of their own whose order no parameter changes.
//
// fvqa_decode_next_trie is the template with TRIE = true as well (false in the two entries above, in which none of the following
// exists): constrained decoding over a trie of allowed answers in CSR form (fvqa/constrain.py). A row at node >= 0 picks among
// the children of its node only. Its passes run over the node's EDGE LIST instead of over the vocabulary — element i of every
// loop is edge i of the node, its logit the one at edge_token[i] —: the maximum, Z, the counts and the masked sums of both
// bisections, the tie group and the walk all see the allowed tokens and nothing else, and since a node's edges are in ascending
// token order the list order is the index order of the rule. An edge whose token lies outside [0, V) is skipped: it is left out
// of every count by an explicit test (its e would otherwise tie with an allowed token whose e underflowed to 0), top-k is cut
// against the NUMBER ALLOWED, and the walk falls back to the last kept (or, on a row of NaNs, the first allowed) edge. Every
// index read from the trie is clamped before it is used (csrc/token_step.h): the edge range into [0, n_edges], the child into
// [0, n_nodes) (else the row is sent to the node n_nodes, which ends it at the next step). A row at node == -1 runs the loops
// over V as before.
//
// fvqa_decode_next_pair is the template with PAIR = true (false in the three entries above, in which none of the following
// exists), with and without TRIE: contrastive decoding against a twin row. A workgroup owns a PAIR of rows — b, the positive
// one (the prompt with its clip), and b + n_seq, the negative one (the same ids with the twin's features) — and n_seq counts
// pairs. With lp = l - lse(l) over the whole raw row:
//   P        the plausible set: the allowed tokens (the vocabulary, or the usable edges of the pair's node) whose l+ lies within
//            logf(beta) of the largest allowed l+. ok() asks for it as well, so a token outside P takes no part anywhere, just
//            as an edge outside [0, V) takes none; n_ok = |P| is what top-k is cut against.
//   c        c_i = l+_i + alpha * (lp+_i - lp-_i), computed inside l1() wherever a logit is read: no row of c exists, LDS holds
//            one row of e_i and the bitmap as before, and a row beyond LDS re-reads BOTH rows per pass. alpha == 0, or twin rows
//            of the same bits (whose two lse then have the same bits too), give c_i = l+_i + 0 = l+_i bit for bit.
//   step     pos and done are read from the positive row; the token, pos, done, pos64 and x_next are written to both rows, so
//            the two caches stay in step. logprob stays lp+ of the token; the ticket counts pairs.
//
// fvqa_decode_next_stream is the template with STREAM = true (false in the four entries above, in which none of the following
// exists), with and without TRIE: the token step of in-flight batching (fvqa/stream.py). A row is a SLOT that holds request
// r = req[b] at token index i = pos + 1 - gen_start[b]. A slot whose r lies outside [0, n_req), or whose i lies outside
// [0, min(budget[r], width)), is not live: it becomes done and nothing of any request's results is written. A live slot picks by
// the _ex / _trie rule with the draw at u[i * n_req + r] — the request's own, wherever and whenever it sits —, is stepped as
// before, leaves its token, log-probability and count in the request's result rows, and is also done once i + 1 == budget[r].
//
// fvqa_decode_next_rules is the template with RULES = true (false in the five entries above, in which none of the following
// exists), on the vocabulary alone (TRIE = PAIR = STREAM = false): three more pick rules, include/fvqa.h states them.
//   ban set  X, a second bitmap of V bits behind R's, built once per step from the row's generated ids: the EOS while the token
//            index is below min_new_tokens; with no_repeat_ngram = n the token behind every earlier occurrence, inside the
//            generated ids, of the last n - 1 of them. The view answers ok(i) = false for a banned token — the place where PAIR
//            narrows to the plausible set —, so it enters no maximum, sum, count, tie group or walk, n_ok (what top-k is cut
//            against) counts the others, and a row with none left ends as a trie row at a node without edges does.
//   min-p    e_i >= min_p, with e = 1 at the non-banned maximum: a third prefix of the one order, whole tie groups; the kept set
//            is the shortest of the three. One counting pass behind the nucleus cut (csrc/row_sample.h, MINP).
#include "row_sample.h"
#include "token_step.h"

namespace {

__device__ unsigned g_ticket = 0;

// a view of a row's elements narrowed to those keep(i) admits as well (PAIR: the plausible set), recounted by the caller
template <typename E, typename K>
struct ElemsKept {
  const E& el;
  K keep;
  int N, n_ok, first_ok;
  __device__ __forceinline__ bool ok(int i) const { return el.ok(i) && keep(i); }
  __device__ __forceinline__ int tok(int i) const { return el.tok(i); }
};

// the operands fvqa_decode_next_pair adds (PAIR = true)
struct PairArgs {
  float alpha, beta;
  int32_t* n_plausible;
};

// the operands fvqa_decode_next_stream adds (STREAM = true)
struct StreamArgs {
  const int32_t* req;
  const int32_t* budget;
  int n_req, width;
  int32_t* out_tokens;
  float* out_logprob;
  int32_t* out_n_generated;
};

// the operands fvqa_decode_next_rules adds (RULES = true)
struct RulesArgs {
  float min_p;
  int no_repeat_ngram, min_new_tokens;
};

template <typename T, bool EX, bool TRIE, bool PAIR, bool STREAM, bool RULES>
__global__ __launch_bounds__(NT) void decode_next_k(const float* __restrict__ logits, const float* __restrict__ u_p,
                                                    const T* __restrict__ emb, float temperature, float top_p, int eos_id,
                                                    int stop_at_eos, int64_t* __restrict__ ids, int32_t* __restrict__ pos,
                                                    int32_t* __restrict__ done, T* __restrict__ x_next,
                                                    int32_t* __restrict__ token_out, int32_t* __restrict__ n_kept_out,
                                                    int32_t* __restrict__ n_active, int64_t* __restrict__ pos64, int B, int V,
                                                    int D, int S, int row_in_lds, int vec16, int top_k, float rep,
                                                    const int32_t* __restrict__ gen_start,
                                                    float* __restrict__ logprob_out, unsigned* __restrict__ counter,
                                                    TrieArgs ta, PairArgs pr, StreamArgs sa, RulesArgs ru) {
  const Trie& tr = ta.trie;
  static_assert(EX || !TRIE, "the trie entry extends the EX entry");
  static_assert(EX || !PAIR, "the pair entry extends the EX entry");
  static_assert((EX && !PAIR) || !STREAM, "the stream entry extends the EX entry, one row per slot");
  static_assert((EX && !TRIE && !PAIR && !STREAM) || !RULES, "the rules entry extends the EX entry on the vocabulary");
  extern __shared__ __attribute__((aligned(16))) float erow[];     // the row's e_i (row_in_lds), then the bitmap (EX), then X (RULES)
  __shared__ float redf[4], wtotf[4];
  __shared__ int redi[4], wtoti[4];
  const int b = blockIdx.x, tid = threadIdx.x;
  const float* lg = logits + (size_t)b * V;
  const float* lgn = PAIR ? logits + ((size_t)b + B) * V : nullptr;   // the twin's row (B pairs: rows b and b + B)
  int p = pos[b];
  // a finished row, and one with no room for another token (the reference would index past the end), pick nothing
  bool live = done[b] == 0 && p >= -1 && p + 1 < S;
  int tok = -1, kept = 0;
  int64_t* row_ids = ids + (size_t)b * S;
  // ---- STREAM: the slot's request r and token index ti, every index checked before it is used
  int r = -1, ti = 0, last_of_budget = 0;
  if constexpr (STREAM) {
    r = sa.req[b];
    const long long i = (long long)p + 1 - (long long)gen_start[b];
    bool seated = r >= 0 && r < sa.n_req;
    if (seated) {
      const int bud = sa.budget[r];
      const int lim = bud < sa.width ? bud : sa.width;
      seated = i >= 0 && i < (long long)lim;
      last_of_budget = seated && i + 1 == (long long)bud;
    }
    if (seated) ti = (int)i; else live = false;
  }

  // ---- the row's elements: the vocabulary, or (TRIE, a row at a node) the node's edge list
  int nd = -1;
  if constexpr (TRIE) nd = ta.node[b];
  const RowElems<TRIE> el0 = row_elems<TRIE>(V, tr, live ? nd : -1, redi);
  if (el0.n_ok == 0) live = false;                                 // no children (or a node outside the trie): the row ends
  // ---- PAIR: the plausible set P — the allowed elements whose l+ lies within logf(beta) of the largest allowed l+
  float mxa = 0.f, lbeta = 0.f;
  int n_ok = el0.n_ok, first_ok = el0.first_ok, n_plaus = 0;
  if constexpr (PAIR) {
    if (live) {
      lbeta = logf(pr.beta);                                       // (beta == 0: -inf, every finite logit passes)
      float mx = -INFINITY;
      for (int i = tid; i < el0.N; i += NT)
        if (el0.ok(i)) mx = fmaxf(mx, lg[el0.tok(i)]);
      mxa = block_max_256(mx, redf);
      int c = 0, f = 0x7fffffff;
      for (int i = tid; i < el0.N; i += NT)
        if (el0.ok(i) && lg[el0.tok(i)] - mxa >= lbeta) { c += 1; f = min(f, i); }
      n_ok = n_plaus = block_sum_int(c, redi);
      first_ok = block_min_int(f, redi);
      if (n_ok == 0) live = false;                                 // (a row of NaNs: the pair ends, as at a node without edges)
    }
  }
  // ---- RULES: the ban set X, from the row's generated ids; what is not banned is what takes part (element i = token i)
  const unsigned* ban = nullptr;
  if constexpr (RULES) {
    if (live) {
      unsigned* bw = sample_ban_at(sample_bitmap_at(erow, V, row_in_lds), V, rep != 1.f);
      sample_ban_build(bw, row_ids, gen_start[b], p, V, ru.no_repeat_ngram, ru.min_new_tokens, eos_id);   // (p <= S - 2)
      ban = bw;
      int c = 0, f = 0x7fffffff;
      for (int i = tid; i < V; i += NT)
        if (!sample_banned(bw, i)) { c += 1; f = min(f, i); }
      n_ok = block_sum_int(c, redi);
      first_ok = block_min_int(f, redi);
      if (n_ok == 0) live = false;                                 // (every token banned: the row ends, as at a node without edges)
    }
  }
  auto in_p = [&](int i) -> bool {                                 // (always, without PAIR and RULES)
    if constexpr (PAIR) return lg[el0.tok(i)] - mxa >= lbeta;
    if constexpr (RULES) return !sample_banned(ban, i);
    return true;
  };
  const ElemsKept<RowElems<TRIE>, decltype(in_p)> el{el0, in_p, el0.N, n_ok, first_ok};   // what takes part in the pick
  const bool use_lds = row_in_lds && (!TRIE || el.N <= V);         // (a list longer than V: recomputed, never past the row)

  // ---- EX: the raw row's lse; the bitmap of the ids generated so far
  float lse = 0.f, lse_n = 0.f;
  const bool pen = EX && rep != 1.f;
  const SampleLds sl{erow, sample_bitmap_at(erow, V, row_in_lds), redf, wtotf, redi, wtoti};
  if constexpr (EX) {
    if (live) lse = row_lse(lg, V, redf);
    if constexpr (PAIR) {
      if (live) lse_n = row_lse(lgn, V, redf);
    }
    if (live && pen) sample_bitmap_build(sl.bm, row_ids, gen_start[b], p, V);   // (p <= S - 2)
  }
  auto l1 = [&](int t) -> float {                                  // the logit the pick sees at token t
    float v = lg[t];
    if constexpr (PAIR) v = v + pr.alpha * ((v - lse) - (lgn[t] - lse_n));   // c_t in place of l_t
    if constexpr (EX) {
      if (pen) v = sample_penalised(v, t, sl.bm, rep);
    }
    return v;
  };

  // ---- the pick (csrc/row_sample.h) -> `sel`, the element picked
  int sel = -1;
  if (live && temperature == 0.f) {
    sel = row_pick_greedy(el, l1, redf, redi);
    kept = 1;
  } else if (live) {
    const float u = STREAM ? u_p[(size_t)ti * sa.n_req + r] : u_p[b];
    sel = row_pick_sampled<EX, RULES>(el, l1, use_lds, sl, u, temperature, top_p, top_k, kept, RULES ? ru.min_p : 0.f);
  }
  int child = -1;
  if (live) {
    tok = el0.tok(sel);
    if constexpr (TRIE) {
      if (el0.cons) child = tr.child(el0.ec[sel]);
    }
  }

  // ---- step the row
  int now_done = done[b] != 0 ? 1 : 0;
  int src;
  if (live) {
    p += 1;
    src = tok;
    if (stop_at_eos && tok == eos_id) now_done = 1;
    if constexpr (STREAM) {
      if (last_of_budget) now_done = 1;                            // (the token is still written)
    }
  } else {
    now_done = 1;
    src = valid_token(row_ids[valid_pos(p, S)], V);
  }
  __syncthreads();                                                 // (every read of done / pos / ids above is over)
  if (tid == 0) {
    if (live) {
      row_ids[p] = tok;
      pos[b] = p;
    }
    done[b] = now_done;
    if (pos64) pos64[b] = live ? p : valid_pos(p, S);
    if constexpr (PAIR) {                                          // the twin row is stepped, or left, like the positive one
      if (live) ids[((size_t)b + B) * S + p] = tok;
      pos[b + B] = p;
      done[b + B] = now_done;
      if (pos64) pos64[b + B] = live ? p : valid_pos(p, S);
      pr.n_plausible[b] = live ? n_plaus : 0;
    }
    token_out[b] = tok;
    n_kept_out[b] = kept;
    if constexpr (TRIE) {
      if (live && el0.cons) ta.node[b] = child;
    }
    if constexpr (EX) logprob_out[b] = live ? lg[tok] - lse : 0.f;
    if constexpr (STREAM) {
      if (live) {                                                  // the request's own result row, at its own token index
        sa.out_tokens[(size_t)r * sa.width + ti] = tok;
        if (sa.out_logprob) sa.out_logprob[(size_t)r * sa.width + ti] = lg[tok] - lse;
        sa.out_n_generated[r] = ti + 1;
      }
    }
    ticket_arrive(EX ? counter : &g_ticket, n_active, B, !now_done);
  }
  // ---- the next input row
  const T* erow_src = emb + (size_t)src * D;
  T* dst = x_next + (size_t)b * D;
  copy_row(dst, erow_src, D, vec16, tid);
  if constexpr (PAIR) copy_row(dst + (size_t)B * D, erow_src, D, vec16, tid);   // the twin's row
}

// the operands fvqa_decode_next_ex adds (the old entry passes none: EX = false)
struct ExArgs {
  int top_k;
  float rep;
  const int32_t* gen_start;
  float* logprob;
  unsigned* counter;
};

template <typename T, bool EX, bool TRIE, bool PAIR = false, bool STREAM = false, bool RULES = false>
int launch(const float* logits, const float* u, const void* emb, float temperature, float top_p, int eos_id, int stop_at_eos,
           int64_t* ids, int32_t* pos, int32_t* done, void* x_next, int32_t* token, int32_t* n_kept, int32_t* n_active,
           int64_t* pos64, int B, int V, int D, int S, ExArgs ex, TrieArgs tr, hipStream_t st,
           PairArgs pr = PairArgs{0.f, 0.f, nullptr},
           StreamArgs sa = StreamArgs{nullptr, nullptr, 0, 0, nullptr, nullptr, nullptr}, RulesArgs ru = RulesArgs{0.f, 0, 0}) {
  int in_lds, fits;                                                // (without EX rep is 1: no bitmap)
  const size_t lds = fvqa_sample_lds(V, ex.rep, temperature > 0.f, &in_lds, &fits, RULES);
  if (!fits) return FVQA_ESHAPE;                                   // (a vocabulary beyond 1.2 million ids under a penalty)
  fvqa_sample_lds_limit<decode_next_k<T, EX, TRIE, PAIR, STREAM, RULES>>((EX ? 1 : 0) + (RULES ? 1 : 0));
  const int vec16 = fvqa_vec16((size_t)D * sizeof(T), emb, x_next);   // (PAIR: the twin half follows B * D elements on, whole rows)
  hipLaunchKernelGGL((decode_next_k<T, EX, TRIE, PAIR, STREAM, RULES>), dim3(B), dim3(NT), lds, st, logits, u, (const T*)emb, temperature,
                     top_p, eos_id, stop_at_eos, ids, pos, done, (T*)x_next, token, n_kept, n_active, pos64, B, V, D, S, in_lds,
                     vec16, ex.top_k, ex.rep, ex.gen_start, ex.logprob, ex.counter, tr, pr, sa, ru);
  FVQA_CHECK_LAUNCH();
  return FVQA_OK;
}

// the operand checks the entries share; then the launch
template <bool EX, bool TRIE = false, bool PAIR = false, bool STREAM = false, bool RULES = false>
int checked_launch(const float* logits, const float* u, const void* emb, float temperature, float top_p, int eos_id,
                   int stop_at_eos, int64_t* ids, int32_t* pos, int32_t* done, void* x_next, int32_t* token, int32_t* n_kept,
                   int32_t* n_active, int64_t* pos64, int n_seq, int vocab, int dim, int seq_len, int dtype, ExArgs ex,
                   void* stream, TrieArgs tr = TrieArgs{},
                   PairArgs pr = PairArgs{0.f, 0.f, nullptr},
                   StreamArgs sa = StreamArgs{nullptr, nullptr, 0, 0, nullptr, nullptr, nullptr},
                   RulesArgs ru = RulesArgs{0.f, 0, 0}) {
  if (!logits || !emb || !ids || !pos || !done || !x_next || !token || !n_kept || !n_active) return FVQA_EINVAL;
  if (EX && (!ex.gen_start || !ex.logprob || !ex.counter)) return FVQA_EINVAL;
  if (TRIE && fvqa_trie_given(tr.node, tr.trie.node_first, tr.trie.edge_token, tr.trie.edge_child) != 1) return FVQA_EINVAL;
  if (!fvqa_dtype_ok(dtype)) return FVQA_EINVAL;
  if (!(temperature >= 0.f)) return FVQA_EINVAL;                   // (a NaN fails the comparison)
  if (!(top_p > 0.f && top_p <= 1.f)) return FVQA_EINVAL;
  if (EX && (!(ex.rep >= 1.f) || ex.top_k < 0)) return FVQA_EINVAL;
  if (PAIR && (!pr.n_plausible || !(pr.alpha >= 0.f) || !(pr.beta >= 0.f && pr.beta <= 1.f))) return FVQA_EINVAL;
  if (RULES && (!(ru.min_p >= 0.f && ru.min_p < 1.f) || ru.no_repeat_ngram < 0 || ru.min_new_tokens < 0)) return FVQA_EINVAL;
  if (RULES && ru.min_new_tokens > 0 && !stop_at_eos) return FVQA_EINVAL;   // (the EOS ends nothing: no length to hold back)
  if (temperature > 0.f && !u) return FVQA_EINVAL;
  if (STREAM && (!sa.req || !sa.budget || !sa.out_tokens || !sa.out_n_generated)) return FVQA_EINVAL;
  if (STREAM && (sa.n_req <= 0 || sa.width <= 0)) return FVQA_ESHAPE;
  if (n_seq <= 0 || vocab <= 0 || dim <= 0 || seq_len <= 0) return FVQA_ESHAPE;
  if (n_seq > 65535) return FVQA_ESHAPE;                           // (the ticket word counts arrivals in 16 bits)
  if (PAIR && 2 * (int64_t)n_seq > 65535) return FVQA_ESHAPE;      // (n_seq pairs are 2 * n_seq rows of the token loop)
  if (TRIE && (tr.trie.n_nodes <= 0 || tr.trie.n_edges < 0)) return FVQA_ESHAPE;
  if (!fvqa_aligned(fvqa_dtype_size(dtype), emb, x_next) || !fvqa_aligned(4, logits, u, pos, done, token, n_kept, n_active) ||
      !fvqa_aligned(8, ids, pos64) || !fvqa_aligned(4, ex.gen_start, ex.logprob, ex.counter) ||
      !fvqa_aligned(4, tr.node, tr.trie.node_first, tr.trie.edge_token, tr.trie.edge_child) || !fvqa_aligned(4, pr.n_plausible) ||
      !fvqa_aligned(4, sa.req, sa.budget, sa.out_tokens, sa.out_logprob, sa.out_n_generated))
    return FVQA_EALIGN;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == FVQA_H16)
    return launch<bf16_t, EX, TRIE, PAIR, STREAM, RULES>(logits, u, emb, temperature, top_p, eos_id, stop_at_eos, ids, pos, done,
                                                         x_next, token, n_kept, n_active, pos64, n_seq, vocab, dim, seq_len, ex,
                                                         tr, st, pr, sa, ru);
  return launch<float, EX, TRIE, PAIR, STREAM, RULES>(logits, u, emb, temperature, top_p, eos_id, stop_at_eos, ids, pos, done,
                                                      x_next, token, n_kept, n_active, pos64, n_seq, vocab, dim, seq_len, ex, tr,
                                                      st, pr, sa, ru);
}

}  // namespace

extern "C" int fvqa_decode_next(const float* logits, const float* u, const void* emb, float temperature, float top_p,
                                int eos_id, int stop_at_eos, int64_t* ids, int32_t* pos, int32_t* done, void* x_next,
                                int32_t* token, int32_t* n_kept, int32_t* n_active, int64_t* pos64, int n_seq, int vocab,
                                int dim, int seq_len, int dtype, void* stream) {
  return checked_launch<false>(logits, u, emb, temperature, top_p, eos_id, stop_at_eos, ids, pos, done, x_next, token, n_kept,
                               n_active, pos64, n_seq, vocab, dim, seq_len, dtype, ExArgs{0, 1.f, nullptr, nullptr, nullptr},
                               stream);
}

extern "C" int fvqa_decode_next_ex(const float* logits, const float* u, const void* emb, float temperature, float top_p,
                                   int top_k, float repetition_penalty, int eos_id, int stop_at_eos, int64_t* ids, int32_t* pos,
                                   int32_t* done, const int32_t* gen_start, void* x_next, int32_t* token, int32_t* n_kept,
                                   float* logprob, int32_t* n_active, uint32_t* counter, int64_t* pos64, int n_seq, int vocab,
                                   int dim, int seq_len, int dtype, void* stream) {
  return checked_launch<true>(logits, u, emb, temperature, top_p, eos_id, stop_at_eos, ids, pos, done, x_next, token, n_kept,
                              n_active, pos64, n_seq, vocab, dim, seq_len, dtype,
                              ExArgs{top_k, repetition_penalty, gen_start, logprob, counter}, stream);
}

extern "C" int fvqa_decode_next_rules(const float* logits, const float* u, const void* emb, float temperature, float top_p,
                                      int top_k, float repetition_penalty, int eos_id, int stop_at_eos, int64_t* ids,
                                      int32_t* pos, int32_t* done, const int32_t* gen_start, void* x_next, int32_t* token,
                                      int32_t* n_kept, float* logprob, int32_t* n_active, uint32_t* counter, int64_t* pos64,
                                      int n_seq, int vocab, int dim, int seq_len, int dtype, void* stream, float min_p,
                                      int no_repeat_ngram, int min_new_tokens) {
  return checked_launch<true, false, false, false, true>(
      logits, u, emb, temperature, top_p, eos_id, stop_at_eos, ids, pos, done, x_next, token, n_kept, n_active, pos64, n_seq,
      vocab, dim, seq_len, dtype, ExArgs{top_k, repetition_penalty, gen_start, logprob, counter}, stream, TrieArgs{},
      PairArgs{0.f, 0.f, nullptr}, StreamArgs{nullptr, nullptr, 0, 0, nullptr, nullptr, nullptr},
      RulesArgs{min_p, no_repeat_ngram, min_new_tokens});
}

extern "C" int fvqa_decode_next_trie(const float* logits, const float* u, const void* emb, float temperature, float top_p,
                                     int top_k, float repetition_penalty, int eos_id, int stop_at_eos, int64_t* ids,
                                     int32_t* pos, int32_t* done, const int32_t* gen_start, void* x_next, int32_t* token,
                                     int32_t* n_kept, float* logprob, int32_t* n_active, uint32_t* counter, int64_t* pos64,
                                     int32_t* node, const int32_t* node_first, const int32_t* edge_token,
                                     const int32_t* edge_child, int n_nodes, int n_edges, int n_seq, int vocab, int dim,
                                     int seq_len, int dtype, void* stream) {
  return checked_launch<true, true>(logits, u, emb, temperature, top_p, eos_id, stop_at_eos, ids, pos, done, x_next, token,
                                    n_kept, n_active, pos64, n_seq, vocab, dim, seq_len, dtype,
                                    ExArgs{top_k, repetition_penalty, gen_start, logprob, counter}, stream,
                                    TrieArgs{node, {node_first, edge_token, edge_child, n_nodes, n_edges}});
}

extern "C" int fvqa_decode_next_pair(const float* logits, const float* u, const void* emb, float temperature, float top_p,
                                     int top_k, float repetition_penalty, float alpha, float beta, int eos_id, int stop_at_eos,
                                     int64_t* ids, int32_t* pos, int32_t* done, const int32_t* gen_start, void* x_next,
                                     int32_t* token, int32_t* n_kept, int32_t* n_plausible, float* logprob, int32_t* n_active,
                                     uint32_t* counter, int64_t* pos64, int32_t* node, const int32_t* node_first,
                                     const int32_t* edge_token, const int32_t* edge_child, int n_nodes, int n_edges, int n_seq,
                                     int vocab, int dim, int seq_len, int dtype, void* stream) {
  const ExArgs ex{top_k, repetition_penalty, gen_start, logprob, counter};
  const PairArgs pr{alpha, beta, n_plausible};
  if (fvqa_trie_given(node, node_first, edge_token, edge_child) == 0)   // no trie at all: the pairs pick from the vocabulary
    return checked_launch<true, false, true>(logits, u, emb, temperature, top_p, eos_id, stop_at_eos, ids, pos, done, x_next,
                                             token, n_kept, n_active, pos64, n_seq, vocab, dim, seq_len, dtype, ex, stream,
                                             TrieArgs{}, pr);
  return checked_launch<true, true, true>(logits, u, emb, temperature, top_p, eos_id, stop_at_eos, ids, pos, done, x_next, token,
                                          n_kept, n_active, pos64, n_seq, vocab, dim, seq_len, dtype, ex, stream,
                                          TrieArgs{node, {node_first, edge_token, edge_child, n_nodes, n_edges}}, pr);
}

extern "C" int fvqa_decode_next_stream(const float* logits, const float* u, const void* emb, float temperature, float top_p,
                                       int top_k, float repetition_penalty, int eos_id, int stop_at_eos, int64_t* ids,
                                       int32_t* pos, int32_t* done, const int32_t* gen_start, void* x_next, int32_t* token,
                                       int32_t* n_kept, float* logprob, int32_t* n_active, uint32_t* counter, int64_t* pos64,
                                       int32_t* node, const int32_t* node_first, const int32_t* edge_token,
                                       const int32_t* edge_child, int n_nodes, int n_edges, const int32_t* req,
                                       const int32_t* budget, int n_req, int width, int32_t* out_tokens, float* out_logprob,
                                       int32_t* out_n_generated, int n_seq, int vocab, int dim, int seq_len, int dtype,
                                       void* stream) {
  const ExArgs ex{top_k, repetition_penalty, gen_start, logprob, counter};
  const PairArgs pr{0.f, 0.f, nullptr};
  const StreamArgs sa{req, budget, n_req, width, out_tokens, out_logprob, out_n_generated};
  if (fvqa_trie_given(node, node_first, edge_token, edge_child) == 0)   // no trie at all: the slots pick from the vocabulary
    return checked_launch<true, false, false, true>(logits, u, emb, temperature, top_p, eos_id, stop_at_eos, ids, pos, done,
                                                    x_next, token, n_kept, n_active, pos64, n_seq, vocab, dim, seq_len, dtype, ex,
                                                    stream, TrieArgs{}, pr, sa);
  return checked_launch<true, true, false, true>(logits, u, emb, temperature, top_p, eos_id, stop_at_eos, ids, pos, done, x_next,
                                                 token, n_kept, n_active, pos64, n_seq, vocab, dim, seq_len, dtype, ex, stream,
                                                 TrieArgs{node, {node_first, edge_token, edge_child, n_nodes, n_edges}}, pr, sa);
}
