// The token step of draft-and-verify greedy decoding (fvqa/generate.py: generate(lookahead=T)): everything between the LM head
// and the next pass's first RMSNorm in ONE launch, one 256-thread workgroup per sequence. A pass carries up to T rows per
// sequence — the last committed token and a draft of what follows it — and this step keeps every draft token the model would
// have picked itself, so that the ids are greedy's, token for token (include/fvqa.h fvqa_spec_step states the rule).
//
//   verify   row i of the sequence's logits is scanned only if the drafts 1..i were all accepted (csrc/token_step.h row_verify:
//            the largest logit, lowest index on exact ties, then the row's lse for the log-probability — fvqa_decode_next_ex's
//            rule 5: maximum, sum of expf in strided order, shuffles, the four waves in order). The token committed at row i is
//            argmax L_i whether it was drafted or not — a draft only decides whether row i + 1 may be used —, so there is one
//            commit loop and no separate "fresh token" case.
//   commit   thread 0 writes the id row; the committed tokens also stay in LDS, so that the draft below never reads back what
//            this launch wrote to global memory.
//   draft    given drafts: a slice of the caller's (n_seq, max_new_tokens) array at the row's n_generated. Prompt lookup: the
//            longest suffix of the committed ids (g = G down to 1 tokens) that occurs earlier in the row, the most recent
//            occurrence, found by all threads over the match ends e and one block-wide maximum; the draft is what followed it.
//            Every index is clamped, every id that would be fed on is checked against [0, vocab).
//   outputs  the rows of the next pass (embeddings; zeros behind the draft), start / len for fvqa_attn_suffix_append, the step's
//            tokens and log-probabilities, the count of running rows through the caller's ticket word (an INTEGER atomic; the
//            workgroup that arrives last writes the count and puts the word back to zero: csrc/token_step.h).
// fvqa_spec_step_sample is the kernel template with SAMPLE = true (false in fvqa_spec_step, whose instantiation holds none of
// the sampling code): draft-and-verify under sampling. The pick at row i is not the arg-max but
// csrc/row_sample.h's row_sample — the one sampled pick, decode_next_k's own, on the vocabulary with the draw of the token's index,
// u[(n_generated + i) * n_seq + n] — and a draft is accepted iff it equals the token sampled in front of it: for a point-mass
// draft that is the rejection rule of speculative sampling, so the ids are the plain sampled call's. The bitmap of the
// repetition penalty is built once per step and gains one bit per commit. Everything behind the pick is the code above.
// No float atomics, fixed summation orders: two launches on the same inputs give the same bits.
#include "row_sample.h"
#include "token_step.h"

namespace {

constexpr int TMAX = 16;                 // rows of a sequence per pass (fvqa_attn_suffix's suffix_len limit)
constexpr int GMAX = 4;                  // the longest n-gram the prompt lookup matches

template <typename T, bool SAMPLE>
__global__ __launch_bounds__(NT) void spec_step_k(const float* __restrict__ logits, const T* __restrict__ emb,
                                                  const int32_t* __restrict__ draft_tokens, int G, int eos_id, int stop_at_eos,
                                                  int max_new, int64_t* __restrict__ ids, int32_t* __restrict__ pos,
                                                  int32_t* __restrict__ done, int32_t* __restrict__ n_generated,
                                                  int32_t* __restrict__ w, int32_t* __restrict__ len_p,
                                                  int32_t* __restrict__ start_p, T* __restrict__ x_next,
                                                  int32_t* __restrict__ token_out, float* __restrict__ logprob_out,
                                                  int32_t* __restrict__ n_committed, int32_t* __restrict__ n_drafted,
                                                  int32_t* __restrict__ n_active, unsigned* __restrict__ counter,
                                                  int64_t* __restrict__ pos64, int B, int Tn, int V, int D, int S, int vec16,
                                                  SampleArgs sa) {
  extern __shared__ __attribute__((aligned(16))) float erow[];     // SAMPLE: the row's e_i (row_in_lds), then the bitmap
  __shared__ float redf[4];
  __shared__ int redi[4];
  __shared__ float wtotf[4];             // (SAMPLE: the scans of the walk)
  __shared__ int wtoti[4];
  __shared__ int cm[TMAX];               // the tokens committed by this step, in order
  __shared__ int wn[TMAX];               // the rows of the next pass: w'_0 .. w'_{m'-1}
  __shared__ int s_len;
  const int b = blockIdx.x, tid = threadIdx.x;
  int64_t* row_ids = ids + (size_t)b * S;
  const int32_t* wrow = w + (size_t)b * Tn;
  const int p0 = pos[b];
  int ngen = n_generated[b];
  const int m = verify_rows(len_p[b], Tn);
  const bool live = verify_live(done[b], p0, S, ngen, max_new);
  int now_done = live ? 0 : 1;
  int p = p0, nc = 0;
  // ---- SAMPLE: the picks' scratch; under a penalty the bitmap of the ids generated before this step
  SampleLds sl{};
  bool pen = false;
  if constexpr (SAMPLE) {
    sl = SampleLds{erow, sample_bitmap_at(erow, V, sa.row_in_lds), redf, wtotf, redi, wtoti};
    pen = sa.rep != 1.f;
    if (live && pen) sample_bitmap_build(sl.bm, row_ids, sa.gen_start[b], p0, V);
  }

  // ---- verify and commit: row i is scanned only while the drafts keep being accepted
  if (live) {
    for (int i = 0; i < m; ++i) {
      const float* lg = logits + ((size_t)b * Tn + i) * V;
      float lse;
      int g, kept = 1;
      if constexpr (SAMPLE)                                        // the sampled pick, with the draw of this token's index
        g = row_sample(lg, V, sample_draw(sa.u, ngen, max_new, B, b), sa, pen, sl, kept, lse);
      else
        g = row_verify(lg, V, redf, redi, lse);
      p += 1;
      ngen += 1;
      if (tid == 0) {
        cm[nc] = g;
        row_ids[p] = g;                                            // (p <= S - 1: checked before every commit)
        token_out[(size_t)b * Tn + nc] = g;
        logprob_out[(size_t)b * Tn + nc] = lg[g] - lse;
        if constexpr (SAMPLE) sa.n_kept[(size_t)b * Tn + nc] = kept;
      }
      if constexpr (SAMPLE) {
        if (pen) sample_bitmap_add(sl.bm, g);                      // row i + 1 sees what rows 0 .. i committed
      }
      nc += 1;
      if (stop_at_eos && g == eos_id) { now_done = 1; break; }
      if (ngen >= max_new) { now_done = 1; break; }
      if (p + 1 >= S || i + 1 >= m) break;
      if (wrow[i + 1] != g) break;                                 // the draft of row i + 1 is not what the model picks
    }
  }
  __syncthreads();                                                 // (cm is published; every read of pos / done / len is over)

  // ---- the next pass: w'_0, the room m', the draft
  const int P = p;                                                 // the row's position now (live: 0 <= P <= S - 1)
  const int at = valid_pos(P, S);
  int m2 = 0;
  if (!now_done) {
    m2 = min(Tn, min(max_new - ngen, S - 1 - P));
    if (m2 < 0) m2 = 0;
  }
  // id j of the row, 0 <= j <= P: what this step committed comes from LDS
  auto id_at = [&](int j) -> int64_t { return j > p0 ? (int64_t)cm[j - p0 - 1] : row_ids[j]; };
  int e_best = -1;
  if (m2 >= 2 && !draft_tokens) {
    for (int g = min(G, P); g >= 1; --g) {                         // an occurrence ends at e with g - 1 <= e < P
      int best = -1;
      for (int e = g - 1 + tid; e < P; e += NT) {
        bool same = true;
        for (int k = 0; k < g; ++k) same = same && id_at(e - k) == id_at(P - k);
        if (same) best = e;                                        // (ascending e: the thread's most recent match)
      }
      best = block_max_int(best, redi);
      if (best >= 0) { e_best = best; break; }
    }
  }
  if (tid == 0) {
    wn[0] = live ? cm[nc - 1] : valid_token(row_ids[at], V);
    int nd = 0;
    if (m2 >= 2) {
      if (draft_tokens) {
        for (int i = 1; i < m2; ++i) {
          const int at_d = ngen + i - 1;
          if (at_d < 0 || at_d >= max_new) break;
          const int t = draft_tokens[(size_t)b * max_new + at_d];
          if ((unsigned)t >= (unsigned)V) break;
          wn[i] = t;
          nd += 1;
        }
      } else if (e_best >= 0) {
        const int lim = min(m2 - 1, P - e_best);
        for (int i = 1; i <= lim; ++i) {
          const int64_t t = id_at(e_best + i);
          if (t < 0 || t >= V) break;
          wn[i] = (int)t;
          nd += 1;
        }
      }
    }
    const int mlen = m2 >= 1 ? 1 + nd : 0;
    s_len = mlen;
    // ---- the row's state (a row that committed nothing keeps its ids, pos, n_generated and w) and the step's results
    if (live) {
      pos[b] = p;
      n_generated[b] = ngen;
      for (int j = 0; j < Tn; ++j) w[(size_t)b * Tn + j] = j < mlen ? wn[j] : -1;
    }
    done[b] = now_done;
    len_p[b] = mlen;
    start_p[b] = at;
    if (pos64) pos64[b] = at;
    verify_pad(token_out, logprob_out, (size_t)b * Tn, nc, Tn);
    if constexpr (SAMPLE) {
      for (int j = nc; j < Tn; ++j) sa.n_kept[(size_t)b * Tn + j] = 0;
    }
    n_committed[b] = nc;
    n_drafted[b] = live ? m - 1 : 0;
    ticket_arrive(counter, n_active, B, !now_done);
  }
  __syncthreads();
  // ---- the next pass's input rows: emb[w'_j] for j < m' (row 0 always: a row that feeds nothing stays a valid row), zeros behind
  next_pass_rows(x_next, emb, b, Tn, D, vec16, tid, s_len < 1 ? 1 : s_len, [&](int j) { return wn[j]; });
}

// the operand checks and the launch of both entries; sa: the operands fvqa_spec_step_sample adds (SAMPLE = true), else NULL
int spec_step_launch(const float* logits, const void* emb, const int32_t* draft_tokens, int lookup_ngram, int eos_id,
                     int stop_at_eos, int max_new_tokens, int64_t* ids, int32_t* pos, int32_t* done, int32_t* n_generated,
                     int32_t* w, int32_t* len, int32_t* start, void* x_next, int32_t* token, float* logprob, int32_t* n_committed,
                     int32_t* n_drafted, int32_t* n_active, uint32_t* counter, int64_t* pos64, int n_seq, int lookahead, int vocab,
                     int dim, int seq_len, int dtype, void* stream, const SampleArgs* sa) {
  if (!logits || !emb || !ids || !pos || !done || !n_generated || !w || !len || !start || !x_next || !token || !logprob ||
      !n_committed || !n_drafted || !n_active || !counter)
    return FVQA_EINVAL;
  if (!fvqa_dtype_ok(dtype)) return FVQA_EINVAL;
  if (!draft_tokens && (lookup_ngram < 1 || lookup_ngram > GMAX)) return FVQA_EINVAL;
  if (const int rc = fvqa_sample_args_ok(sa); rc != FVQA_OK) return rc;
  if (n_seq <= 0 || lookahead <= 0 || vocab <= 0 || dim <= 0 || seq_len <= 0 || max_new_tokens <= 0) return FVQA_ESHAPE;
  if (lookahead > TMAX || n_seq > 65535 || (int64_t)n_seq * lookahead > 65535) return FVQA_ESHAPE;   // (the ticket counts
                                                                   // arrivals in 16 bits; the pass's rows are a grid dimension)
  if (!fvqa_aligned(fvqa_dtype_size(dtype), emb, x_next) ||
      !fvqa_aligned(4, logits, draft_tokens, pos, done, n_generated, w, len, start, token, logprob, n_committed, n_drafted,
                    n_active, counter) ||
      !fvqa_aligned(8, ids, pos64))
    return FVQA_EALIGN;
  hipStream_t st = (hipStream_t)stream;
  SampleArgs s;
  size_t lds;
  if (const int rc = fvqa_sample_launch_args(sa, vocab, &s, &lds); rc != FVQA_OK) return rc;
  fvqa_by_dtype(dtype, [&](auto* t) {
    using T = std::remove_pointer_t<decltype(t)>;
    const int vec16 = fvqa_vec16(dim * sizeof(T), emb, x_next);
    auto launch = [&](auto sample) {                               // SAMPLE = sample.value
      constexpr bool SAMPLE = decltype(sample)::value;
      if constexpr (SAMPLE) fvqa_sample_lds_limit<spec_step_k<T, true>>(true);
      hipLaunchKernelGGL((spec_step_k<T, SAMPLE>), dim3(n_seq), dim3(NT), lds, st, logits, (const T*)emb, draft_tokens,
                         lookup_ngram, eos_id, stop_at_eos, max_new_tokens, ids, pos, done, n_generated, w, len, start,
                         (T*)x_next, token, logprob, n_committed, n_drafted, n_active, counter, pos64, n_seq, lookahead, vocab,
                         dim, seq_len, vec16, s);
    };
    if (sa) launch(std::true_type{});
    else launch(std::false_type{});
  });
  FVQA_CHECK_LAUNCH();
  return FVQA_OK;
}

}  // namespace

extern "C" int fvqa_spec_step(const float* logits, const void* emb, const int32_t* draft_tokens, int lookup_ngram, int eos_id,
                              int stop_at_eos, int max_new_tokens, int64_t* ids, int32_t* pos, int32_t* done,
                              int32_t* n_generated, int32_t* w, int32_t* len, int32_t* start, void* x_next, int32_t* token,
                              float* logprob, int32_t* n_committed, int32_t* n_drafted, int32_t* n_active, uint32_t* counter,
                              int64_t* pos64, int n_seq, int lookahead, int vocab, int dim, int seq_len, int dtype,
                              void* stream) {
  return spec_step_launch(logits, emb, draft_tokens, lookup_ngram, eos_id, stop_at_eos, max_new_tokens, ids, pos, done,
                          n_generated, w, len, start, x_next, token, logprob, n_committed, n_drafted, n_active, counter, pos64,
                          n_seq, lookahead, vocab, dim, seq_len, dtype, stream, nullptr);
}

extern "C" int fvqa_spec_step_sample(const float* logits, const float* u, const void* emb, const int32_t* draft_tokens,
                                     int lookup_ngram, float temperature, float top_p, int top_k, float repetition_penalty,
                                     int eos_id, int stop_at_eos, int max_new_tokens, int64_t* ids, int32_t* pos, int32_t* done,
                                     int32_t* n_generated, const int32_t* gen_start, int32_t* w, int32_t* len, int32_t* start,
                                     void* x_next, int32_t* token, int32_t* n_kept, float* logprob, int32_t* n_committed,
                                     int32_t* n_drafted, int32_t* n_active, uint32_t* counter, int64_t* pos64, int n_seq,
                                     int lookahead, int vocab, int dim, int seq_len, int dtype, void* stream) {
  const SampleArgs sa{u, temperature, top_p, top_k, repetition_penalty, gen_start, n_kept, 0};
  return spec_step_launch(logits, emb, draft_tokens, lookup_ngram, eos_id, stop_at_eos, max_new_tokens, ids, pos, done,
                          n_generated, w, len, start, x_next, token, logprob, n_committed, n_drafted, n_active, counter, pos64,
                          n_seq, lookahead, vocab, dim, seq_len, dtype, stream, &sa);
}
