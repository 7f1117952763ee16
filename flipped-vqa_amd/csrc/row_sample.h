// The sampled row pick of the draft-and-verify steps (csrc/spec.hip, csrc/treespec.hip with SAMPLE = true): rules 1 to 5 of
// fvqa_decode_next_ex (include/fvqa.h) on ONE raw logits row, by the whole 256-thread workgroup, with one draw — the rule
// csrc/sample.hip's decode_next_k<T, EX = true> applies to an unconstrained row, restated here operation for operation (the same
// strided and contiguous summation orders, the same two bisections over bit patterns, the same tie group and index-order walk)
// so that a step of one row per pass gives fvqa_decode_next_ex's bits. The two kernels share the block reductions and scans of
// csrc/token_step.h; csrc/sample.hip does not include this header.
//
// A step calls the pick up to 16 (chain) or 32 (tree walk) times in sequence. What the calls share:
//   LDS      one dynamic block: the row of e_i (4 * V bytes, when they fit: row_in_lds), then the bitmap of V bits on a 16-byte
//            boundary. Every pick rewrites the row; the block reductions at the end of a pick are the barrier in front of the next.
//   bitmap   R, the ids generated so far: built once per step from ids[gen_start .. pos] (sample_bitmap_build), one bit more
//            after every commit of the step (sample_bitmap_add), so that row i + 1 sees the tokens rows 0 .. i committed. Only
//            under a penalty (rep != 1): without one no bitmap exists and none is read.
//   draws    u (max_new_tokens, n_seq): token index t of sequence n reads u[t * n_seq + n] (sample_draw; the index is clamped).
#pragma once
#include "token_step.h"

namespace {

constexpr size_t SAMPLE_ROW_LDS_MAX = 144 * 1024;                   // csrc/sample.hip ROW_LDS_MAX: the same rows live in LDS
constexpr size_t SAMPLE_BITMAP_LDS_MAX = SAMPLE_ROW_LDS_MAX / 32;   // the bitmap of the largest row that lives in LDS

// the operands the sampled entries add to the entry each extends
struct SampleArgs {
  const float* u;
  float temperature, top_p;
  int top_k;
  float rep;
  const int32_t* gen_start;
  int32_t* n_kept;
  int row_in_lds;
};

// the scratch of a workgroup's picks: the reductions' words in static LDS, the row and the bitmap in the dynamic block
struct SampleLds {
  float* erow;
  unsigned* bm;
  float *redf, *wtotf;
  int *redi, *wtoti;
};

// the bitmap's place in the dynamic block (behind the row when the row lives there)
__device__ __forceinline__ unsigned* sample_bitmap_at(float* erow, int V, int row_in_lds) {
  return reinterpret_cast<unsigned*>(erow) + (row_in_lds ? ((V + 3) & ~3) : 0);
}
// R of a row before the step: the distinct ids at positions max(g0, 0) .. p (p <= S - 2: the row is live)
__device__ __forceinline__ void sample_bitmap_build(unsigned* bm, const int64_t* row_ids, int g0, int p, int V) {
  const int tid = threadIdx.x;
  for (int i = tid; i < ((V + 31) >> 5); i += NT) bm[i] = 0u;
  __syncthreads();
  for (int j = (g0 < 0 ? 0 : g0) + tid; j <= p; j += NT) {
    const int64_t t = row_ids[j];
    if (t >= 0 && t < V) atomicOr(&bm[t >> 5], 1u << (t & 31));
  }
  __syncthreads();
}
// ... and one committed token more (0 <= t < V: a pick), seen by the next pick of the step; every thread calls this
__device__ __forceinline__ void sample_bitmap_add(unsigned* bm, int t) {
  if (threadIdx.x == 0) bm[t >> 5] |= 1u << (t & 31);
  __syncthreads();
}

// the draw of token index t of sequence n
__device__ __forceinline__ float sample_draw(const float* u, int t, int max_new, int n_seq, int n) {
  const int tc = t < 0 ? 0 : (t >= max_new ? max_new - 1 : t);
  return u[(size_t)tc * n_seq + n];
}

// The pick: rules 1 to 5 on the raw row lg (V logits) with the draw u -> the token; kept = n_kept, lse = the raw row's
// m + log(sum exp(l - m)) (row_lse). pen: the bitmap holds R and rep != 1.
__device__ __forceinline__ int row_sample(const float* lg, int V, float u, float temperature, float top_p, int top_k, float rep,
                                          bool pen, int use_lds, const SampleLds& s, int& kept, float& lse) {
  const int tid = threadIdx.x;
  const int N = V;
  float* erow = s.erow;
  const unsigned* bm = s.bm;
  float* redf = s.redf;
  int* redi = s.redi;
  lse = row_lse(lg, V, redf);
  auto l1 = [&](int i) -> float {                                  // the logit the pick sees
    float v = lg[i];
    if (pen && ((bm[i >> 5] >> (i & 31)) & 1u)) v = v > 0.f ? v / rep : v * rep;
    return v;
  };
  // ---- pass 1, 2: max, e_i, Z
  float mx = -INFINITY;
  for (int i = tid; i < N; i += NT) mx = fmaxf(mx, l1(i));
  const float m = block_max_256(mx, redf);
  float z = 0.f;
  for (int i = tid; i < N; i += NT) {
    const float e = __expf((l1(i) - m) / temperature);
    if (use_lds) erow[i] = e;
    z += e;
  }
  const float Z = block_sum_256(z, redf);                          // (its barriers also publish erow)
  auto pe = [&](int i) -> float { return use_lds ? erow[i] : __expf((l1(i) - m) / temperature); };
  // ---- top-k: the smallest t with C(t) <= k - 1 is the value at rank k
  float Zk = Z;
  unsigned tkb = 0u;
  int tie_k = 0;
  const bool cut_k = top_k >= 1 && top_k < N;
  if (cut_k) {
    unsigned lo = 0u, hi = 0x3f800000u;                            // C(bits(1.0f)) = 0
    while (lo < hi) {
      const unsigned mid = lo + ((hi - lo) >> 1);
      int c = 0;
      for (int i = tid; i < N; i += NT) c += __float_as_uint(pe(i)) > mid ? 1 : 0;
      c = block_sum_int(c, redi);
      if (c < top_k) hi = mid; else lo = mid + 1u;
    }
    tkb = lo;
    float g = 0.f;
    int c = 0;
    for (int i = tid; i < N; i += NT) {
      const float e = pe(i);
      const bool over = __float_as_uint(e) > tkb;
      g += over ? e : 0.f;
      c += over ? 1 : 0;
    }
    g = block_sum_256(g, redf);
    tie_k = top_k - block_sum_int(c, redi);                        // >= 1, and the tie group at tkb has at least as many
    Zk = g + (float)tie_k * __uint_as_float(tkb);
  }
  // ---- the cut: the smallest t with G(t) <= top_p * Z (Z_k under top-k)
  const float X = top_p * Zk;
  unsigned lo = 0u, hi = 0x3f800000u;                              // G(bits(1.0f)) = 0: no e_i exceeds exp(0)
  if (cut_k && top_p >= 1.f) lo = hi = tkb;                        // every rank < k has at most Z_k in front: the top-k cut
  while (lo < hi) {
    const unsigned mid = lo + ((hi - lo) >> 1);
    float g = 0.f;
    for (int i = tid; i < N; i += NT) {
      const float e = pe(i);
      g += __float_as_uint(e) > mid ? e : 0.f;
    }
    g = block_sum_256(g, redf);
    if (g <= X) hi = mid; else lo = mid + 1u;
  }
  unsigned tb = lo;
  const float tf = __uint_as_float(tb);
  float g = 0.f;
  int n_gt = 0, n_eq = 0;
  for (int i = tid; i < N; i += NT) {
    const float e = pe(i);
    const unsigned eb = __float_as_uint(e);
    g += eb > tb ? e : 0.f;
    n_gt += eb > tb ? 1 : 0;
    n_eq += eb == tb ? 1 : 0;
  }
  g = block_sum_256(g, redf);
  n_gt = block_sum_int(n_gt, redi);
  n_eq = block_sum_int(n_eq, redi);
  int n_tie = n_eq;                                                // of the tie group, the j-th has g + j * t in front
  if (tf > 0.f) {
    const float q = (X - g) / tf;
    if (q < (float)n_eq) n_tie = (int)q + 1;
  }
  kept = n_gt + n_tie;
  if (cut_k && (kept > top_k || top_p >= 1.f)) {                   // the shorter prefix of the one order
    tb = tkb;
    n_tie = tie_k;
    kept = top_k;
  }
  // ---- the walk, in index order over contiguous ranges
  const int chunk = (N + NT - 1) / NT;
  const int i0 = min(N, tid * chunk), i1 = min(N, i0 + chunk);
  int c_eq = 0;
  for (int i = i0; i < i1; ++i) c_eq += __float_as_uint(pe(i)) == tb ? 1 : 0;
  const int rank0 = block_scan_i(c_eq, s.wtoti);
  float mass = 0.f;
  int rank = rank0, last = -1;
  for (int i = i0; i < i1; ++i) {
    const float e = pe(i);
    const unsigned eb = __float_as_uint(e);
    const bool k = eb > tb || (eb == tb && rank++ < n_tie);
    if (k) { mass += e; last = i; }
  }
  float M;
  const float before = block_scan_f(mass, s.wtotf, &M);
  const float target = u * M;
  float run = before;
  int cand = 0x7fffffff;
  rank = rank0;
  for (int i = i0; i < i1; ++i) {
    const float e = pe(i);
    const unsigned eb = __float_as_uint(e);
    const bool k = eb > tb || (eb == tb && rank++ < n_tie);
    if (k) {
      run += e;
      if (run > target && cand == 0x7fffffff) cand = i;
    }
  }
  cand = block_min_int(cand, redi);
  last = block_max_int(last, redi);
  return cand < N ? cand : (last >= 0 ? last : 0);                 // (u * M rounded up to M: the last KEPT token)
}

// ---- host side
// the dynamic LDS of a sampled step (row_in_lds: does the row of e_i live there) -> bytes, or 0 and *ok = 0 when the bitmap
// of a penalty does not fit (fvqa_decode_next_ex's vocabulary limit)
inline size_t fvqa_sample_lds(int V, float rep, int* row_in_lds, int* ok) {
  const size_t row_bytes = (size_t)V * sizeof(float);
  const int in_lds = row_bytes <= SAMPLE_ROW_LDS_MAX;
  size_t lds = in_lds ? row_bytes : 0;
  *ok = 1;
  if (rep != 1.f) {                                                // the bitmap: V bits behind the row (on a 16-byte boundary)
    const size_t bitmap = (((size_t)V + 31) / 32) * 4;
    lds = in_lds ? (((size_t)V + 3) & ~(size_t)3) * sizeof(float) + bitmap : bitmap;
    if (lds > SAMPLE_ROW_LDS_MAX + SAMPLE_BITMAP_LDS_MAX) *ok = 0;
  }
  *row_in_lds = in_lds;
  return lds;
}
// the operands and parameters the sampled entries add: FVQA_OK, or the error fvqa_decode_next_ex gives
inline int fvqa_sample_args_ok(const float* u, float temperature, float top_p, int top_k, float rep, const int32_t* gen_start,
                               const int32_t* n_kept) {
  if (!u || !gen_start || !n_kept) return FVQA_EINVAL;
  if (!(temperature > 0.f)) return FVQA_EINVAL;                    // (a NaN fails the comparison)
  if (!(top_p > 0.f && top_p <= 1.f)) return FVQA_EINVAL;
  if (!(rep >= 1.f) || top_k < 0) return FVQA_EINVAL;
  return FVQA_OK;
}

}  // namespace
