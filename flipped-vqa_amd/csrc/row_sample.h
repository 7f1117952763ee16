// The row pick of the token steps, written once: which elements of a row take part (RowElems: the vocabulary, or the edge list of
// a trie node), the greedy pick (row_pick_greedy) and the sampled pick (row_pick_sampled: rules 1 to 4 of fvqa_decode_next_ex,
// include/fvqa.h — temperature, top-k and the nucleus cut by two bisections over bit patterns, the tie group, the walk in index
// order), each by the whole 256-thread workgroup on ONE row. csrc/sample.hip's decode_next_k calls them in every instantiation,
// csrc/jump.hip the view and the greedy pick, csrc/spec.hip and csrc/treespec.hip (SAMPLE = true) the sampled pick on the
// vocabulary through row_sample. The "ids are the plain sampled call's" contracts of the draft-and-verify steps hold because
// there is one pick; csrc/sample.hip's header comment states the rule itself.
//
// What a pick is given:
//   elements the view: N elements of which those with ok(i) take part, tok(i) the token of element i, n_ok of them (what top-k is
//            cut against), first_ok the first (the fall-back of a row of NaNs). A caller may narrow a view (csrc/sample.hip, PAIR:
//            the plausible set) by handing over anything with these five members.
//   l1(t)    the logit the pick sees at token t: raw, penalised (sample_penalised), or PAIR's c_t. The raw row's lse, which the
//            log-probabilities are taken against, is the caller's (csrc/token_step.h row_lse).
//   u        the draw. Which one is the caller's business: u[b], the stream's u[ti * n_req + r], sample_draw.
//   LDS      one dynamic block: the row of e_i (4 * V bytes, when they fit: row_in_lds), then the bitmap of V bits on a 16-byte
//            boundary (sample_bitmap_at); fvqa_sample_lds sizes it. A pick rewrites the row; the block reductions at its end are
//            the barrier in front of the next pick of a step.
//   bitmap   R, the ids generated so far: built from ids[gen_start .. pos] (sample_bitmap_build); a step that commits several
//            tokens adds one bit after every commit (sample_bitmap_add), so that row i + 1 sees the tokens rows 0 .. i committed.
//            Only under a penalty (rep != 1): without one no bitmap exists and none is read.
//   ban set  X (fvqa_decode_next_rules, rule 0): a second bitmap of V bits behind R's (sample_ban_at), built from the same ids once
//            per step (sample_ban_build). The pick does not know it: the caller's view answers ok(i) = false for a banned token,
//            so it takes part nowhere — exactly as an edge outside [0, V) or a token outside the plausible set takes none.
//   min-p    MINP = true: rule 3' — one counting pass behind the nucleus cut; false (every other caller): none of its code exists.
#pragma once
#include "token_step.h"

namespace {

constexpr size_t ROW_LDS_MAX = 144 * 1024;                // the largest row of e_i kept in LDS: beside ~100 bytes of reduction
                                                          // scratch and the bitmap, under the CU's 160 KiB
constexpr size_t BITMAP_LDS_MAX = ROW_LDS_MAX / 32;       // the bitmap of the largest row that lives in LDS

// the operands the sampled draft-and-verify entries add to the entry each extends
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
// R of a row: the distinct ids at positions max(g0, 0) .. p (p <= S - 2: the row is live)
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
// the ban set's place in the dynamic block: behind the bitmap of R when there is one (pen), else in its place
__device__ __forceinline__ unsigned* sample_ban_at(unsigned* bm, int V, bool pen) { return bm + (pen ? ((V + 31) >> 5) : 0); }
// X of a row (fvqa_decode_next_rules, rule 0), from the generated ids at positions g0c = max(g0, 0) .. p (p <= S - 2: the row is
// live; every index read lies in [g0c, p]): the EOS while the token index p + 1 - g0 is below min_new; with ngram = n >= 1 the
// token behind every earlier occurrence, inside the generated ids, of the last n - 1 of them. Ids outside [0, V) are ignored.
__device__ __forceinline__ void sample_ban_build(unsigned* ban, const int64_t* row_ids, int g0, int p, int V, int ngram,
                                                 int min_new, int eos_id) {
  const int tid = threadIdx.x;
  for (int i = tid; i < ((V + 31) >> 5); i += NT) ban[i] = 0u;
  __syncthreads();
  if (tid == 0 && (long long)p + 1 - (long long)g0 < (long long)min_new && eos_id >= 0 && eos_id < V)
    atomicOr(&ban[eos_id >> 5], 1u << (eos_id & 31));
  const long long g0c = g0 < 0 ? 0 : g0;
  const long long n1 = (long long)ngram - 1;                       // the suffix s = ids[p - n1 + 1 .. p]
  if (ngram >= 1 && (long long)p - n1 + 1 >= g0c) {
    const int64_t* s = row_ids + ((long long)p - n1 + 1);
    for (long long j = g0c + tid; j + n1 <= (long long)p; j += NT) {
      bool eq = true;
      for (long long k = 0; k < n1 && eq; ++k) eq = row_ids[j + k] == s[k];
      const int64_t t = row_ids[j + n1];
      if (eq && t >= 0 && t < V) atomicOr(&ban[t >> 5], 1u << (t & 31));
    }
  }
  __syncthreads();
}
__device__ __forceinline__ bool sample_banned(const unsigned* ban, int t) { return (ban[t >> 5] >> (t & 31)) & 1u; }
// the penalty's read of the logit v of token t: l / r or l * r where the bit is set. The logits are not written.
__device__ __forceinline__ float sample_penalised(float v, int t, const unsigned* bm, float rep) {
  if ((bm[t >> 5] >> (t & 31)) & 1u) v = v > 0.f ? v / rep : v * rep;
  return v;
}

// the draw of token index t of sequence n
__device__ __forceinline__ float sample_draw(const float* u, int t, int max_new, int n_seq, int n) {
  const int tc = t < 0 ? 0 : (t >= max_new ? max_new - 1 : t);
  return u[(size_t)tc * n_seq + n];
}

// The elements a pick runs over: the vocabulary (element i = token i, all of them usable; without TRIE nothing else exists and
// ok / tok fold away) or, for a row at a trie node, the node's edge list — element i is edge i, its token edge_token[i]; a node's
// edges are in ascending token order, so the list order is the index order of the rule. An edge whose token lies outside [0, V)
// is not usable.
template <bool TRIE>
struct RowElems {
  int N, n_ok, first_ok;                 // elements; the usable ones: how many, and the first
  int V;
  bool cons;                             // the row sits at a node
  const int32_t *et, *ec;                // the node's edge tokens and children (cons, N > 0)
  __device__ __forceinline__ bool ok(int i) const {
    if constexpr (TRIE) {
      if (cons) return (unsigned)et[i] < (unsigned)V;
    }
    return true;
  }
  __device__ __forceinline__ int tok(int i) const {                // (ok(i) holds)
    if constexpr (TRIE) {
      if (cons) return et[i];
    }
    return i;
  }
};
// the view of a row at node nd (-1, and every row without TRIE: the vocabulary), every index clamped: a node outside the trie has
// no edges, the edge range lies in [0, n_edges] (Trie::edges). n_ok == 0 — no children — ends the row: the caller's to act on.
// The whole workgroup calls this with one nd.
template <bool TRIE>
__device__ __forceinline__ RowElems<TRIE> row_elems(int V, const Trie& tr, int nd, int* redi) {
  RowElems<TRIE> el{V, V, 0, V, false, nullptr, nullptr};
  if constexpr (TRIE) {
    if (nd != -1) {
      el.cons = true;
      el.N = 0;
      if (nd >= 0 && nd < tr.n_nodes) {
        int e0, e1;
        tr.edges(nd, e0, e1);
        el.et = tr.edge_token + e0;
        el.ec = tr.edge_child + e0;
        el.N = e1 - e0;
      }
      int c = 0, f = 0x7fffffff;
      for (int i = threadIdx.x; i < el.N; i += NT)
        if ((unsigned)el.et[i] < (unsigned)V) { c += 1; f = min(f, i); }
      el.n_ok = block_sum_int(c, redi);
      el.first_ok = block_min_int(f, redi);
    }
  }
  return el;
}

// The greedy pick -> the element: the largest l1, the lowest element on exact ties; first_ok on a row of NaNs.
template <typename E, typename L>
__device__ __forceinline__ int row_pick_greedy(const E& el, L l1, float* redf, int* redi) {
  float bv = -INFINITY;
  int bi = 0x7fffffff;
  for (int i = threadIdx.x; i < el.N; i += NT) {
    if (!el.ok(i)) continue;
    const float v = l1(el.tok(i));
    if (v > bv || (v == bv && i < bi)) { bv = v; bi = i; }
  }
  const float m = block_max_256(bv, redf);
  const int sel = block_min_int(bv == m ? bi : 0x7fffffff, redi);
  return sel < el.N ? sel : el.first_ok;
}

// The sampled pick -> the element; kept = n_kept. TOPK = false: an entry without top-k (fvqa_decode_next), whose instantiation
// holds none of its code. use_lds: the row of e_i lives in s.erow (N <= the floats sized for it), else every pass recomputes it.
// MINP = true (fvqa_decode_next_rules): rule 3' with min_p in [0, 1) — false everywhere else, and none of its code exists.
template <bool TOPK, bool MINP = false, typename E, typename L>
__device__ __forceinline__ int row_pick_sampled(const E& el, L l1, bool use_lds, const SampleLds& s, float u, float temperature,
                                                float top_p, int top_k, int& kept, float min_p = 0.f) {
  const int tid = threadIdx.x;
  const int N = el.N;
  float* erow = s.erow;
  float* redf = s.redf;
  int* redi = s.redi;
  // ---- pass 1, 2: max, e_i, Z
  float mx = -INFINITY;
  for (int i = tid; i < N; i += NT)
    if (el.ok(i)) mx = fmaxf(mx, l1(el.tok(i)));
  const float m = block_max_256(mx, redf);
  float z = 0.f;
  for (int i = tid; i < N; i += NT) {
    const float e = el.ok(i) ? __expf((l1(el.tok(i)) - m) / temperature) : 0.f;
    if (use_lds) erow[i] = e;
    z += e;
  }
  const float Z = block_sum_256(z, redf);                          // (its barriers also publish erow)
  // (an element without ok() has e = 0: no `> t` test below sees it, and every `== t` test asks ok() as well)
  auto pe = [&](int i) -> float {
    return use_lds ? erow[i] : (el.ok(i) ? __expf((l1(el.tok(i)) - m) / temperature) : 0.f);
  };
  // ---- top-k: the smallest t with C(t) <= k - 1 is the value at rank k
  float Zk = Z;
  unsigned tkb = 0u;
  int tie_k = 0;
  const bool cut_k = TOPK && top_k >= 1 && top_k < el.n_ok;
  if constexpr (TOPK) {
    if (cut_k) {
      unsigned lo = 0u, hi = 0x3f800000u;                          // C(bits(1.0f)) = 0
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
      tie_k = top_k - block_sum_int(c, redi);                      // >= 1, and the tie group at tkb has at least as many
      Zk = g + (float)tie_k * __uint_as_float(tkb);
    }
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
    n_eq += (eb == tb && el.ok(i)) ? 1 : 0;
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
  // ---- min-p: the elements with e >= min_p are a prefix of the same order made of whole tie groups (the maximum has e == 1 >
  // min_p: never empty); where it is the shortest of the prefixes it is the kept set — every e at or above bits(min_p)
  if constexpr (MINP) {
    if (min_p > 0.f) {
      const unsigned mpb = __float_as_uint(min_p);                 // (non-negative floats order as their bits do)
      int c = 0;
      for (int i = tid; i < N; i += NT) c += (el.ok(i) && __float_as_uint(pe(i)) >= mpb) ? 1 : 0;
      c = block_sum_int(c, redi);
      if (c < kept) {
        tb = mpb;
        n_tie = 0x7fffffff;
        kept = c;
      }
    }
  }
  // ---- the walk, in index order over contiguous ranges
  const int chunk = (N + NT - 1) / NT;
  const int i0 = min(N, tid * chunk), i1 = min(N, i0 + chunk);
  int c_eq = 0;
  for (int i = i0; i < i1; ++i) c_eq += (__float_as_uint(pe(i)) == tb && el.ok(i)) ? 1 : 0;
  const int rank0 = block_scan_i(c_eq, s.wtoti);
  float mass = 0.f;
  int rank = rank0, last = -1;
  for (int i = i0; i < i1; ++i) {
    const float e = pe(i);
    const unsigned eb = __float_as_uint(e);
    const bool k = eb > tb || (eb == tb && el.ok(i) && rank++ < n_tie);
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
    const bool k = eb > tb || (eb == tb && el.ok(i) && rank++ < n_tie);
    if (k) {
      run += e;
      if (run > target && cand == 0x7fffffff) cand = i;
    }
  }
  cand = block_min_int(cand, redi);
  last = block_max_int(last, redi);
  return cand < N ? cand : (last >= 0 ? last : el.first_ok);       // (u * M rounded up to M: the last KEPT element)
}

// The pick of a draft-and-verify step under sampling: fvqa_decode_next_ex's on the raw row lg (V logits, the vocabulary view)
// with the draw u -> the token; kept = n_kept, lse = the raw row's. pen: the bitmap holds R and rep != 1.
__device__ __forceinline__ int row_sample(const float* lg, int V, float u, const SampleArgs& sa, bool pen, const SampleLds& s,
                                          int& kept, float& lse) {
  lse = row_lse(lg, V, s.redf);
  auto l1 = [&](int t) -> float { return pen ? sample_penalised(lg[t], t, s.bm, sa.rep) : lg[t]; };
  return row_pick_sampled<true>(RowElems<false>{V, V, 0, V, false, nullptr, nullptr}, l1, sa.row_in_lds, s, u, sa.temperature,
                                sa.top_p, sa.top_k, kept);
}

// ---- host side
// the dynamic LDS of a launch that picks (keep_row: may the row of e_i live there — a greedy launch keeps none; ban: a ban set
// follows, fvqa_decode_next_rules) -> bytes, with *row_in_lds; 0 and *ok = 0 when the bitmaps do not fit: one bitmap (a penalty,
// or a ban set without one) beyond 1216512 ids, the two together beyond 626688
inline size_t fvqa_sample_lds(int V, float rep, bool keep_row, int* row_in_lds, int* ok, bool ban = false) {
  const size_t row_bytes = (size_t)V * sizeof(float);
  const int in_lds = keep_row && row_bytes <= ROW_LDS_MAX;
  size_t lds = in_lds ? row_bytes : 0;
  *ok = 1;
  const size_t n_bitmaps = (rep != 1.f ? 1 : 0) + (ban ? 1 : 0);
  if (n_bitmaps) {                                                 // the bitmaps: V bits each behind the row (on a 16-byte boundary)
    const size_t bitmap = (((size_t)V + 31) / 32) * 4 * n_bitmaps;
    lds = in_lds ? (((size_t)V + 3) & ~(size_t)3) * sizeof(float) + bitmap : bitmap;
    if (lds > ROW_LDS_MAX + n_bitmaps * BITMAP_LDS_MAX) *ok = 0;
  }
  *row_in_lds = in_lds;
  return lds;
}
// the dynamic-LDS limit of kernel K, once per device: the largest row, and the largest bitmaps behind it (0, 1 or 2 of them)
template <auto K>
inline void fvqa_sample_lds_limit(int n_bitmaps) {
  static std::atomic<unsigned long long> attr_done{0};             // one bit per device (fvqa_attr_needed)
  if (fvqa_attr_needed(attr_done))
    (void)hipFuncSetAttribute((const void*)K, hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)(ROW_LDS_MAX + (size_t)n_bitmaps * BITMAP_LDS_MAX));
}
// The operands and parameters a sampled draft-and-verify entry adds, in the two places of its checks (the order of an entry's
// outcomes is part of the ABI): among the FVQA_EINVAL checks ...
inline int fvqa_sample_args_ok(const SampleArgs* sa) {
  if (!sa) return FVQA_OK;
  if (!sa->u || !sa->gen_start || !sa->n_kept) return FVQA_EINVAL;
  if (!(sa->temperature > 0.f)) return FVQA_EINVAL;                // (a NaN fails the comparison)
  if (!(sa->top_p > 0.f && sa->top_p <= 1.f)) return FVQA_EINVAL;
  if (!(sa->rep >= 1.f) || sa->top_k < 0) return FVQA_EINVAL;
  return FVQA_OK;
}
// ... and behind the entry's own shape and alignment checks: their alignment, then the launch's dynamic LDS -> *s (the operands
// with row_in_lds set; all zero without sa) and *lds
inline int fvqa_sample_launch_args(const SampleArgs* sa, int vocab, SampleArgs* s, size_t* lds) {
  *s = SampleArgs{};
  *lds = 0;
  if (!sa) return FVQA_OK;
  if (!fvqa_aligned(4, sa->u, sa->gen_start, sa->n_kept)) return FVQA_EALIGN;
  *s = *sa;
  int fits;
  *lds = fvqa_sample_lds(vocab, sa->rep, true, &s->row_in_lds, &fits);
  return fits ? FVQA_OK : FVQA_ESHAPE;                             // (a vocabulary beyond 1.2 million ids under a penalty)
}

}  // namespace
