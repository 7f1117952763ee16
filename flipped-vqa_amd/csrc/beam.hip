// Beam search on the device (fvqa/generate.py: generate(num_beams > 1)): the two pieces that sit between the LM head and the
// next token's first RMSNorm.
//
// fvqa_beam_step — one launch per token, one 256-thread workgroup per SAMPLE (its K slots, K <= 8):
//   lse      per live slot j: m = max logit, lse = m + logf(sum expf(l - m)), fp32; every sum runs a thread's strided elements in
//            order, then a shuffle tree, then the four waves in order.
//   rank     the candidates of the sample are numbered c = j * V + v — the order (parent ascending, token ascending) —; a live
//            slot offers value(c) = score[j] + (l[j, v] - lse[j]) for every v, a finished slot (or one with no room) offers the
//            one candidate c = j * V with value score[j]. "Better" is (value descending, c ascending). Each thread keeps the
//            eight best of its strided slice in registers (sorted insertion, statically indexed); K rounds of a block-wide
//            arg-best over the threads' heads then pop the K winners in order. No sort, no float atomics: the same bits on
//            every launch.
//   re-seat  slot i takes winner i: its parent's id row (read from ids_in, written to ids_out — the two must not alias, the
//            host ping-pongs them), the token at pos + 1, pos, score, done, n_generated; x_next = emb[token] (a carried slot:
//            the embedding of its current token, so that the layer pass stays well-defined).
//   count    one integer per launch crosses workgroups, through a CALLER-owned word that the caller zeroes once: each workgroup
//            adds (1 | counts << 16) with an integer atomic, the last to arrive writes the count and puts the word back to zero
//            (csrc/token_step.h).
//
// fvqa_beam_step_trie — the same template with TRIE = true (false in fvqa_beam_step, in which none of this exists): constrained
// decoding over a trie in CSR form (fvqa/constrain.py). Every slot sits at a node; a live slot at a node >= 0 offers (j, v) only
// for the tokens v on the node's edges — the candidate loop runs over the edge list, the numbering c = j * V + v and so the
// order are unchanged, lse stays that of the whole raw row —, a live slot without a usable edge (or at a node outside the trie)
// is finished first, a slot at node -1 offers every v. After the K winners are known the edge (j, v) of each child is looked up
// again in its parent's list (a block-wide search, K of them) and the slot takes that edge's child; a carried slot keeps its
// parent's node. All K old nodes are read into LDS before any is written. Every index read from the trie is clamped
// (csrc/token_step.h): the edge range into [0, n_edges], tokens outside [0, V) are skipped, a child outside [0, n_nodes) becomes
// n_nodes (which finishes the slot at its next step).
//
// fvqa_kv_beam_move — cached keys and values follow the beams: for destination sequence n the k and v thirds of cache rows
// [lo[n], hi[n]) of every layer come from sequence src[n]. Direct (scratch == NULL, dst != src: the fan-out of a B-sequence
// prefill into a B*K-sequence cache, adapter rows included) in one launch; through a scratch window (the per-token move inside
// one cache, where the parents of a sample may form cycles) in two: gather every moved row, then scatter. A slot that is its own
// parent launches blocks that return at once. The q third and every row outside the ranges are never written.
#include "token_step.h"

namespace {

constexpr int KMAX = 8;
constexpr int NONE = 0x7fffffff;

__device__ __forceinline__ bool better(float v1, int i1, float v2, int i2) { return v1 > v2 || (v1 == v2 && i1 < i2); }

template <typename T, bool TRIE>
__global__ __launch_bounds__(NT) void beam_step_k(const float* __restrict__ logits, const T* __restrict__ emb, int eos_id,
                                                  int stop_at_eos, int count_any_live, const int64_t* __restrict__ ids_in,
                                                  int64_t* __restrict__ ids_out, int32_t* __restrict__ pos,
                                                  float* __restrict__ score, int32_t* __restrict__ done,
                                                  int32_t* __restrict__ n_generated, int64_t* __restrict__ pos64,
                                                  int32_t* __restrict__ parent_out, int32_t* __restrict__ token_out,
                                                  T* __restrict__ x_next, int32_t* __restrict__ n_active,
                                                  unsigned* __restrict__ counter, int B, int K, int V, int D, int S, int vec16,
                                                  TrieArgs ta) {
  const Trie& tr = ta.trie;
  __shared__ float s_score[KMAX], s_lse[KMAX], redf[4];
  __shared__ int s_done[KMAX], s_pos[KMAX], s_ngen[KMAX];
  __shared__ float w_val[2][4], win_val[KMAX];
  __shared__ int w_idx[2][4], win_idx[KMAX];
  __shared__ int s_node[KMAX], s_e0[KMAX], s_ne[KMAX], s_find[4];   // (TRIE)
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const size_t r0 = (size_t)b * K;                                // the sample's first slot

  if (tid < K) {
    const int p = pos[r0 + tid];
    s_pos[tid] = p;
    s_score[tid] = score[r0 + tid];
    s_ngen[tid] = n_generated[r0 + tid];
    s_done[tid] = (done[r0 + tid] != 0 || p < -1 || p + 1 >= S) ? 1 : 0;      // no room: the slot is finished first
  }
  __syncthreads();

  // ---- TRIE: every slot's node and (clamped) edge range; a live slot at a node without a usable edge is finished first
  if constexpr (TRIE) {
    if (tid < K) {
      const int nd = ta.node[r0 + tid];
      int e0 = 0, e1 = 0;
      if (nd >= 0 && nd < tr.n_nodes) tr.edges(nd, e0, e1);
      s_node[tid] = nd;
      s_e0[tid] = e0;
      s_ne[tid] = e1 - e0;
    }
    __syncthreads();
    for (int j = 0; j < K; ++j) {
      if (s_done[j] || s_node[j] == -1) continue;                  // (uniform over the workgroup)
      const int32_t* et = tr.edge_token + s_e0[j];
      int any = 0;
      for (int i = tid; i < s_ne[j]; i += NT) any |= (unsigned)et[i] < (unsigned)V ? 1 : 0;
      any = __syncthreads_or(any);
      if (!any && tid == 0) s_done[j] = 1;
    }
    __syncthreads();
  }

  // ---- lse of the live slots
  for (int j = 0; j < K; ++j) {
    if (s_done[j]) continue;                                       // (uniform over the workgroup)
    const float* lg = logits + (r0 + j) * V;                       // row_lse of csrc/token_step.h, thread 0 alone taking the
    float mx = -INFINITY;                                          // logarithm (as a call this launch measured slower)
    for (int i = tid; i < V; i += NT) mx = fmaxf(mx, lg[i]);
    const float m = block_max_256(mx, redf);
    float z = 0.f;
    for (int i = tid; i < V; i += NT) z += expf(lg[i] - m);
    const float Z = block_sum_256(z, redf);
    if (tid == 0) s_lse[j] = m + logf(Z);
  }
  __syncthreads();

  // ---- the eight best candidates of this thread's slice, best first
  float tv[KMAX];
  int ti[KMAX];
#pragma unroll
  for (int i = 0; i < KMAX; ++i) { tv[i] = -INFINITY; ti[i] = NONE; }
  auto consider = [&](float val, int idx) {
    if (!better(val, idx, tv[KMAX - 1], ti[KMAX - 1])) return;     // (a NaN is never better)
    tv[KMAX - 1] = val; ti[KMAX - 1] = idx;
#pragma unroll
    for (int i = KMAX - 1; i > 0; --i) {
      if (better(tv[i], ti[i], tv[i - 1], ti[i - 1])) {
        const float fv = tv[i]; tv[i] = tv[i - 1]; tv[i - 1] = fv;
        const int iv = ti[i]; ti[i] = ti[i - 1]; ti[i - 1] = iv;
      }
    }
  };
  for (int j = 0; j < K; ++j) {
    const float sj = s_score[j];
    if (s_done[j]) {
      if (tid == 0) consider(sj, j * V);
      continue;
    }
    const float* lg = logits + (r0 + j) * V;
    const float lse = s_lse[j];
    if constexpr (TRIE) {
      if (s_node[j] != -1) {                                       // the node's edges, in list order = token order
        const int32_t* et = tr.edge_token + s_e0[j];
        for (int i = tid; i < s_ne[j]; i += NT) {
          const int v = et[i];
          if ((unsigned)v < (unsigned)V) consider(sj + (lg[v] - lse), j * V + v);
        }
        continue;
      }
    }
    for (int v = tid; v < V; v += NT) consider(sj + (lg[v] - lse), j * V + v);
  }

  // ---- K rounds: the best head of the workgroup wins and is popped by its owner
  for (int r = 0; r < K; ++r) {
    float bv = tv[0];
    int bi = ti[0];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bv, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
    }
    const int buf = r & 1;                                         // (two buffers: one barrier per round)
    if (lane == 0) { w_val[buf][w] = bv; w_idx[buf][w] = bi; }
    __syncthreads();
    bv = w_val[buf][0]; bi = w_idx[buf][0];
#pragma unroll
    for (int k = 1; k < 4; ++k)
      if (better(w_val[buf][k], w_idx[buf][k], bv, bi)) { bv = w_val[buf][k]; bi = w_idx[buf][k]; }
    if (tid == 0) { win_val[r] = bv; win_idx[r] = bi; }
    if (bi != NONE && ti[0] == bi) {
#pragma unroll
      for (int i = 0; i + 1 < KMAX; ++i) { tv[i] = tv[i + 1]; ti[i] = ti[i + 1]; }
      tv[KMAX - 1] = -INFINITY; ti[KMAX - 1] = NONE;
    }
  }
  __syncthreads();

  // ---- TRIE: the node of every new slot (its parent's, or the child of the edge it took), from the OLD nodes in LDS
  if constexpr (TRIE) {
    for (int i = 0; i < K; ++i) {
      const int c = win_idx[i];
      const bool none = c == NONE;
      const int j = none ? i : c / V;
      const int v = none ? 0 : c - j * V;
      int nd = s_node[j];
      if (!none && s_done[j] == 0 && nd != -1) {                   // (uniform) a child: find the edge (j, v) again
        const int32_t* et = tr.edge_token + s_e0[j];
        int at = NONE;
        for (int e = tid; e < s_ne[j]; e += NT)
          if (et[e] == v) at = min(at, e);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) at = min(at, __shfl_xor(at, o, 64));
        if (lane == 0) s_find[w] = at;
        __syncthreads();
        at = min(min(s_find[0], s_find[1]), min(s_find[2], s_find[3]));
        nd = at != NONE ? tr.child(tr.edge_child[s_e0[j] + at]) : tr.n_nodes;
        __syncthreads();                                           // (s_find is read before the next round writes it)
      }
      if (tid == 0) ta.node[r0 + i] = nd;                          // (the old nodes are all in s_node)
    }
  }

  // ---- re-seat the slots
  for (int i = 0; i < K; ++i) {
    const int c = win_idx[i];
    const bool none = c == NONE;                                   // (fewer than K comparable candidates: rows of NaN)
    const int j = none ? i : c / V;
    const int v = none ? 0 : c - j * V;
    const bool carried = none || s_done[j] != 0;
    const int pj = s_pos[j];
    const int64_t* src_row = ids_in + (r0 + j) * S;
    int64_t* dst_row = ids_out + (r0 + i) * S;
    for (int s = tid; s < S; s += NT) dst_row[s] = (!carried && s == pj + 1) ? (int64_t)v : src_row[s];
    int src_tok = v;
    if (carried) src_tok = valid_token(src_row[valid_pos(pj, S)], V);
    if (tid == 0) {
      const size_t n = r0 + i;
      const int np = carried ? pj : pj + 1;
      pos[n] = np;
      pos64[n] = valid_pos(np, S);
      score[n] = none ? s_score[j] : win_val[i];
      done[n] = (carried || (stop_at_eos && v == eos_id)) ? 1 : 0;
      n_generated[n] = s_ngen[j] + (carried ? 0 : 1);
      parent_out[n] = j;
      token_out[n] = carried ? -1 : v;
    }
    copy_row(x_next + (r0 + i) * D, emb + (size_t)src_tok * D, D, vec16, tid);
  }

  // ---- the count: samples whose slot 0 is not finished, or samples with any unfinished slot
  if (tid == 0) {
    int running = 0;
    for (int i = 0; i < (count_any_live ? K : 1); ++i) {
      const int c = win_idx[i];
      const bool none = c == NONE;
      const int j = none ? i : c / V;
      const int v = none ? 0 : c - j * V;
      const bool fin = none || s_done[j] != 0 || (stop_at_eos && v == eos_id);
      running |= fin ? 0 : 1;
    }
    ticket_arrive(counter, n_active, B, running);
  }
}

// mode 0: dst <- src directly (+ adapter rows); 1: scratch <- src; 2: dst <- scratch. One workgroup per (row, sequence, layer).
template <int MODE>
__global__ __launch_bounds__(NT) void kv_move_k(uint4* __restrict__ dst, const uint4* __restrict__ src, uint4* __restrict__ scratch,
                                                const int32_t* __restrict__ src_seq, const int32_t* __restrict__ lo_p,
                                                const int32_t* __restrict__ hi_p, int n_dst, int n_src, int group, int S, int A,
                                                int rows, int d16) {        // d16: 16-byte words of ONE third of a row
  const int r = blockIdx.x, n = blockIdx.y, l = blockIdx.z, tid = threadIdx.x;
  const size_t dst_layer = ((size_t)n_dst * S + A) * 3 * d16, src_layer = ((size_t)n_src * S + A) * 3 * d16;
  if (MODE == 0 && r >= rows) {                                    // adapter row r - rows, once per layer
    if (n != 0) return;
    const int a = r - rows;
    const uint4* s = src + (size_t)l * src_layer + ((size_t)n_src * S + a) * 3 * d16 + d16;
    uint4* d = dst + (size_t)l * dst_layer + ((size_t)n_dst * S + a) * 3 * d16 + d16;
    for (int k = tid; k < 2 * d16; k += NT) d[k] = s[k];
    return;
  }
  int sq = src_seq[n];
  if (group > 0) sq += (n / group) * group;
  if (MODE != 0 && sq == n) return;                                // its own parent: nothing moves
  if (sq < 0 || sq >= n_src) return;
  int lo = lo_p[n], hi = hi_p[n];
  lo = lo < 0 ? 0 : lo;
  hi = hi > S ? S : hi;
  if (MODE != 0 && hi > lo + rows) hi = lo + rows;                 // (the window's contract: hi - lo <= rows)
  const int row = MODE == 0 ? r : lo + r;
  if (row < lo || row >= hi) return;
  const size_t win = (((size_t)l * n_dst + n) * rows + r) * 2 * d16;
  const uint4* s = MODE == 2 ? scratch + win : src + (size_t)l * src_layer + ((size_t)sq * S + row) * 3 * d16 + d16;
  uint4* d = MODE == 1 ? scratch + win : dst + (size_t)l * dst_layer + ((size_t)n * S + row) * 3 * d16 + d16;
  for (int k = tid; k < 2 * d16; k += NT) d[k] = s[k];
}

}  // namespace

namespace {

template <bool TRIE>
int beam_step_checked(const float* logits, const void* emb, int eos_id, int stop_at_eos, int count_any_live,
                      const int64_t* ids_in, int64_t* ids_out, int32_t* pos, float* score, int32_t* done, int32_t* n_generated,
                      int64_t* pos64, int32_t* parent, int32_t* token, void* x_next, int32_t* n_active, uint32_t* counter,
                      int n_samples, int n_beams, int vocab, int dim, int seq_len, int dtype, void* stream, TrieArgs tr) {
  if (!logits || !emb || !ids_in || !ids_out || !pos || !score || !done || !n_generated || !pos64 || !parent || !token ||
      !x_next || !n_active || !counter)
    return FVQA_EINVAL;
  if (TRIE && fvqa_trie_given(tr.node, tr.trie.node_first, tr.trie.edge_token, tr.trie.edge_child) != 1) return FVQA_EINVAL;
  if (ids_in == ids_out) return FVQA_EINVAL;
  if (!fvqa_dtype_ok(dtype)) return FVQA_EINVAL;
  if (n_samples <= 0 || vocab <= 0 || dim <= 0 || seq_len <= 0) return FVQA_ESHAPE;
  if (n_beams < 1 || n_beams > KMAX || n_beams > vocab) return FVQA_ESHAPE;
  if (n_samples > 65535 || (long long)n_beams * vocab > 0x7ffffffeLL) return FVQA_ESHAPE;   // 16-bit arrivals; c fits an int
  if (TRIE && (tr.trie.n_nodes <= 0 || tr.trie.n_edges < 0)) return FVQA_ESHAPE;
  if (!fvqa_aligned(fvqa_dtype_size(dtype), emb, x_next) ||
      !fvqa_aligned(4, logits, pos, score, done, n_generated, parent, token, n_active, counter) ||
      !fvqa_aligned(8, ids_in, ids_out, pos64) || !fvqa_aligned(4, tr.node, tr.trie.node_first, tr.trie.edge_token, tr.trie.edge_child))
    return FVQA_EALIGN;
  hipStream_t st = (hipStream_t)stream;
  const int vec16 = fvqa_vec16((size_t)dim * fvqa_dtype_size(dtype), emb, x_next);
  if (dtype == FVQA_H16)
    hipLaunchKernelGGL((beam_step_k<bf16_t, TRIE>), dim3(n_samples), dim3(NT), 0, st, logits, (const bf16_t*)emb, eos_id,
                       stop_at_eos, count_any_live, ids_in, ids_out, pos, score, done, n_generated, pos64, parent, token,
                       (bf16_t*)x_next, n_active, counter, n_samples, n_beams, vocab, dim, seq_len, vec16, tr);
  else
    hipLaunchKernelGGL((beam_step_k<float, TRIE>), dim3(n_samples), dim3(NT), 0, st, logits, (const float*)emb, eos_id,
                       stop_at_eos, count_any_live, ids_in, ids_out, pos, score, done, n_generated, pos64, parent, token,
                       (float*)x_next, n_active, counter, n_samples, n_beams, vocab, dim, seq_len, vec16, tr);
  FVQA_CHECK_LAUNCH();
  return FVQA_OK;
}

}  // namespace

extern "C" int fvqa_beam_step(const float* logits, const void* emb, int eos_id, int stop_at_eos, int count_any_live,
                              const int64_t* ids_in, int64_t* ids_out, int32_t* pos, float* score, int32_t* done,
                              int32_t* n_generated, int64_t* pos64, int32_t* parent, int32_t* token, void* x_next,
                              int32_t* n_active, uint32_t* counter, int n_samples, int n_beams, int vocab, int dim, int seq_len,
                              int dtype, void* stream) {
  return beam_step_checked<false>(logits, emb, eos_id, stop_at_eos, count_any_live, ids_in, ids_out, pos, score, done,
                                  n_generated, pos64, parent, token, x_next, n_active, counter, n_samples, n_beams, vocab, dim,
                                  seq_len, dtype, stream, TrieArgs{});
}

extern "C" int fvqa_beam_step_trie(const float* logits, const void* emb, int eos_id, int stop_at_eos, int count_any_live,
                                   const int64_t* ids_in, int64_t* ids_out, int32_t* pos, float* score, int32_t* done,
                                   int32_t* n_generated, int64_t* pos64, int32_t* parent, int32_t* token, void* x_next,
                                   int32_t* n_active, uint32_t* counter, int32_t* node, const int32_t* node_first,
                                   const int32_t* edge_token, const int32_t* edge_child, int n_nodes, int n_edges,
                                   int n_samples, int n_beams, int vocab, int dim, int seq_len, int dtype, void* stream) {
  return beam_step_checked<true>(logits, emb, eos_id, stop_at_eos, count_any_live, ids_in, ids_out, pos, score, done,
                                 n_generated, pos64, parent, token, x_next, n_active, counter, n_samples, n_beams, vocab, dim,
                                 seq_len, dtype, stream, TrieArgs{node, {node_first, edge_token, edge_child, n_nodes, n_edges}});
}

extern "C" size_t fvqa_kv_beam_move_scratch(int n_seq, int window_rows, int dim, int n_layers, int dtype) {
  if (n_seq <= 0 || window_rows <= 0 || dim <= 0 || n_layers <= 0) return 0;
  return (size_t)n_layers * n_seq * window_rows * 2 * dim * fvqa_dtype_size(dtype);
}

extern "C" int fvqa_kv_beam_move(void* dst, const void* src, void* scratch, size_t scratch_bytes, const int32_t* src_seq,
                                 const int32_t* lo, const int32_t* hi, int n_dst_seq, int n_src_seq, int group, int seq_len,
                                 int dim, int n_layers, int adapter_len, int window_rows, int dtype, void* stream) {
  if (!dst || !src || !src_seq || !lo || !hi) return FVQA_EINVAL;
  if (!fvqa_dtype_ok(dtype)) return FVQA_EINVAL;
  if (!scratch && dst == src) return FVQA_EINVAL;                  // inside one cache the move goes through the window
  if (n_dst_seq <= 0 || n_src_seq <= 0 || seq_len <= 0 || dim <= 0 || n_layers <= 0 || adapter_len < 0 || group < 0)
    return FVQA_ESHAPE;
  if (n_dst_seq > 65535 || n_layers > 65535 || ((size_t)dim * fvqa_dtype_size(dtype)) % 16 != 0) return FVQA_ESHAPE;
  if (scratch && (window_rows <= 0 || n_dst_seq != n_src_seq)) return FVQA_ESHAPE;
  if (!fvqa_aligned(16, dst, src, scratch) || !fvqa_aligned(4, src_seq, lo, hi)) return FVQA_EALIGN;
  if (scratch && scratch_bytes < fvqa_kv_beam_move_scratch(n_dst_seq, window_rows, dim, n_layers, dtype)) return FVQA_EALIGN;
  hipStream_t st = (hipStream_t)stream;
  const int d16 = (int)((size_t)dim * fvqa_dtype_size(dtype) / 16);
  if (!scratch) {
    hipLaunchKernelGGL(kv_move_k<0>, dim3(seq_len + adapter_len, n_dst_seq, n_layers), dim3(NT), 0, st, (uint4*)dst,
                       (const uint4*)src, (uint4*)nullptr, src_seq, lo, hi, n_dst_seq, n_src_seq, group, seq_len, adapter_len,
                       seq_len, d16);
    FVQA_CHECK_LAUNCH();
    return FVQA_OK;
  }
  const int rows = window_rows < seq_len ? window_rows : seq_len;
  const dim3 grid(rows, n_dst_seq, n_layers);
  hipLaunchKernelGGL(kv_move_k<1>, grid, dim3(NT), 0, st, (uint4*)dst, (const uint4*)src, (uint4*)scratch, src_seq, lo, hi,
                     n_dst_seq, n_src_seq, group, seq_len, adapter_len, window_rows, d16);
  FVQA_CHECK_LAUNCH();
  hipLaunchKernelGGL(kv_move_k<2>, grid, dim3(NT), 0, st, (uint4*)dst, (const uint4*)src, (uint4*)scratch, src_seq, lo, hi,
                     n_dst_seq, n_src_seq, group, seq_len, adapter_len, window_rows, d16);
  FVQA_CHECK_LAUNCH();
  return FVQA_OK;
}
