// What the token-step kernels share (csrc/sample.hip, beam.hip, spec.hip, treespec.hip, jump.hip: one 256-thread workgroup per
// sequence or sample, everything between the LM head and the next pass's first RMSNorm in one launch), each rule written once: the
// integer block reductions, the block scans and the lse of a raw row, the verify scan of the draft-and-verify steps, the view of a trie with its
// two clamps, the clamps that keep a finished row's reads inside its arrays, the ticket word that counts running rows across
// workgroups, the embedding rows of the next pass, and the host side's operand rules (16-byte rows, storage-type dispatch, "no
// trie or a whole one"). The pick of a row — the elements that take part, greedy, sampled, the penalty's bitmap, the dynamic LDS
// — is csrc/row_sample.h, on top of this header; row_verify below stays beside it because its arg-max shares a pass with the lse.
#pragma once
#include <type_traits>
#include "common.h"

namespace {

constexpr int NT = 256;

__device__ __forceinline__ int block_sum_int(int v, int* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  const int w = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[w] = v;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}
__device__ __forceinline__ int block_min_int(int v, int* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
  const int w = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[w] = v;
  __syncthreads();
  return min(min(red[0], red[1]), min(red[2], red[3]));
}
__device__ __forceinline__ int block_max_int(int v, int* red) { return -block_min_int(-v, red); }

// exclusive prefix of v over the 256 threads in thread order (fixed tree); *total = the sum over all of them
__device__ __forceinline__ float block_scan_f(float v, float* wtot, float* total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  float x = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const float y = __shfl_up(x, o, 64);
    if (lane >= o) x += y;
  }
  __syncthreads();
  if (lane == 63) wtot[w] = x;
  __syncthreads();
  float base = 0.f;
  for (int k = 0; k < w; ++k) base += wtot[k];
  *total = ((wtot[0] + wtot[1]) + wtot[2]) + wtot[3];
  return base + (x - v);
}
__device__ __forceinline__ int block_scan_i(int v, int* wtot) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int x = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int y = __shfl_up(x, o, 64);
    if (lane >= o) x += y;
  }
  __syncthreads();
  if (lane == 63) wtot[w] = x;
  __syncthreads();
  int base = 0;
  for (int k = 0; k < w; ++k) base += wtot[k];
  return base + x - v;
}

// m + log(sum exp(l - m)) of one raw row: the maximum, then the sum of expf over a thread's strided elements in order, a shuffle
// tree, the four waves in order. Every log-probability of the token steps is taken against this value (row_verify below fuses
// the same operations into its arg-max pass).
__device__ __forceinline__ float row_lse(const float* __restrict__ lg, int V, float* red) {
  float mx = -INFINITY;
  for (int i = threadIdx.x; i < V; i += NT) mx = fmaxf(mx, lg[i]);
  const float m = block_max_256(mx, red);
  float z = 0.f;
  for (int i = threadIdx.x; i < V; i += NT) z += expf(lg[i] - m);
  return m + logf(block_sum_256(z, red));
}

// The verify scan of one raw row by the whole workgroup (csrc/spec.hip, csrc/treespec.hip): the largest logit, the lowest index on
// exact ties (fvqa_decode_next's loop; 0 for a row of NaNs), and into `lse` row_lse's second half on the arg-max's maximum — a
// call of row_lse would add a pass over the row; the operations and the bits are the same.
__device__ __forceinline__ int row_verify(const float* lg, int V, float* redf, int* redi, float& lse) {
  float bv = -INFINITY;
  int bi = 0x7fffffff;
  for (int v = threadIdx.x; v < V; v += NT) {
    const float x = lg[v];
    if (x > bv || (x == bv && v < bi)) { bv = x; bi = v; }
  }
  const float mx = block_max_256(bv, redf);
  int g = block_min_int(bv == mx ? bi : 0x7fffffff, redi);
  if (g >= V) g = 0;                                               // (a row of NaNs)
  float z = 0.f;
  for (int v = threadIdx.x; v < V; v += NT) z += expf(lg[v] - mx);
  lse = mx + logf(block_sum_256(z, redf));
  return g;
}

// What the draft-and-verify steps say of a sequence before they scan: a finished row, one with no room for another token and
// one whose budget is spent commit nothing; a pass fed between 1 and `rows` rows, whatever len says.
__device__ __forceinline__ bool verify_live(int done, int p0, int S, int ngen, int max_new) {
  return done == 0 && p0 >= -1 && p0 + 1 < S && ngen < max_new;
}
__device__ __forceinline__ int verify_rows(int len, int rows) { return len < 1 ? 1 : (len > rows ? rows : len); }
// ... and behind the nc tokens a step committed, in its `width` result slots from `at`: token -1, log-probability 0 (one thread
// per workgroup calls this)
__device__ __forceinline__ void verify_pad(int32_t* token, float* logprob, size_t at, int nc, int width) {
  for (int j = nc; j < width; ++j) {
    token[at + j] = -1;
    logprob[at + j] = 0.f;
  }
}

// A trie of allowed answers in CSR form (fvqa/constrain.py). Every index read from it is clamped before it is used.
struct Trie {
  const int32_t* node_first;
  const int32_t* edge_token;
  const int32_t* edge_child;
  int n_nodes, n_edges;

  // the edges [e0, e1) of node nd (0 <= nd < n_nodes), clamped into [0, n_edges]
  __device__ __forceinline__ void edges(int nd, int& e0, int& e1) const {
    e0 = node_first[nd];
    e1 = node_first[nd + 1];
    e0 = e0 < 0 ? 0 : (e0 > n_edges ? n_edges : e0);
    e1 = e1 < e0 ? e0 : (e1 > n_edges ? n_edges : e1);
  }
  // the child an edge names; one outside [0, n_nodes) becomes n_nodes (a broken trie: the row ends at its next step)
  __device__ __forceinline__ int child(int ch) const { return (ch < 0 || ch >= n_nodes) ? n_nodes : ch; }
};

// the trie operands of an entry whose rows sit at nodes: node (in and out, one per row or slot; -1: unconstrained) and the trie
struct TrieArgs {
  int32_t* node;
  Trie trie;
};

// any valid embedding row for a row that picked nothing (the batch stays rectangular), and the position it is read at
__device__ __forceinline__ int valid_token(int64_t t, int V) { return t < 0 ? 0 : (t >= V ? V - 1 : (int)t); }
__device__ __forceinline__ int valid_pos(int p, int S) { return p < 0 ? 0 : (p >= S ? S - 1 : p); }

// n_active needs a count across workgroups: each adds (1 arrival | its row still running << 16) to one device-resident ticket
// word with an INTEGER atomic; the one of the n_wg workgroups that arrives last writes the count and puts the word back to zero.
// Launches that share a word must be ordered (one stream, or events). One thread per workgroup calls this.
__device__ __forceinline__ void ticket_arrive(unsigned* ticket, int32_t* n_active, int n_wg, bool running) {
  const unsigned old = atomicAdd(ticket, 1u + (running ? 0x10000u : 0u));
  if ((int)(old & 0xffffu) == n_wg - 1) {
    *n_active = (int)(old >> 16) + (running ? 1 : 0);
    atomicExch(ticket, 0u);
  }
}

// one row of D elements, by the whole workgroup (tid: the caller's threadIdx.x): 16-byte words when vec16 (fvqa_vec16), else
// element by element
template <typename T>
__device__ __forceinline__ void copy_row(T* dst, const T* src, int D, int vec16, int tid) {
  if (vec16) {
    const int n16 = (int)((size_t)D * sizeof(T) / 16);
    for (int i = tid; i < n16; i += NT) reinterpret_cast<uint4*>(dst)[i] = reinterpret_cast<const uint4*>(src)[i];
  } else {
    for (int i = tid; i < D; i += NT) dst[i] = src[i];
  }
}
template <typename T>
__device__ __forceinline__ void zero_row(T* dst, int D, int vec16, int tid) {
  if (vec16) {
    const int n16 = (int)((size_t)D * sizeof(T) / 16);
    for (int i = tid; i < n16; i += NT) reinterpret_cast<uint4*>(dst)[i] = make_uint4(0u, 0u, 0u, 0u);
  } else {
    for (int i = tid; i < D; i += NT) dst[i] = from_f32<T>(0.f);
  }
}

// the Tn input rows of sequence b in the next pass: emb[tok(j)] for j < n_emb, zeros behind
template <typename T, typename F>
__device__ __forceinline__ void next_pass_rows(T* x_next, const T* emb, int b, int Tn, int D, int vec16, int tid, int n_emb,
                                               F tok) {
  for (int j = 0; j < Tn; ++j) {
    T* dst = x_next + ((size_t)b * Tn + j) * D;
    if (j < n_emb) copy_row(dst, emb + (size_t)tok(j) * D, D, vec16, tid);
    else zero_row(dst, D, vec16, tid);
  }
}

// ---- host side
// rows of row_bytes bytes are whole 16-byte words on 16-byte boundaries in both buffers
inline int fvqa_vec16(size_t row_bytes, const void* emb, const void* x_next) {
  return row_bytes % 16 == 0 && fvqa_aligned(16, emb, x_next);
}
// f(T*) with T the storage type of a checked dtype code (fvqa_dtype_ok): this build's 16-bit type, or float
template <typename F> inline void fvqa_by_dtype(int dtype, F&& f) {
  if (dtype == FVQA_H16) f((bf16_t*)nullptr);
  else f((float*)nullptr);
}
// the four trie operands of an entry that may run without one: 0 none of them, 1 all of them, -1 a trie given in part
inline int fvqa_trie_given(const void* node, const void* node_first, const void* edge_token, const void* edge_child) {
  if (!node && !node_first && !edge_token && !edge_child) return 0;
  return node && node_first && edge_token && edge_child ? 1 : -1;
}

}  // namespace
