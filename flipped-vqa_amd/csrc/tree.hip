// Exact answer-vocabulary scoring (fvqa/vocab.py score_vocab): every allowed answer of a sample is a root-to-leaf path of a trie
// (fvqa/constrain.py TokenTrie), every internal node of the trie is ONE row of one pass through the layers (the attention is
// fvqa_attn_suffix_tree, csrc/score.hip, with the other suffix attentions), and the LM head runs on those rows only, in blocks of
// rows so that the fp32 logits stay bounded. One kernel here turns the rows' logits into the answers' log-probabilities:
//
// fvqa_trie_score — one workgroup per sample, two steps.
//   edges    lp[e] = logits[parent row of e][token of e] - lse[parent row of e] for the edges whose parent row lies in the block of
//            rows this launch was handed (lse: fvqa_ce_fwd's, the one implementation). A launch per block of the head; a launch
//            without logits takes lp as it stands (the dense route of score_vocab fills it from its per-token losses).
//   members  (reduce != 0: the last launch) one thread walks one member: the sum of lp along its path, root first, in fp32 — at most
//            32 steps —, count = its length, mean = sum / count; then per sample log_posterior = sum - logsumexp(sums), and the
//            best `top` members by mean (by_mean) or by sum, best first: the larger key wins, a NaN key beats every number (torch's
//            rule, as fvqa_option_pick's argmin has it), ties and NaNs among themselves go to the member listed first.
//   Fixed order everywhere (a thread's members in ascending order, the butterfly of common.h across threads, the ranking by a total
//   order on (key, slot)), no float atomics: two launches give the same bits. Every index read from the plan's arrays is clamped.
#include "common.h"

namespace {

constexpr int PATH = FVQA_TREE_DEPTH_MAX + 1;          // edges of the longest member (EOS included)
constexpr int MMAX = FVQA_TREE_ROWS_MAX;               // members per sample: their sums and keys stay in LDS (2 x 16 KiB)
constexpr int TOPMAX = 8;

__device__ __forceinline__ bool is_nan(float x) { return x != x; }
// does (ka, a) rank in front of (kb, b)? slot < 0: no candidate
__device__ __forceinline__ bool in_front(float ka, int a, float kb, int b) {
  if (a < 0) return false;
  if (b < 0) return true;
  const bool na = is_nan(ka), nb = is_nan(kb);
  if (na != nb) return na;
  if (!na && ka != kb) return ka > kb;
  return a < b;
}

__global__ __launch_bounds__(256) void trie_score_k(const float* __restrict__ logits, const float* __restrict__ lse, int row0,
                                                    int n_blk, const int32_t* __restrict__ edge_parent,
                                                    const int32_t* __restrict__ edge_token, const int32_t* __restrict__ n_edges,
                                                    float* __restrict__ edge_lp, const int32_t* __restrict__ member_path,
                                                    const int32_t* __restrict__ member_len, const int32_t* __restrict__ member_index,
                                                    const int32_t* __restrict__ n_members, float* __restrict__ sum_o,
                                                    int64_t* __restrict__ cnt_o, float* __restrict__ mean_o, float* __restrict__ post_o,
                                                    int64_t* __restrict__ rank_o, int64_t* __restrict__ pred_o, int R, int E, int MU,
                                                    int M, int V, int top, int by_mean, int reduce) {
  __shared__ float s_sum[MMAX], s_key[MMAX];
  __shared__ float red[4];
  __shared__ float w_key[4];
  __shared__ int w_slot[4];
  const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  int nE = n_edges[n];
  nE = nE < 0 ? 0 : (nE > E ? E : nE);
  float* lp = edge_lp + (size_t)n * E;
  if (logits) {
    for (int e = tid; e < nE; e += 256) {
      int p = edge_parent[(size_t)n * E + e];
      p = p < 0 ? 0 : (p >= R ? R - 1 : p);
      const long long g = (long long)n * R + p - row0;   // the parent's row of this launch's block
      if (g < 0 || g >= n_blk) continue;
      int t = edge_token[(size_t)n * E + e];
      t = t < 0 ? 0 : (t >= V ? V - 1 : t);
      lp[e] = logits[(size_t)g * V + t] - lse[g];
    }
  }
  if (!reduce) return;
  int nM = n_members[n];
  nM = nM < 0 ? 0 : (nM > MU ? MU : nM);
  const float ninf = -__builtin_inff();
  for (int c = tid; c < M; c += 256) {
    sum_o[(size_t)n * M + c] = ninf;
    mean_o[(size_t)n * M + c] = ninf;
    post_o[(size_t)n * M + c] = ninf;
    cnt_o[(size_t)n * M + c] = 0;
  }
  __syncthreads();                                       // lp and the cleared columns are written
  float mx = ninf;
  for (int m = tid; m < nM; m += 256) {
    int len = member_len[(size_t)n * MU + m];
    len = len < 1 ? 1 : (len > PATH ? PATH : len);
    const int32_t* path = member_path + ((size_t)n * MU + m) * PATH;
    float s = 0.f;
    for (int i = 0; i < len; ++i) {
      int e = path[i];
      e = e < 0 ? 0 : (e >= nE ? nE - 1 : e);
      s += nE > 0 ? lp[e] : 0.f;
    }
    const float mean = s / (float)len;
    s_sum[m] = s;
    s_key[m] = by_mean ? mean : s;
    mx = fmaxf(mx, s);
    int c = member_index[(size_t)n * MU + m];
    c = c < 0 ? 0 : (c >= M ? M - 1 : c);
    sum_o[(size_t)n * M + c] = s;
    mean_o[(size_t)n * M + c] = mean;
    cnt_o[(size_t)n * M + c] = len;
  }
  mx = block_max_256(mx, red);
  float z = 0.f;
  for (int m = tid; m < nM; m += 256) z += expf(s_sum[m] - mx);
  __syncthreads();                                       // (red is read by every thread before it is written again)
  z = block_sum_256(z, red);
  const float lz = mx + logf(z);
  for (int m = tid; m < nM; m += 256) {
    int c = member_index[(size_t)n * MU + m];
    c = c < 0 ? 0 : (c >= M ? M - 1 : c);
    post_o[(size_t)n * M + c] = s_sum[m] - lz;
  }
  // ---- the best `top` members, one round each: the thread's best, the wave's, the workgroup's; the winner leaves the field
  __shared__ int taken[TOPMAX];
  for (int r = 0; r < top; ++r) {
    float bk = 0.f;
    int bs = -1;
    for (int m = tid; m < nM; m += 256) {
      bool free_ = true;
      for (int i = 0; i < r; ++i) free_ = free_ && taken[i] != m;
      if (free_ && in_front(s_key[m], m, bk, bs)) { bk = s_key[m]; bs = m; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ok = __shfl_xor(bk, o, 64);
      const int os = __shfl_xor(bs, o, 64);
      if (in_front(ok, os, bk, bs)) { bk = ok; bs = os; }
    }
    if (lane == 0) { w_key[w] = bk; w_slot[w] = bs; }
    __syncthreads();
    if (tid == 0) {
      for (int i = 1; i < 4; ++i)
        if (in_front(w_key[i], w_slot[i], bk, bs)) { bk = w_key[i]; bs = w_slot[i]; }
      taken[r] = bs;
      int64_t c = -1;
      if (bs >= 0) {
        const int ci = member_index[(size_t)n * MU + bs];
        c = ci < 0 ? 0 : (ci >= M ? M - 1 : ci);
      }
      rank_o[(size_t)n * top + r] = c;
      if (r == 0) pred_o[n] = c < 0 ? 0 : c;
    }
    __syncthreads();
  }
}

}  // namespace

extern "C" int fvqa_trie_score(const float* logits, const float* lse, int row0, int n_block_rows, const int32_t* edge_parent,
                               const int32_t* edge_token, const int32_t* n_edges, float* edge_lp, const int32_t* member_path,
                               const int32_t* member_len, const int32_t* member_index, const int32_t* n_members, float* sum,
                               int64_t* count, float* mean, float* log_posterior, int64_t* ranking, int64_t* prediction,
                               int n_seq, int rows, int max_edges, int max_members, int n_columns, int vocab, int top,
                               int by_mean, int reduce, void* stream) {
  if (!edge_parent || !edge_token || !n_edges || !edge_lp) return FVQA_EINVAL;
  if (!logits != !lse) return FVQA_EINVAL;
  if (reduce && (!member_path || !member_len || !member_index || !n_members || !sum || !count || !mean || !log_posterior ||
                 !ranking || !prediction))
    return FVQA_EINVAL;
  if (!logits && !reduce) return FVQA_EINVAL;            // (a launch with nothing to do)
  if (n_seq <= 0 || n_seq > 65535 || rows <= 0 || rows > FVQA_TREE_ROWS_MAX || max_edges <= 0 || vocab <= 0 || row0 < 0 ||
      n_block_rows < 0 || (long long)n_seq * rows > FVQA_TREE_TOTAL_ROWS_MAX)
    return FVQA_ESHAPE;
  if ((long long)n_seq * max_edges > 0x7fffffffLL) return FVQA_ESHAPE;
  if (logits && (n_block_rows == 0 || (long long)row0 + n_block_rows > (long long)n_seq * rows)) return FVQA_ESHAPE;
  if (reduce && (max_members <= 0 || max_members > MMAX || n_columns <= 0 || top < 1 || top > TOPMAX ||
                 (long long)n_seq * n_columns > 0x7fffffffLL))
    return FVQA_ESHAPE;
  if (!fvqa_aligned(4, logits, lse, edge_parent, edge_token, n_edges, edge_lp, member_path, member_len, member_index, n_members,
                    sum, mean, log_posterior) || !fvqa_aligned(8, count, ranking, prediction))
    return FVQA_EALIGN;
  hipLaunchKernelGGL(trie_score_k, dim3(n_seq), dim3(256), 0, (hipStream_t)stream, logits, lse, row0, n_block_rows, edge_parent,
                     edge_token, n_edges, edge_lp, member_path, member_len, member_index, n_members, sum, count, mean,
                     log_posterior, ranking, prediction, rows, max_edges, max_members, n_columns, vocab, top, by_mean, reduce);
  FVQA_CHECK_LAUNCH();
  return FVQA_OK;
}
