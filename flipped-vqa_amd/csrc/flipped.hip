// Option scoring by all three flipped tasks (fvqa/flipped.py): the answer options of a sample are ranked by the VQA loss, by the
// VAQ loss (the question predicted from the clip and each candidate answer) and by the QAV loss (the frame order predicted from
// the question and each candidate answer). A VAQ option differs at its answer and the scored question follows it, a QAV option
// has its frame slots behind the answer: the suffix rows of these streams are many more than fvqa_attn_suffix's 16, and they are
// not all token embeddings. Three kernels serve that:
//
// fvqa_attn_suffix_wide — fvqa_attn_suffix (csrc/score.hip: same operands, same semantics) for 1 <= suffix_len <= 64. Query row
//   (n, c, j) sits at position start[n] + j and attends to the cached keys / values [0, start[n]) of sample n, to rows 0..j of
//   its OWN option's suffix (rotated here and rounded to the storage type, as the prefill holds them) and to the A adapter keys
//   (own softmax scaled by tanh(gate1[h])); gate2[h] is added on the frame keys [vs, vs + F) when the query position is
//   >= vs + F, wherever that window lies — in the cache, across start[n] or inside the suffix; vs < 0: no window.
//   One 256-thread workgroup per (head, sample, option x tile of 32 queries): fvqa_attn_suffix's (head, sample) workgroup would
//   walk O * T / 32 = 10 tiles in a row at five options of 64 rows; here the tiles run side by side and the prompt's keys are
//   read once per tile, from L2 after the first. A tile stages the suffix keys of its own option up to its last query only.
//   Keys in chunks of 32 in LDS as fp32, a running (max, sum) per query: the sums run in one fixed order, no atomics, two
//   launches give the same bits. Rows j >= len[n] are padding: never loaded, their output rows are zeros.
//
// fvqa_suffix_embed — the suffix rows' inputs in one launch: row (n, c, j) is the token embedding of its id, or the bits of
//   vf_tok[n, f] where the slot map names frame f (the QAV frame rows: llama/model.py:335-336 zeroes the row and adds the frame
//   token), or zeros for j >= len[n].
//
// fvqa_flipped_pick — per sample: total = sum over the requested tasks of w_t * mean_t (fp32, in the order vqa, vaq, qav, no
//   contraction), the argmin over the eligible options of the total and of each task's mean, and each task's mean at the gold
//   option. One workgroup per sample.
#include "attn_decode_body.h"

namespace {
using namespace fvqa_decode;

#include "suffix_rows.h"                 // QT, KC, KLD, load16, rope16, store16, half_max, half_sum
constexpr int TWIDE = 64;                // suffix rows per option

template <typename T>
__global__ __launch_bounds__(256) void attn_suffix_wide_k(const T* __restrict__ suf, const T* __restrict__ cache,
                                                          T* __restrict__ o_suf, const float* __restrict__ gate1,
                                                          const float* __restrict__ gate2, const int32_t* __restrict__ vstart,
                                                          const int32_t* __restrict__ start_p, const int32_t* __restrict__ len_p,
                                                          const float* __restrict__ cs, const float* __restrict__ sn, int B, int O,
                                                          int Tn, int S, int H, int A, int F, int cache_rot) {
  __shared__ __attribute__((aligned(16))) float Qs[QT][KLD];     // the tile's queries: rotated, rounded
  __shared__ __attribute__((aligned(16))) float Ks[KC][KLD];     // the chunk's keys, as the prefill holds them
  __shared__ __attribute__((aligned(16))) float Vs[KC][DH];
  __shared__ __attribute__((aligned(16))) float Ps[QT][KC];      // the chunk's probabilities (unnormalised)
  __shared__ float mrun[QT], lrun[QT], alpha[QT];
  const int tid = threadIdx.x;
  const int h = blockIdx.x, n = blockIdx.y;
  const int NT = (Tn + QT - 1) / QT;
  const int c = blockIdx.z / NT, j0 = (blockIdx.z % NT) * QT;    // the option, the tile's first suffix row
  const int D = H * DH;
  const size_t ld = (size_t)3 * D;
  int start = start_p[n];
  start = start < 0 ? 0 : (start > S ? S : start);
  int len = len_p[n];
  len = len < 0 ? 0 : (len > Tn ? Tn : len);
  if (len > S - start) len = S - start;
  const size_t row0 = ((size_t)n * O + c) * Tn;                  // the option's first row in qkv_suf / o_suf
  const T* seq = cache + (size_t)n * S * ld + h * DH;
  const T* arow = cache + (size_t)B * S * ld + h * DH;
  const T* sufc = suf + row0 * ld + h * DH;
  const float scale = rsqrtf((float)DH);
  const int vs = vstart[n];
  const float g2 = gate2[h];
  const float tg1 = tanhf(gate1[h]);
  // staging role: 8 threads per row, 16 head dims each
  const int srow = tid >> 3, sd0 = (tid & 7) * 16;
  // score role: key column kk, queries 4*qg .. 4*qg + 3
  const int kk = tid & 31, qg = tid >> 5;
  // value role: head dim vd, queries 16*qh .. 16*qh + 15
  const int vd = tid & 127, qh = tid >> 7;

  if (j0 >= len) {                                       // a tile of padding rows (the whole workgroup takes this branch)
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const int j = j0 + 16 * qh + u;
      if (j < Tn) o_suf[(row0 + j) * D + h * DH + vd] = from_f32<T>(0.f);
    }
    return;
  }
  // ---- the tile's queries
  {
    const int j = j0 + srow;
    float v[16];
    if (j < len) {
      load16<T>(sufc + (size_t)j * ld + sd0, v);
      rope16<T>(v, cs, sn, start + j, sd0);
    } else {
#pragma unroll
      for (int e = 0; e < 16; ++e) v[e] = 0.f;
    }
    store16(&Qs[srow][sd0], v);
    if (tid < QT) { mrun[tid] = -1e30f; lrun[tid] = 0.f; }
  }
  float acc[16];
#pragma unroll
  for (int u = 0; u < 16; ++u) acc[u] = 0.f;
  int qj[4];
  bool qok[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    qj[u] = j0 + 4 * qg + u;
    qok[u] = qj[u] < len;
  }
  // the suffix keys a query of this tile can see: rows 0 .. its own, of its own option
  const int s_hi = j0 + QT < len ? j0 + QT : len;
  const int n_pre = (start + KC - 1) / KC, n_suf = (s_hi + KC - 1) / KC;
  // chunks: [0, n_pre) cached prompt keys, [n_pre, n_pre + n_suf) suffix keys, then the adapter keys (own softmax)
  for (int ch = 0; ch <= n_pre + n_suf; ++ch) {
    const int kind = ch < n_pre ? 0 : (ch < n_pre + n_suf ? 1 : 2);
    const int k0 = kind == 0 ? ch * KC : (kind == 1 ? (ch - n_pre) * KC : 0);
    __syncthreads();                                     // the previous chunk's readers are done (and Qs / mrun are written)
    if (kind == 2 && tid < QT) {                         // text softmax closed: o = acc / l, then the adapter's share is added
      alpha[tid] = lrun[tid] > 0.f ? 1.f / lrun[tid] : 0.f;
      mrun[tid] = -1e30f;
    }
    // ---- stage the chunk's keys and values
    {
      const int ki = k0 + srow;
      float k[16], v[16];
      const T* row = nullptr;
      int pos = 0;
      bool rot = false;
      if (kind == 0) {
        if (ki < start) { row = seq + (size_t)ki * ld; pos = ki; rot = !cache_rot; }
      } else if (kind == 1) {
        if (ki < s_hi) { row = sufc + (size_t)ki * ld; pos = start + ki; rot = true; }     // pos < S: len <= S - start
      } else if (ki < A) {
        row = arow + (size_t)ki * ld;
      }
      if (row) {
        load16<T>(row + D + sd0, k);
        load16<T>(row + 2 * D + sd0, v);
        if (rot) rope16<T>(k, cs, sn, pos, sd0);
      } else {
#pragma unroll
        for (int e = 0; e < 16; ++e) k[e] = v[e] = 0.f;
      }
      store16(&Ks[srow][sd0], k);
      store16(&Vs[srow][sd0], v);
    }
    __syncthreads();
    // ---- scores of (4 queries) x (key kk)
    float s[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
    for (int d = 0; d < DH; d += 4) {
      const float4 k4 = *reinterpret_cast<const float4*>(&Ks[kk][d]);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const float4 q4 = *reinterpret_cast<const float4*>(&Qs[4 * qg + u][d]);
        s[u] += q4.x * k4.x + q4.y * k4.y + q4.z * k4.z + q4.w * k4.w;
      }
    }
    const int ki = k0 + kk;
    const int kpos = kind == 1 ? start + ki : ki;
    const bool kok = kind == 0 ? ki < start : (kind == 1 ? ki < s_hi : ki < A);
    const bool frame_key = kind != 2 && vs >= 0 && kpos >= vs && kpos < vs + F;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      bool see = qok[u] && kok;
      if (kind == 1) see = see && ki <= qj[u];
      float x = s[u] * scale;
      if (frame_key && start + qj[u] >= vs + F) x += g2;
      x = see ? x : -1e30f;
      const int q = 4 * qg + u;
      const float m_old = mrun[q];
      const float m_new = fmaxf(m_old, half_max(x));
      const float e = see ? __expf(x - m_new) : 0.f;
      const float sum = half_sum(e);
      if (kind == 2) {
        Ps[q][kk] = sum > 0.f ? e / sum * tg1 : 0.f;
      } else {
        Ps[q][kk] = e;
        if (kk == 0) {
          const float a = __expf(m_old - m_new);
          alpha[q] = a;
          lrun[q] = lrun[q] * a + sum;
        }
      }
      if (kk == 0) mrun[q] = m_new;        // (read above by this half wave only: each query belongs to one)
    }
    __syncthreads();
    // ---- values: acc[q] = acc[q] * alpha[q] + sum_k P[q][k] V[k][vd]
    float vcol[KC];
#pragma unroll
    for (int k = 0; k < KC; ++k) vcol[k] = Vs[k][vd];
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const int q = 16 * qh + u;
      float a = acc[u] * alpha[q];
#pragma unroll
      for (int k = 0; k < KC; k += 4) {
        const float4 p4 = *reinterpret_cast<const float4*>(&Ps[q][k]);
        a += p4.x * vcol[k];
        a += p4.y * vcol[k + 1];
        a += p4.z * vcol[k + 2];
        a += p4.w * vcol[k + 3];
      }
      acc[u] = a;
    }
  }
  // ---- the tile's output rows (padding rows: zeros)
#pragma unroll
  for (int u = 0; u < 16; ++u) {
    const int j = j0 + 16 * qh + u;
    if (j < Tn) o_suf[(row0 + j) * D + h * DH + vd] = from_f32<T>(j < len ? acc[u] : 0.f);
  }
}

// one workgroup per suffix row: 16 bytes per thread and step
template <typename T>
__global__ __launch_bounds__(256) void suffix_embed_k(const int64_t* __restrict__ ids, const int32_t* __restrict__ slot,
                                                      const T* __restrict__ emb, const T* __restrict__ vf_tok,
                                                      const int32_t* __restrict__ len_p, T* __restrict__ x, int O, int Tn, int D,
                                                      int V, int F) {
  const size_t r = blockIdx.x;
  const int j = (int)(r % Tn), n = (int)(r / ((size_t)O * Tn));
  const int f = slot ? slot[r] : -1;
  const T* src = nullptr;
  if (j < len_p[n]) {
    if (f >= 0) {
      src = vf_tok + ((size_t)n * F + (f < F ? f : F - 1)) * D;
    } else {
      int64_t id = ids[r];
      id = id < 0 ? 0 : (id >= V ? V - 1 : id);          // (the host checks the range; never read outside the table)
      src = emb + (size_t)id * D;
    }
  }
  constexpr int E = 16 / sizeof(T);
  uint4* dst = reinterpret_cast<uint4*>(x + r * D);
  for (int i = threadIdx.x; i < D / E; i += 256)
    dst[i] = src ? reinterpret_cast<const uint4*>(src)[i] : make_uint4(0u, 0u, 0u, 0u);
}

constexpr int OMAX = 64;                 // options (fvqa_option_pick's limit)

// argmin with torch's rule over the options with ok[c]: the first NaN wins, ties stay with the lowest index; 0 when none is ok
__device__ int pick_of(const float* v, const bool* ok, int O) {
  int best = -1;
  for (int c = 0; c < O; ++c) {
    if (!ok[c]) continue;
    const float x = v[c];
    if (x != x) return c;
    if (best < 0 || x < v[best]) best = c;
  }
  return best < 0 ? 0 : best;
}

__global__ __launch_bounds__(64) void flipped_pick_k(const float* __restrict__ m0, const float* __restrict__ m1,
                                                     const float* __restrict__ m2, const int64_t* __restrict__ c0,
                                                     const int64_t* __restrict__ c1, const int64_t* __restrict__ c2, float w0,
                                                     float w1, float w2, const int64_t* __restrict__ answer,
                                                     float* __restrict__ total, int64_t* __restrict__ pred,
                                                     int64_t* __restrict__ pred_t, float* __restrict__ gold, int B, int O) {
#pragma clang fp contract(off)
  __shared__ float tot[OMAX], mt[3][OMAX];
  __shared__ bool all_ok[OMAX], ok_t[3][OMAX];
  const int n = blockIdx.x, c = threadIdx.x;
  const float* mean[3] = {m0, m1, m2};
  const int64_t* cnt[3] = {c0, c1, c2};
  const float w[3] = {w0, w1, w2};
  if (c < O) {
    float t = 0.f;
    bool ok = true;
    for (int k = 0; k < 3; ++k) {
      ok_t[k][c] = false;
      mt[k][c] = 0.f;
      if (!mean[k]) continue;
      const float m = mean[k][n * O + c];
      const bool has = cnt[k][n * O + c] > 0;
      t = t + w[k] * m;                                  // fp32, in the order vqa, vaq, qav
      mt[k][c] = m;
      ok_t[k][c] = has;
      ok = ok && has;
    }
    tot[c] = t;
    all_ok[c] = ok;
    total[n * O + c] = t;
  }
  __syncthreads();
  if (c == 0) pred[n] = pick_of(tot, all_ok, O);
  if (c >= 1 && c <= 3) {
    const int k = c - 1;
    pred_t[(size_t)k * B + n] = mean[k] ? pick_of(mt[k], ok_t[k], O) : -1;
    if (gold) {
      const int64_t a = answer[n];
      gold[n * 3 + k] = mean[k] && a >= 0 && a < O ? mt[k][a] : __builtin_nanf("");
    }
  }
}

}  // namespace

extern "C" int fvqa_attn_suffix_wide(const void* qkv_suf, const void* qkv_cache, void* o_suf, const float* gate1,
                                     const float* gate2, const int32_t* vstart, const int32_t* start, const int32_t* len,
                                     const float* cos_t, const float* sin_t, int n_seq, int n_options, int suffix_len,
                                     int seq_len, int n_heads, int head_dim, int adapter_len, int max_feats, int cache_rotated,
                                     int dtype, void* stream) {
  if (!qkv_suf || !qkv_cache || !o_suf || !gate1 || !gate2 || !vstart || !start || !len || !cos_t || !sin_t)
    return FVQA_EINVAL;
  if (!fvqa_dtype_ok(dtype)) return FVQA_EINVAL;
  if (n_seq <= 0 || n_options <= 0 || suffix_len <= 0 || suffix_len > TWIDE || seq_len <= 0 || n_heads <= 0 ||
      head_dim != DH || adapter_len < 0 || adapter_len > 16 || max_feats < 0)
    return FVQA_ESHAPE;
  if (seq_len > SMAX || n_heads > 65535 || n_seq > 65535 || n_options > 4096) return FVQA_ESHAPE;
  const int tiles = (suffix_len + QT - 1) / QT;             // (n_options * tiles <= 8192: inside the grid's third axis)
  if (((uintptr_t)qkv_suf | (uintptr_t)qkv_cache | (uintptr_t)o_suf) & 15) return FVQA_EALIGN;
  dim3 grid(n_heads, n_seq, n_options * tiles), block(256);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == FVQA_H16)
    hipLaunchKernelGGL(attn_suffix_wide_k<bf16_t>, grid, block, 0, st, (const bf16_t*)qkv_suf, (const bf16_t*)qkv_cache,
                       (bf16_t*)o_suf, gate1, gate2, vstart, start, len, cos_t, sin_t, n_seq, n_options, suffix_len, seq_len,
                       n_heads, adapter_len, max_feats, cache_rotated);
  else
    hipLaunchKernelGGL(attn_suffix_wide_k<float>, grid, block, 0, st, (const float*)qkv_suf, (const float*)qkv_cache,
                       (float*)o_suf, gate1, gate2, vstart, start, len, cos_t, sin_t, n_seq, n_options, suffix_len, seq_len,
                       n_heads, adapter_len, max_feats, cache_rotated);
  FVQA_CHECK_LAUNCH();
  return FVQA_OK;
}

extern "C" int fvqa_suffix_embed(const int64_t* ids, const int32_t* slot, const void* emb, const void* vf_tok,
                                 const int32_t* len, void* x, int n_seq, int n_options, int suffix_len, int dim, int vocab,
                                 int max_feats, int dtype, void* stream) {
  if (!ids || !emb || !len || !x || (slot && !vf_tok)) return FVQA_EINVAL;
  if (!fvqa_dtype_ok(dtype)) return FVQA_EINVAL;
  if (n_seq <= 0 || n_options <= 0 || suffix_len <= 0 || dim <= 0 || vocab <= 0 || max_feats < 0 || (slot && max_feats == 0))
    return FVQA_ESHAPE;
  if ((long long)n_seq * n_options * suffix_len > 0x7fffffffLL) return FVQA_ESHAPE;
  const int esz = dtype == FVQA_F32 ? 4 : 2;
  if ((dim * esz) % 16) return FVQA_ESHAPE;
  if (((uintptr_t)emb | (uintptr_t)vf_tok | (uintptr_t)x) & 15) return FVQA_EALIGN;
  dim3 grid(n_seq * n_options * suffix_len), block(256);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == FVQA_H16)
    hipLaunchKernelGGL(suffix_embed_k<bf16_t>, grid, block, 0, st, ids, slot, (const bf16_t*)emb, (const bf16_t*)vf_tok, len,
                       (bf16_t*)x, n_options, suffix_len, dim, vocab, max_feats);
  else
    hipLaunchKernelGGL(suffix_embed_k<float>, grid, block, 0, st, ids, slot, (const float*)emb, (const float*)vf_tok, len,
                       (float*)x, n_options, suffix_len, dim, vocab, max_feats);
  FVQA_CHECK_LAUNCH();
  return FVQA_OK;
}

extern "C" int fvqa_flipped_pick(const float* mean_vqa, const float* mean_vaq, const float* mean_qav, const int64_t* count_vqa,
                                 const int64_t* count_vaq, const int64_t* count_qav, float w_vqa, float w_vaq, float w_qav,
                                 const int64_t* answer, float* total, int64_t* prediction, int64_t* prediction_t,
                                 float* gold_loss, int n_seq, int n_options, void* stream) {
  if (!total || !prediction || !prediction_t) return FVQA_EINVAL;
  if (!mean_vqa && !mean_vaq && !mean_qav) return FVQA_EINVAL;
  if ((!mean_vqa != !count_vqa) || (!mean_vaq != !count_vaq) || (!mean_qav != !count_qav)) return FVQA_EINVAL;
  if (!answer != !gold_loss) return FVQA_EINVAL;         // the gold option's losses come with the answers
  if (n_seq <= 0 || n_seq > 65535 || n_options <= 0 || n_options > OMAX) return FVQA_ESHAPE;
  hipLaunchKernelGGL(flipped_pick_k, dim3(n_seq), dim3(64), 0, (hipStream_t)stream, mean_vqa, mean_vaq, mean_qav, count_vqa,
                     count_vaq, count_qav, w_vqa, w_vaq, w_qav, answer, total, prediction, prediction_t, gold_loss, n_seq,
                     n_options);
  FVQA_CHECK_LAUNCH();
  return FVQA_OK;
}
