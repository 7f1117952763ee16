// One-query-row attention for the generation path (reference llama/model.py:428-470 re-runs the whole sequence for
// every new token; Attention.forward :87-128 is what each of those runs evaluates at the new row).
//
// Decode shape: one new token per sequence. For sequence n at position p = pos[n] and head h the kernel takes the RAW
// q / k / v projections of the new token (qkv_row), rotates q and k (RoPE at position p), attends over
//   * the A adapter keys / values (no RoPE, own softmax scaled by tanh(gate1[h]), llama/model.py:98-100,115) and
//   * the cached keys / values 0..p-1 of the sequence plus the new token's own (causal softmax, gate2[h] added on the
//     frame columns [vs, vs+F) when p >= vs+F, llama/model.py:116-120),
// writes the output row, and stores the new token's k and v into the cache row n*S + p of the layer's qkv arena —
// what the full-sequence kernel + two torch index ops did per token and layer before (13.5 us + glue for 256 (n, h)
// pairs against one streaming pass over 64 KiB of cached K/V per pair here).
// HBM-bound (K/V read once: 2 * (p+1+A) * 256 B per pair); no matrix cores: a 1-row product has nothing to feed them.
// cache_rot: 1 = the cache holds ROTATED k — the fp32 vector build, and the bf16 build when the QKV projection rotates q, k in
// its epilogue (fvqa_rope_in_gemm, the default); 0 = RAW k (bf16 build with FVQA_ROPE_IN_GEMM=0: the attention kernels
// rotate on the fly). The caller's rule: cache_rotated = !fvqa_attn_rope_fused(dtype) || fvqa_rope_in_gemm(dtype). The new
// token's rotated q and k are rounded to the storage type before use, as the prefill's are. One workgroup (4 waves) per (head, sequence): a quad of lanes per key in the score pass (64-byte
// contiguous reads per quad), one lane per pair of head dims in the value pass (256-byte rows per wave instruction).
#include "attn_decode_body.h"

namespace {
using namespace fvqa_decode;

template <typename T>
__global__ __launch_bounds__(256) void attn_decode_k(const T* __restrict__ qkv_row, T* __restrict__ cache,
                                                     T* __restrict__ o_row, const float* __restrict__ gate1,
                                                     const float* __restrict__ gate2,
                                                     const int32_t* __restrict__ vstart, const int64_t* __restrict__ pos,
                                                     const float* __restrict__ cs, const float* __restrict__ sn,
                                                     int n_seq, int S, int H, int A, int F, int cache_rot) {
  __shared__ float sc[SMAX];                       // text scores, then probabilities
  __shared__ float sa[16];                         // adapter scores, then probabilities (x tanh gate1)
  __shared__ float red[8];
  __shared__ float part[4][DH];
  attn_decode_body<T>(qkv_row, cache, o_row, gate1, gate2, vstart, pos, cs, sn, n_seq, S, H, A, F, cache_rot,
                      (int)blockIdx.x, (int)blockIdx.y, sc, sa, red, part);
}

// attn_decode_k with the body's MASS switch on: the same output row and cache stores, and the row's frame-attention summary.
template <typename T>
__global__ __launch_bounds__(256) void attn_decode_mass_k(const T* __restrict__ qkv_row, T* __restrict__ cache,
                                                          T* __restrict__ o_row, const float* __restrict__ gate1,
                                                          const float* __restrict__ gate2,
                                                          const int32_t* __restrict__ vstart,
                                                          const int64_t* __restrict__ pos, const float* __restrict__ cs,
                                                          const float* __restrict__ sn, int n_seq, int S, int H, int A, int F,
                                                          int cache_rot, float* __restrict__ mass) {
  __shared__ float sc[SMAX];
  __shared__ float sa[16];
  __shared__ float red[8];
  __shared__ float part[4][DH];
  __shared__ float mred[8];                        // the two masked sums, one partial per wave
  attn_decode_body<T, false, true>(qkv_row, cache, o_row, gate1, gate2, vstart, pos, cs, sn, n_seq, S, H, A, F, cache_rot,
                                   (int)blockIdx.x, (int)blockIdx.y, sc, sa, red, part, mass, mred);
}

// The summary for rows that already sit in an arena (q | k | v of every row, q and k in ONE convention: both rotated when
// cache_rot, both raw otherwise): workgroup (head h, row r) takes the query of position pos[r] of sequence seq[r] and runs
// attn_decode_body's score pass and softmax over the keys 0..p of that sequence — key p from the arena as well. No values are
// loaded and nothing is stored but mass (R, H, F + 2).
template <typename T>
__global__ __launch_bounds__(256) void attn_row_mass_k(const T* __restrict__ qkv, const int32_t* __restrict__ seq_of,
                                                       const int32_t* __restrict__ pos, const float* __restrict__ gate2,
                                                       const int32_t* __restrict__ vstart, const float* __restrict__ cs,
                                                       const float* __restrict__ sn, int n_seq, int S, int H, int F,
                                                       int cache_rot, float* __restrict__ mass) {
  __shared__ float sc[SMAX];
  __shared__ float red[8];
  __shared__ float mred[8];
  constexpr int CH = Chunk<T>::CH;
  constexpr int NCH = DH / CH;
  constexpr int CPL = NCH / 4;
  const int h = blockIdx.x, r = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int D = H * DH;
  const size_t ld = (size_t)3 * D;
  int n = seq_of[r], p = pos[r];
  n = n < 0 ? 0 : (n >= n_seq ? n_seq - 1 : n);
  p = p < 0 ? 0 : (p >= S ? S - 1 : p);
  const T* seq = qkv + (size_t)n * S * ld + h * DH;
  const float scale = rsqrtf((float)DH);
  const int vs = vstart[n];
  const bool biased_row = vs >= 0 && p >= vs + F;
  const float g2 = gate2[h];
  const int part_id = lane & 3, slot = lane >> 2;
  float q[CPL][CH];
#pragma unroll
  for (int u = 0; u < CPL; ++u) {
    const int c = part_id + 4 * u;
    Chunk<T>::load(seq + (size_t)p * ld + c * CH, q[u]);
    rope_chunk<CH>(q[u], cs, sn, p, c * CH, !cache_rot);
#pragma unroll
    for (int e = 0; e < CH; ++e) q[u][e] = round_to<T>(q[u][e]);     // (a rotated row is in the storage type already)
  }
  auto score = [&](int j) {
    const int jj = j < p ? j : p;
    const T* krow = seq + (size_t)jj * ld + D;
    float acc = 0.f;
#pragma unroll
    for (int u = 0; u < CPL; ++u) {
      const int c = part_id + 4 * u;
      float k[CH];
      Chunk<T>::load(krow + c * CH, k);
      rope_chunk<CH>(k, cs, sn, jj, c * CH, !cache_rot);
#pragma unroll
      for (int e = 0; e < CH; ++e) acc += q[u][e] * (cache_rot ? k[e] : round_to<T>(k[e]));
    }
    float x = quad_sum(acc) * scale;
    if (biased_row && jj >= vs && jj < vs + F) x += g2;
    if (j <= p && part_id == 0) sc[j] = x;
  };
  score(w * 16 + slot);
  score(64 + w * 16 + slot);
  for (int j0 = 128; j0 <= p; j0 += 64) score(j0 + w * 16 + slot);
  __syncthreads();
  float mx = -1e30f;
  for (int j = tid; j <= p; j += 256) mx = fmaxf(mx, sc[j]);
  mx = wave_max(mx);
  if (lane == 0) red[w] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  float sum = 0.f;
  for (int j = tid; j <= p; j += 256) {
    const float e = __expf(sc[j] - mx);
    sc[j] = e;
    sum += e;
  }
  sum = wave_sum(sum);
  if (lane == 0) red[4 + w] = sum;
  __syncthreads();
  const float inv = 1.f / ((red[4] + red[5]) + (red[6] + red[7]));
  float* out = mass + ((size_t)r * H + h) * (F + 2);
  mass_partials(sc, inv, p, vs, F, out, mred);
  __syncthreads();
  if (tid == 0) mass_finish(F, out, mred);
}

}  // namespace

extern "C" int fvqa_attn_decode_mass(const void* qkv_row, void* qkv_cache, void* o_row, const float* gate1,
                                     const float* gate2, const int32_t* vstart, const int64_t* pos, const float* cos_t,
                                     const float* sin_t, float* mass, int n_seq, int seq_len, int n_heads, int head_dim,
                                     int adapter_len, int max_feats, int cache_rotated, int dtype, void* stream) {
  if (!qkv_row || !qkv_cache || !o_row || !gate1 || !gate2 || !vstart || !pos || !cos_t || !sin_t || !mass) return FVQA_EINVAL;
  if (!fvqa_dtype_ok(dtype)) return FVQA_EINVAL;
  if (n_seq <= 0 || seq_len <= 0 || n_heads <= 0 || head_dim != DH || adapter_len < 0 || adapter_len > 16 || max_feats < 0 ||
      max_feats > SMAX)
    return FVQA_ESHAPE;
  if (seq_len > SMAX || n_heads > 65535 || n_seq > 65535) return FVQA_ESHAPE;
  if (((uintptr_t)qkv_row | (uintptr_t)qkv_cache | (uintptr_t)o_row) & 15) return FVQA_EALIGN;
  if ((uintptr_t)mass & 3) return FVQA_EALIGN;
  dim3 grid(n_heads, n_seq), block(256);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == FVQA_H16)
    hipLaunchKernelGGL(attn_decode_mass_k<bf16_t>, grid, block, 0, st, (const bf16_t*)qkv_row, (bf16_t*)qkv_cache,
                       (bf16_t*)o_row, gate1, gate2, vstart, pos, cos_t, sin_t, n_seq, seq_len, n_heads, adapter_len,
                       max_feats, cache_rotated, mass);
  else
    hipLaunchKernelGGL(attn_decode_mass_k<float>, grid, block, 0, st, (const float*)qkv_row, (float*)qkv_cache,
                       (float*)o_row, gate1, gate2, vstart, pos, cos_t, sin_t, n_seq, seq_len, n_heads, adapter_len,
                       max_feats, cache_rotated, mass);
  FVQA_CHECK_LAUNCH();
  return FVQA_OK;
}

extern "C" int fvqa_attn_row_mass(const void* qkv, const int32_t* seq, const int32_t* pos, const float* gate2,
                                  const int32_t* vstart, const float* cos_t, const float* sin_t, float* mass, int n_rows,
                                  int n_seq, int seq_len, int n_heads, int head_dim, int adapter_len, int max_feats,
                                  int cache_rotated, int dtype, void* stream) {
  if (!qkv || !seq || !pos || !gate2 || !vstart || !cos_t || !sin_t || !mass) return FVQA_EINVAL;
  if (!fvqa_dtype_ok(dtype)) return FVQA_EINVAL;
  if (n_rows <= 0 || n_seq <= 0 || seq_len <= 0 || n_heads <= 0 || head_dim != DH || adapter_len < 0 || adapter_len > 16 ||
      max_feats < 0 || max_feats > SMAX)
    return FVQA_ESHAPE;
  if (seq_len > SMAX || n_heads > 65535 || n_seq > 65535 || n_rows > 65535) return FVQA_ESHAPE;
  if ((uintptr_t)qkv & 15) return FVQA_EALIGN;
  if (((uintptr_t)seq | (uintptr_t)pos | (uintptr_t)mass) & 3) return FVQA_EALIGN;
  dim3 grid(n_heads, n_rows), block(256);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == FVQA_H16)
    hipLaunchKernelGGL(attn_row_mass_k<bf16_t>, grid, block, 0, st, (const bf16_t*)qkv, seq, pos, gate2, vstart, cos_t, sin_t,
                       n_seq, seq_len, n_heads, max_feats, cache_rotated, mass);
  else
    hipLaunchKernelGGL(attn_row_mass_k<float>, grid, block, 0, st, (const float*)qkv, seq, pos, gate2, vstart, cos_t, sin_t,
                       n_seq, seq_len, n_heads, max_feats, cache_rotated, mass);
  FVQA_CHECK_LAUNCH();
  return FVQA_OK;
}

extern "C" int fvqa_attn_decode(const void* qkv_row, void* qkv_cache, void* o_row, const float* gate1,
                                const float* gate2, const int32_t* vstart, const int64_t* pos, const float* cos_t,
                                const float* sin_t, int n_seq, int seq_len, int n_heads, int head_dim, int adapter_len,
                                int max_feats, int cache_rotated, int dtype, void* stream) {
  if (!qkv_row || !qkv_cache || !o_row || !gate1 || !gate2 || !vstart || !pos || !cos_t || !sin_t) return FVQA_EINVAL;
  if (!fvqa_dtype_ok(dtype)) return FVQA_EINVAL;
  if (n_seq <= 0 || seq_len <= 0 || n_heads <= 0 || head_dim != DH || adapter_len < 0 || adapter_len > 16 || max_feats < 0)
    return FVQA_ESHAPE;
  if (seq_len > SMAX || n_heads > 65535 || n_seq > 65535) return FVQA_ESHAPE;
  if (((uintptr_t)qkv_row | (uintptr_t)qkv_cache | (uintptr_t)o_row) & 15) return FVQA_EALIGN;
  dim3 grid(n_heads, n_seq), block(256);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == FVQA_H16)
    hipLaunchKernelGGL(attn_decode_k<bf16_t>, grid, block, 0, st, (const bf16_t*)qkv_row, (bf16_t*)qkv_cache,
                       (bf16_t*)o_row, gate1, gate2, vstart, pos, cos_t, sin_t, n_seq, seq_len, n_heads, adapter_len,
                       max_feats, cache_rotated);
  else
    hipLaunchKernelGGL(attn_decode_k<float>, grid, block, 0, st, (const float*)qkv_row, (float*)qkv_cache,
                       (float*)o_row, gate1, gate2, vstart, pos, cos_t, sin_t, n_seq, seq_len, n_heads, adapter_len,
                       max_feats, cache_rotated);
  FVQA_CHECK_LAUNCH();
  return FVQA_OK;
}
