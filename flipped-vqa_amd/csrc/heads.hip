// Input/output heads of the Flipped-VQA step on gfx950: the front-end projections (one kernel family for the video-only
// step and the audio modes, + temporal embedding), the audio cross-attention, LM-head cross-entropy over fp32 logits, and
// the QAV frame-ordering head. All fp32 arithmetic, fixed-order reductions (no float atomics ⇒ bitwise repeatable).
#include "common.h"

namespace {

// ---- front-end projections (reference llama/model.py:209-227,306-324) -------------------------------------------------
// out[r,d] = sum over 1..2 sources of X_s[r,:]·W_s[d,:] (+ bias[d]), every operand read where it lies — a source is (pointer,
// row pitch, K), its weight (pointer, row pitch). The video-only step is one contiguous source (pitch = K, no bias), `concat`
// two sources against two column ranges of one weight, `sum` two sources against two weights, `audio_only` and the projections
// of `attention` one. One kernel family serves them all: what the video-only entries launch is the one-source instantiation.
struct ProjSrc { const float* x; const float* w; int ldx, ldw, k; };
struct ProjSrcs { ProjSrc s[2]; int n; };

// raw[r,d] on the exact-fp32 matrix cores (v_mfma_f32_16x16x4_f32: the same fma chain per output as a scalar loop over k in
// 16-element strides), then tok = cast(raw + temporal[r % F]). One workgroup per 16 output features: its 4 waves split EACH
// source's K (K_s % 64 == 0), each keeps the R <= 128 rows as 16-row MFMA blocks; the 4 partial sums meet in LDS. 256
// workgroups instead of the 32 tiles of a 128x128 GEMM at M = 80: 69 -> ~8 us. Per output the fma chain of a wave is source
// 0's k ascending, then source 1's; the four partials are added in wave order: fixed, bitwise repeatable. NSRC is a
// compile-time count: with it at run time both K-loops are live at once, 280 VGPRs and one wave per SIMD instead of two.
// OPT: bias and tok are optional and asked for at run time. The step's own projections (no bias, tokens written) launch
// OPT = false, the epilogue the video-only kernels had: with the two branches in it the same loop measured 0.7 us of 20.4
// slower here and 5 us of 163 in proj_fwd_k, where they sit in every row's chain (profiles/front_refactor.log, section 4).
template <typename T, int NSRC, bool OPT>
__global__ __launch_bounds__(256) void proj_fwd_mfma_k(ProjSrcs S, const float* __restrict__ bias,
                                                       const float* __restrict__ temporal, float* __restrict__ raw,
                                                       T* __restrict__ tok, int R, int F, int D) {
  __shared__ float part[4][8][16][17];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int li = lane & 15, g = lane >> 4;
  const int n0 = blockIdx.x * 16;
  const int nrb = (R + 15) >> 4;                           // 16-row blocks of rows (<= 8)
  int bn = n0 + li; bn = bn < D ? bn : D - 1;
  f32x4 acc[8];
#pragma unroll
  for (int b = 0; b < 8; ++b) acc[b] = f32x4{0.f, 0.f, 0.f, 0.f};
  // four k-steps of 16 per trip, every load of the trip in flight before its first MFMA (round 5: one step per trip was a chain of
  // twelve dependent load latencies, 28.9 us in the step); the accumulation order per output is unchanged (k ascending)
  constexpr int VU = 4;
#pragma unroll
  for (int s = 0; s < NSRC; ++s) {
    const ProjSrc& P = S.s[s];
    const int kw = P.k / 4;                                // this wave's K range of the source
    const float* bp = P.w + (size_t)bn * P.ldw + (size_t)w * kw + 4 * g;
    const float* ap[8];
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      int ar = b * 16 + li; ar = ar < R ? ar : R - 1;
      ap[b] = P.x + (size_t)ar * P.ldx + (size_t)w * kw + 4 * g;
    }
    for (int k0 = 0; k0 < kw; k0 += 16 * VU) {
      float4 bf[VU], af[VU][8];
#pragma unroll
      for (int u = 0; u < VU; ++u) {
        const int k = k0 + 16 * u;
        const bool in = k < kw;
        bf[u] = in ? *reinterpret_cast<const float4*>(bp + k) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int b = 0; b < 8; ++b)
          af[u][b] = (in && b < nrb) ? *reinterpret_cast<const float4*>(ap[b] + k) : make_float4(0.f, 0.f, 0.f, 0.f);
      }
#pragma unroll
      for (int u = 0; u < VU; ++u) {
        if (k0 + 16 * u >= kw) break;
#pragma unroll
        for (int b = 0; b < 8; ++b) {
          if (b >= nrb) break;
          acc[b] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[u][b].x, bf[u].x, acc[b], 0, 0, 0);     // D[row 4g+e][feature li]
          acc[b] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[u][b].y, bf[u].y, acc[b], 0, 0, 0);
          acc[b] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[u][b].z, bf[u].z, acc[b], 0, 0, 0);
          acc[b] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[u][b].w, bf[u].w, acc[b], 0, 0, 0);
        }
      }
    }
  }
#pragma unroll
  for (int b = 0; b < 8; ++b)
#pragma unroll
    for (int e = 0; e < 4; ++e) part[w][b][4 * g + e][li] = acc[b][e];
  __syncthreads();
  for (int i = threadIdx.x; i < nrb * 256; i += 256) {
    const int b = i >> 8, rr = (i >> 4) & 15, c = i & 15;
    const int r = b * 16 + rr, d = n0 + c;
    if (r < R && d < D) {
      float v = ((part[0][b][rr][c] + part[1][b][rr][c]) + part[2][b][rr][c]) + part[3][b][rr][c];
      if (OPT && bias) v += bias[d];
      raw[(size_t)r * D + d] = v;
      if (!OPT || tok) tok[(size_t)r * D + d] = from_f32<T>(v + temporal[(size_t)(r % F) * D + d]);
    }
  }
}

// any row count, K_s % 4 == 0: one wave per output feature sweeps the rows (the fallback beyond 128 rows or off K_s % 64 == 0).
// HELD, for ONE source of at most 64 * KMAX = 2048 columns: W[d,:] stays in registers (161 against 198 us at R = 160, K = 768,
// D = 4096, the video-only step at batch 16: profiles/front_refactor.log). Otherwise the weight row is read again for every
// row, any K, one or two sources. Either way a lane's chain is k = 4 * lane + 256 t ascending, source 0 then source 1.
template <typename T, bool HELD, bool OPT>
__global__ __launch_bounds__(256) void proj_fwd_k(ProjSrcs S, const float* __restrict__ bias,
                                                  const float* __restrict__ temporal, float* __restrict__ raw,
                                                  T* __restrict__ tok, int R, int F, int D) {
  const int d = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (d >= D) return;
  const int lane = threadIdx.x & 63;
  constexpr int KMAX = 32;
  const int K0 = S.s[0].k;
  float w[KMAX];
#pragma unroll
  for (int t = 0; t < KMAX / 4; ++t) {
    const int k = t * 256 + lane * 4;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (HELD && k < K0) Vec4<float>::load(S.s[0].w + (size_t)d * S.s[0].ldw + k, v);
    w[4 * t] = v[0]; w[4 * t + 1] = v[1]; w[4 * t + 2] = v[2]; w[4 * t + 3] = v[3];
  }
  for (int r = 0; r < R; ++r) {
    float acc = 0.f;
    if (HELD) {
#pragma unroll
      for (int t = 0; t < KMAX / 4; ++t) {
        const int k = t * 256 + lane * 4;
        if (k < K0) {
          float v[4];
          Vec4<float>::load(S.s[0].x + (size_t)r * S.s[0].ldx + k, v);
          acc += v[0] * w[4 * t] + v[1] * w[4 * t + 1] + v[2] * w[4 * t + 2] + v[3] * w[4 * t + 3];
        }
      }
    } else {
      for (int s = 0; s < S.n; ++s) {
        const float* x = S.s[s].x + (size_t)r * S.s[s].ldx;
        const float* wr = S.s[s].w + (size_t)d * S.s[s].ldw;
        for (int k = lane * 4; k < S.s[s].k; k += 256) {
          float a[4], b[4];
          Vec4<float>::load(x + k, a);
          Vec4<float>::load(wr + k, b);
          acc += a[0] * b[0] + a[1] * b[1] + a[2] * b[2] + a[3] * b[3];
        }
      }
    }
    acc = wave_sum(acc);
    if (lane == 0) {
      if (OPT && bias) acc += bias[d];
      raw[(size_t)r * D + d] = acc;
      if (!OPT || tok) tok[(size_t)r * D + d] = from_f32<T>(acc + temporal[(size_t)(r % F) * D + d]);
    }
  }
}

// dW_s[d,k] += sum_r (g0[r,d] + g1[r,d]) * X_s[r,k] for source blockIdx.y (the weight gradient of llama/model.py:322), dW_s a
// weight gradient or a column range of one with its own row pitch (S.s[].w / ldw). One wave owns DB output features and the
// whole K row of each in registers (DB x K/64 accumulators), so a row of X fetched from L2 feeds DB features (DB x fewer bytes
// through L2 than one feature per wave), RT rows per trip. Per output the fma chain is rows ascending. The gradient rows have
// pitch ldg (fvqa_av_linear_bwd: a column range of a wider matrix); BIAS: dbias[d] += sum_r g[r,d], rows ascending, by the
// waves of source 0 (a compile-time switch: the sums cost the <16, 4, 8> form nine registers).
template <int KMAX, int DB, int RT, bool BIAS>   // RT rows per trip
__global__ __launch_bounds__(256) void proj_bwd_k(const float* __restrict__ g0, const float* __restrict__ g1, ProjSrcs S,
                                                  int R, int D, int ldg, float* __restrict__ dbias) {
  const ProjSrc src = blockIdx.y == 0 ? S.s[0] : S.s[1];
  const float* __restrict__ X = src.x;
  float* __restrict__ dW = const_cast<float*>(src.w);
  const int K = src.k, ldx = src.ldx, ldw = src.ldw;
  const int d0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * DB;
  if (d0 >= D) return;
  const int lane = threadIdx.x & 63;
  float acc[DB][KMAX];
  float bsum[DB];
#pragma unroll
  for (int j = 0; j < DB; ++j) {
    bsum[j] = 0.f;
#pragma unroll
    for (int t = 0; t < KMAX; ++t) acc[j][t] = 0.f;
  }
  for (int r0 = 0; r0 < R; r0 += RT) {                     // RT rows per trip: their loads are all in flight together (round 5: 8, was 4 —
                                                           // the kernel is a chain of R / RT load latencies: 40.6 us at 20 trips)
    float g[RT][DB];
    float v[RT][KMAX];
#pragma unroll
    for (int rr = 0; rr < RT; ++rr) {
      const int r = r0 + rr < R ? r0 + rr : R - 1;
      const float live = r0 + rr < R ? 1.f : 0.f;
#pragma unroll
      for (int j = 0; j < DB; ++j) {
        const int d = d0 + j < D ? d0 + j : D - 1;
        float gv = g0[(size_t)r * ldg + d];
        if (g1) gv += g1[(size_t)r * ldg + d];
        g[rr][j] = gv * live;
      }
#pragma unroll
      for (int t = 0; t < KMAX / 4; ++t) {
        const int k = t * 256 + lane * 4;
        float q[4] = {0.f, 0.f, 0.f, 0.f};
        if (k < K) Vec4<float>::load(X + (size_t)r * ldx + k, q);
        v[rr][4 * t] = q[0]; v[rr][4 * t + 1] = q[1]; v[rr][4 * t + 2] = q[2]; v[rr][4 * t + 3] = q[3];
      }
    }
#pragma unroll
    for (int rr = 0; rr < RT; ++rr)                        // rows in order: the same fma chain as a row-by-row loop
#pragma unroll
      for (int j = 0; j < DB; ++j) {
        if (BIAS) bsum[j] += g[rr][j];
#pragma unroll
        for (int t = 0; t < KMAX; ++t) acc[j][t] += g[rr][j] * v[rr][t];
      }
  }
  if (BIAS && blockIdx.y == 0 && lane == 0) {
#pragma unroll
    for (int j = 0; j < DB; ++j)
      if (d0 + j < D) dbias[d0 + j] += bsum[j];
  }
#pragma unroll
  for (int j = 0; j < DB; ++j) {
    if (d0 + j >= D) break;
#pragma unroll
    for (int t = 0; t < KMAX / 4; ++t) {
      const int k = t * 256 + lane * 4;
      if (k < K) {
        float v[4];
        Vec4<float>::load(dW + (size_t)(d0 + j) * ldw + k, v);
        v[0] += acc[j][4 * t]; v[1] += acc[j][4 * t + 1]; v[2] += acc[j][4 * t + 2]; v[3] += acc[j][4 * t + 3];
        Vec4<float>::store(dW + (size_t)(d0 + j) * ldw + k, v);
      }
    }
  }
}

__global__ __launch_bounds__(256) void temporal_bwd_k(const float* __restrict__ d_tok, float* __restrict__ dtemp,
                                                      int B, int F, int D) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= F * D) return;
  float s = 0.f;
  for (int b = 0; b < B; ++b) s += d_tok[(size_t)b * F * D + idx];
  dtemp[idx] += s;
}

// ---- LM-head cross entropy (reference llama/model.py:349-350) --------------------------------
// one workgroup per (n, s) row with s < S-1 and a non-ignored label; other rows exit at once
// block-wide max / sum for blockDim.x == 1024 (16 waves); `red` is 16 floats of LDS
__device__ __forceinline__ float block_max_1024(float v, float* red) {
  v = wave_max(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float m = red[0];
#pragma unroll
  for (int i = 1; i < 16; ++i) m = fmaxf(m, red[i]);
  return m;
}
__device__ __forceinline__ float block_sum_1024(float v, float* red) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float s = red[0];
#pragma unroll
  for (int i = 1; i < 16; ++i) s += red[i];               // fixed order
  return s;
}

// 1024 threads per row; a row of up to 32768 logits is read ONCE, all of its loads in flight together (round 5: the scored rows are
// a few dozen workgroups, so a row's latency chain — two dependent passes of 31 loads per thread at 256 threads — was the kernel:
// 16.7 us); longer rows take the two-pass loop.
__global__ __launch_bounds__(1024) void ce_fwd_k(const float* __restrict__ logits, const int64_t* __restrict__ labels,
                                                 float* __restrict__ lse, float* __restrict__ rowloss, int S, int V,
                                                 int64_t ignore) {
  __shared__ float red[16];
  const int row = blockIdx.x;
  const int s = row % S;
  int64_t lab = ignore;
  if (s < S - 1) lab = labels[row + 1];
  if (lab == ignore || lab < 0 || lab >= V) {       // block-uniform
    if (threadIdx.x == 0) { rowloss[row] = 0.f; lse[row] = 0.f; }
    return;
  }
  const float* z = logits + (size_t)row * V;
  constexpr int MAXC = 8;
  float m = -INFINITY, sum = 0.f;
  if (V <= 1024 * 4 * MAXC) {
    float v[MAXC][4];
#pragma unroll
    for (int i = 0; i < MAXC; ++i) {
      const int c = (threadIdx.x + 1024 * i) * 4;
      if (c < V) Vec4<float>::load(z + c, v[i]);
      else v[i][0] = v[i][1] = v[i][2] = v[i][3] = -INFINITY;
    }
#pragma unroll
    for (int i = 0; i < MAXC; ++i) m = fmaxf(fmaxf(m, fmaxf(v[i][0], v[i][1])), fmaxf(v[i][2], v[i][3]));
    m = block_max_1024(m, red);
#pragma unroll
    for (int i = 0; i < MAXC; ++i) sum += __expf(v[i][0] - m) + __expf(v[i][1] - m) + __expf(v[i][2] - m) + __expf(v[i][3] - m);
  } else {
    for (int c = threadIdx.x * 4; c < V; c += 4096) {
      float v[4];
      Vec4<float>::load(z + c, v);
      m = fmaxf(fmaxf(m, fmaxf(v[0], v[1])), fmaxf(v[2], v[3]));
    }
    m = block_max_1024(m, red);
    for (int c = threadIdx.x * 4; c < V; c += 4096) {
      float v[4];
      Vec4<float>::load(z + c, v);
      sum += __expf(v[0] - m) + __expf(v[1] - m) + __expf(v[2] - m) + __expf(v[3] - m);
    }
  }
  sum = block_sum_1024(sum, red);
  if (threadIdx.x == 0) {
    const float l = m + logf(sum);
    lse[row] = l;
    rowloss[row] = l - z[lab];
  }
}

// fixed-order sum of row losses and count of scored rows -> loss_sum[0..1]
__global__ __launch_bounds__(256) void loss_reduce_k(const float* __restrict__ rowloss,
                                                     const int64_t* __restrict__ labels, float* __restrict__ out,
                                                     int rows, int S, int64_t ignore, int64_t nclass) {
  __shared__ float red[4];
  float a = 0.f, c = 0.f;
  for (int r = threadIdx.x; r < rows; r += 256) {
    const int s = r % S;
    if (s < S - 1) {
      const int64_t lab = labels[r + 1];
      if (lab != ignore && lab >= 0 && lab < nclass) { a += rowloss[r]; c += 1.f; }
    }
  }
  a = block_sum_256(a, red);
  c = block_sum_256(c, red);
  if (threadIdx.x == 0) { out[0] += a; out[1] += c; }
}

template <typename T>
__global__ __launch_bounds__(1024) void ce_bwd_k(const float* __restrict__ logits, const int64_t* __restrict__ labels,
                                                const float* __restrict__ lse, const float* __restrict__ loss_sum,
                                                const float* __restrict__ gscale, T* __restrict__ dlogits, int S,
                                                int V, int64_t ignore) {
  const int row = blockIdx.x;
  const int s = row % S;
  int64_t lab = ignore;
  if (s < S - 1) lab = labels[row + 1];
  T* dz = dlogits + (size_t)row * V;
  if (lab == ignore || lab < 0 || lab >= V) {
    const float zero[4] = {0.f, 0.f, 0.f, 0.f};
    for (int c = threadIdx.x * 4; c < V; c += 4096) Vec4<T>::store(dz + c, zero);
    return;
  }
  const float* z = logits + (size_t)row * V;
  const float l = lse[row];
  const float k = gscale[0] / loss_sum[1];
  for (int c = threadIdx.x * 4; c < V; c += 4096) {
    float v[4], o[4];
    Vec4<float>::load(z + c, v);
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = (__expf(v[j] - l) - ((int64_t)(c + j) == lab ? 1.f : 0.f)) * k;
    Vec4<T>::store(dz + c, o);
  }
}

// ---- QAV head (reference llama/model.py:359-361) ----------------------------------------------
// one wave per (n, s) row; only rows whose label (at s+1) is a frame index do work
template <typename T, int FMAX>
__global__ __launch_bounds__(256) void qav_fwd_k(const T* __restrict__ xn, const float* __restrict__ vf,
                                                 const int64_t* __restrict__ labels, float* __restrict__ probs,
                                                 float* __restrict__ rowloss, int rows, int S, int D, int F,
                                                 float inv_tau) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int lane = threadIdx.x & 63;
  const int n = row / S, s = row % S;
  int64_t lab = -1;
  if (s < S - 1) lab = labels[row + 1];
  if (lab < 0 || lab >= F) {
    if (lane == 0) rowloss[row] = 0.f;
    return;
  }
  float z[FMAX];
#pragma unroll
  for (int f = 0; f < FMAX; ++f) z[f] = 0.f;
  const T* x = xn + (size_t)row * D;
  for (int c = lane * 4; c < D; c += 256) {
    float xv[4];
    Vec4<T>::load(x + c, xv);
#pragma unroll
    for (int f = 0; f < FMAX; ++f) {
      if (f < F) {
        float v[4];
        Vec4<float>::load(vf + ((size_t)n * F + f) * D + c, v);
        z[f] += xv[0] * v[0] + xv[1] * v[1] + xv[2] * v[2] + xv[3] * v[3];
      }
    }
  }
  float m = -INFINITY;
#pragma unroll
  for (int f = 0; f < FMAX; ++f) {
    z[f] = wave_sum(z[f]) * inv_tau;
    if (f < F) m = fmaxf(m, z[f]);
  }
  float sum = 0.f, zl = 0.f;
#pragma unroll
  for (int f = 0; f < FMAX; ++f)
    if (f < F) {
      sum += expf(z[f] - m);
      if (f == (int)lab) zl = z[f];
    }
  const float l = m + logf(sum);
  if (lane == 0) {
    rowloss[row] = l - zl;
#pragma unroll
    for (int f = 0; f < FMAX; ++f)
      if (f < F) probs[(size_t)row * F + f] = expf(z[f] - l);
  }
}

// dxn[row,:] = sum_f dl[f] * vf[n,f,:]  (zero on unscored rows)
template <typename T, int FMAX>
__global__ __launch_bounds__(256) void qav_bwd_x_k(const float* __restrict__ vf, const int64_t* __restrict__ labels,
                                                   const float* __restrict__ probs,
                                                   const float* __restrict__ loss_sum,
                                                   const float* __restrict__ gscale, T* __restrict__ dxn, int rows,
                                                   int S, int D, int F, float inv_tau) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int lane = threadIdx.x & 63;
  const int n = row / S, s = row % S;
  int64_t lab = -1;
  if (s < S - 1) lab = labels[row + 1];
  T* dx = dxn + (size_t)row * D;
  if (lab < 0 || lab >= F) {
    const float zero[4] = {0.f, 0.f, 0.f, 0.f};
    for (int c = lane * 4; c < D; c += 256) Vec4<T>::store(dx + c, zero);
    return;
  }
  const float k = gscale[0] / loss_sum[1] * inv_tau;
  float dl[FMAX];
#pragma unroll
  for (int f = 0; f < FMAX; ++f) dl[f] = f < F ? (probs[(size_t)row * F + f] - (f == (int)lab ? 1.f : 0.f)) * k : 0.f;
  for (int c = lane * 4; c < D; c += 256) {
    float o[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int f = 0; f < FMAX; ++f)
      if (f < F) {
        float v[4];
        Vec4<float>::load(vf + ((size_t)n * F + f) * D + c, v);
        o[0] += dl[f] * v[0]; o[1] += dl[f] * v[1]; o[2] += dl[f] * v[2]; o[3] += dl[f] * v[3];
      }
    Vec4<T>::store(dx + c, o);
  }
}

// d_raw[n,f,:] += sum_s dl[n,s,f] * xn[n,s,:]   — one workgroup per (n, f)
template <typename T>
__global__ __launch_bounds__(256) void qav_bwd_v_k(const T* __restrict__ xn, const int64_t* __restrict__ labels,
                                                   const float* __restrict__ probs,
                                                   const float* __restrict__ loss_sum,
                                                   const float* __restrict__ gscale, float* __restrict__ d_raw, int S,
                                                   int D, int F, float inv_tau) {
  const int n = blockIdx.x / F, f = blockIdx.x % F;
  const float k = gscale[0] / loss_sum[1] * inv_tau;
  for (int c = threadIdx.x * 4; c < D; c += 1024) {
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int s = 0; s < S - 1; ++s) {
      const int64_t lab = labels[(size_t)n * S + s + 1];
      if (lab < 0 || lab >= F) continue;
      const size_t row = (size_t)n * S + s;
      const float dl = (probs[row * F + f] - (f == (int)lab ? 1.f : 0.f)) * k;
      float xv[4];
      Vec4<T>::load(xn + row * D + c, xv);
      acc[0] += dl * xv[0]; acc[1] += dl * xv[1]; acc[2] += dl * xv[2]; acc[3] += dl * xv[3];
    }
    float o[4];
    float* dst = d_raw + ((size_t)n * F + f) * D + c;
    Vec4<float>::load(dst, o);
    o[0] += acc[0]; o[1] += acc[1]; o[2] += acc[2]; o[3] += acc[3];
    Vec4<float>::store(dst, o);
  }
}


// ---- audio-visual front end: cross-attention (reference llama/model.py:153-169) ---------------------------------------
// X[n,f,:] = softmax_t(Q[n,f,:]·K[n,t,:] * scale) · V[n,:,:] over the T <= 16 keys of the same sample (reference
// llama/model.py:153-169), fp32 throughout, max subtracted. One workgroup per query row; scores are block sums in key order.
__global__ __launch_bounds__(256) void av_cross_attn_fwd_k(const float* __restrict__ q, const float* __restrict__ k,
                                                           const float* __restrict__ v, float* __restrict__ x, int nq,
                                                           int T, int dim, int ldq, int ldk, int ldv, float scale) {
  __shared__ float red[4];
  const int row = blockIdx.x;
  const int n = row / nq;
  const float* qr = q + (size_t)row * ldq;
  float sc[16];
  float m = -INFINITY;
#pragma unroll
  for (int t = 0; t < 16; ++t) {
    sc[t] = -INFINITY;
    if (t < T) {
      const float* kr = k + ((size_t)n * T + t) * ldk;
      float a = 0.f;
      for (int c = threadIdx.x * 4; c < dim; c += 1024) {
        float qa[4], ka[4];
        Vec4<float>::load(qr + c, qa);
        Vec4<float>::load(kr + c, ka);
        a += qa[0] * ka[0] + qa[1] * ka[1] + qa[2] * ka[2] + qa[3] * ka[3];
      }
      sc[t] = block_sum_256(a, red) * scale;
      m = fmaxf(m, sc[t]);
    }
  }
  float sum = 0.f;
#pragma unroll
  for (int t = 0; t < 16; ++t)
    if (t < T) { sc[t] = expf(sc[t] - m); sum += sc[t]; }
  const float inv = 1.f / sum;
  for (int c = threadIdx.x * 4; c < dim; c += 1024) {
    float o[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < 16; ++t)
      if (t < T) {
        float va[4];
        Vec4<float>::load(v + ((size_t)n * T + t) * ldv + c, va);
        const float p = sc[t] * inv;
        o[0] += p * va[0]; o[1] += p * va[1]; o[2] += p * va[2]; o[3] += p * va[3];
      }
    Vec4<float>::store(x + (size_t)row * dim + c, o);
  }
}

// ---- --train_audio: the backward of the audio half of the front end ---------------------------------------------------
// Backward of av_cross_attn_fwd_k, one workgroup per sample: dq, dk, dv (written) from q, k, v and dx; the softmax is recomputed
// with the maximum subtracted, as the forward does. Queries go through LDS in chunks of 16 (any n_query), columns in tiles of
// 1024; a thread owns 4 columns of a tile and keeps dk_t, dv_t of the T <= 16 keys for them in registers.
//   scores / dP: one wave per (f, t) pair, lanes over dim, wave_sum (a fixed shuffle tree)
//   P, dS = P o (dP - sum_t P dP): one thread per query row, t ascending
//   dv_t += P_ft dx_f, dk_t += dS_ft q_f: f ascending; dq_f = scale sum_t dS_ft k_t: t ascending
// With one key P is exactly 1 and dS = 1 * (dP - 1 * dP) exactly 0: dq and dk come out as zeros.
constexpr int CA_QC = 16;
__global__ __launch_bounds__(256) void av_cross_attn_bwd_k(const float* __restrict__ q, const float* __restrict__ k,
                                                           const float* __restrict__ v, const float* __restrict__ dx,
                                                           float* __restrict__ dq, float* __restrict__ dk,
                                                           float* __restrict__ dv, int nq, int T, int dim, int ldq, int ldk,
                                                           int ldv, int lddq, int lddk, int lddv, float scale) {
  __shared__ float sP[CA_QC][16];      // scores, then P
  __shared__ float sD[CA_QC][16];      // dP, then dS
  const int n = blockIdx.x;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const float* kn = k + (size_t)n * T * ldk;
  const float* vn = v + (size_t)n * T * ldv;
  for (int c0 = 0; c0 < dim; c0 += 1024) {
    const int c = c0 + threadIdx.x * 4;
    const bool live = c < dim;
    float adk[16][4], adv[16][4];
#pragma unroll
    for (int t = 0; t < 16; ++t)
#pragma unroll
      for (int e = 0; e < 4; ++e) adk[t][e] = adv[t][e] = 0.f;
    for (int f0 = 0; f0 < nq; f0 += CA_QC) {
      const int nf = nq - f0 < CA_QC ? nq - f0 : CA_QC;
      __syncthreads();                                         // the previous chunk's readers are done with sP / sD
      for (int p = w; p < nf * T; p += 4) {
        const int f = p / T, t = p - f * T;
        const size_t row = (size_t)n * nq + f0 + f;
        const float* qr = q + row * ldq;
        const float* dr = dx + row * dim;
        const float* kr = kn + (size_t)t * ldk;
        const float* vr = vn + (size_t)t * ldv;
        float s = 0.f, d = 0.f;
        for (int cc = lane * 4; cc < dim; cc += 256) {
          float a[4], b[4];
          Vec4<float>::load(qr + cc, a);
          Vec4<float>::load(kr + cc, b);
          s += a[0] * b[0] + a[1] * b[1] + a[2] * b[2] + a[3] * b[3];
          Vec4<float>::load(dr + cc, a);
          Vec4<float>::load(vr + cc, b);
          d += a[0] * b[0] + a[1] * b[1] + a[2] * b[2] + a[3] * b[3];
        }
        s = wave_sum(s) * scale;
        d = wave_sum(d);
        if (lane == 0) { sP[f][t] = s; sD[f][t] = d; }
      }
      __syncthreads();
      if ((int)threadIdx.x < nf) {
        const int f = threadIdx.x;
        float m = -INFINITY;
        for (int t = 0; t < T; ++t) m = fmaxf(m, sP[f][t]);
        float e[16], sum = 0.f;
#pragma unroll
        for (int t = 0; t < 16; ++t)
          if (t < T) { e[t] = expf(sP[f][t] - m); sum += e[t]; }
        const float inv = 1.f / sum;
        float dot = 0.f;
#pragma unroll
        for (int t = 0; t < 16; ++t)
          if (t < T) { e[t] *= inv; dot += e[t] * sD[f][t]; }
#pragma unroll
        for (int t = 0; t < 16; ++t)
          if (t < T) { sD[f][t] = e[t] * (sD[f][t] - dot); sP[f][t] = e[t]; }
      }
      __syncthreads();
      if (live) {
        for (int f = 0; f < nf; ++f) {
          const size_t row = (size_t)n * nq + f0 + f;
          float qa[4], da[4], o[4] = {0.f, 0.f, 0.f, 0.f};
          Vec4<float>::load(q + row * ldq + c, qa);
          Vec4<float>::load(dx + row * dim + c, da);
#pragma unroll
          for (int t = 0; t < 16; ++t)
            if (t < T) {
              const float p = sP[f][t], ds = sD[f][t];
              float ka[4];
              Vec4<float>::load(kn + (size_t)t * ldk + c, ka);
#pragma unroll
              for (int e = 0; e < 4; ++e) {
                adv[t][e] += p * da[e];
                adk[t][e] += ds * qa[e];
                o[e] += ds * ka[e];
              }
            }
#pragma unroll
          for (int e = 0; e < 4; ++e) o[e] *= scale;
          Vec4<float>::store(dq + row * lddq + c, o);
        }
      }
    }
    if (live) {
#pragma unroll
      for (int t = 0; t < 16; ++t)
        if (t < T) {
          float o[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) o[e] = adk[t][e] * scale;
          Vec4<float>::store(dk + ((size_t)n * T + t) * lddk + c, o);
          Vec4<float>::store(dv + ((size_t)n * T + t) * lddv + c, adv[t]);
        }
    }
  }
}

// Input gradient of a projection: dx[r, j] = sum_d (g0[r,d] + g1[r,d]) * W[d, j] on the exact-fp32 matrix cores. One workgroup
// per 16 output columns and 16 rows (grid.y: at 80 rows and k = 768, 240 workgroups; one workgroup per 128 rows took 68 us at
// dim = 4096, this one 29); its 4 waves split the reduction (dim % 64 == 0), the four partials meet in LDS and are added in
// wave order. Per output the fma chain of a wave is d ascending in 16-element strides: fixed, bitwise repeatable.
__global__ __launch_bounds__(256) void av_proj_dx_k(const float* __restrict__ g0, const float* __restrict__ g1,
                                                    const float* __restrict__ W, float* __restrict__ dx, int R, int D, int K,
                                                    int ldg, int ldw, int lddx) {
  __shared__ float part[4][16][17];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int li = lane & 15, g = lane >> 4;
  const int n0 = blockIdx.x * 16;
  const int r0 = blockIdx.y * 16;
  const int dw = D / 4;                                      // this wave's range of the reduction
  int bn = n0 + li; bn = bn < K ? bn : K - 1;
  int ar = r0 + li; ar = ar < R ? ar : R - 1;
  const float* bp = W + (size_t)(w * dw + 4 * g) * ldw + bn;
  const size_t aoff = (size_t)ar * ldg + (size_t)w * dw + 4 * g;
  f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
  constexpr int VU = 8;
  for (int d0 = 0; d0 < dw; d0 += 16 * VU) {                 // every load of a trip in flight before its first MFMA
    float bf[VU][4];
    float4 af[VU];
#pragma unroll
    for (int u = 0; u < VU; ++u) {
      const int d = d0 + 16 * u;
      const bool in = d < dw;
#pragma unroll
      for (int e = 0; e < 4; ++e) bf[u][e] = in ? bp[(size_t)(d + e) * ldw] : 0.f;
      float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
      if (in) {
        a = *reinterpret_cast<const float4*>(g0 + aoff + d);
        if (g1) {
          const float4 a1 = *reinterpret_cast<const float4*>(g1 + aoff + d);
          a.x += a1.x; a.y += a1.y; a.z += a1.z; a.w += a1.w;
        }
      }
      af[u] = a;
    }
#pragma unroll
    for (int u = 0; u < VU; ++u) {
      if (d0 + 16 * u >= dw) break;
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(af[u].x, bf[u][0], acc, 0, 0, 0);     // D[row 4g+e][column li]
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(af[u].y, bf[u][1], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(af[u].z, bf[u][2], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(af[u].w, bf[u][3], acc, 0, 0, 0);
    }
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) part[w][4 * g + e][li] = acc[e];
  __syncthreads();
  const int rr = threadIdx.x >> 4, c = threadIdx.x & 15;
  const int r = r0 + rr, j = n0 + c;
  if (r < R && j < K)
    dx[(size_t)r * lddx + j] = ((part[0][rr][c] + part[1][rr][c]) + part[2][rr][c]) + part[3][rr][c];
}

// host side: the C sources checked and packed for a launch (16-byte rows everywhere: float4 loads)
static int proj_pack(const fvqa_proj_src* src, int n_src, ProjSrcs* out, bool* mfma_ok) {
  if (n_src < 1 || n_src > 2 || !src) return FVQA_EINVAL;
  *mfma_ok = true;
  out->n = n_src;
  for (int s = 0; s < n_src; ++s) {
    if (!src[s].x || !src[s].w) return FVQA_EINVAL;
    if (src[s].k <= 0 || src[s].k % 4 || src[s].ldx < src[s].k || src[s].ldw < src[s].k) return FVQA_ESHAPE;
    if (src[s].ldx % 4 || src[s].ldw % 4 || (((uintptr_t)src[s].x | (uintptr_t)src[s].w) & 15)) return FVQA_EALIGN;
    if (src[s].k % 64) *mfma_ok = false;
    out->s[s] = ProjSrc{src[s].x, src[s].w, src[s].ldx, src[s].ldw, src[s].k};
  }
  if (n_src == 1) out->s[1] = out->s[0];
  return FVQA_OK;
}

// The forward launch of every projection entry. The wave-per-feature kernel re-reads the whole source matrix for every output
// feature (1 GB of L2 traffic at D = 4096: 120 us). Shapes of the step (every K_s % 64 == 0, at most 128 rows) run on the
// exact-fp32 matrix cores instead, temporal embedding and cast included.
template <typename T, bool OPT>
static void proj_fwd_launch_t(const ProjSrcs& S, bool mfma, const float* bias, const float* temporal, float* raw, void* tok,
                              int R, int F, int D, hipStream_t st) {
  const dim3 block(256);
  if (!mfma && S.n == 1 && S.s[0].k <= 2048)
    hipLaunchKernelGGL((proj_fwd_k<T, true, OPT>), dim3((D + 3) / 4), block, 0, st, S, bias, temporal, raw, (T*)tok, R, F, D);
  else if (!mfma)
    hipLaunchKernelGGL((proj_fwd_k<T, false, OPT>), dim3((D + 3) / 4), block, 0, st, S, bias, temporal, raw, (T*)tok, R, F, D);
  else if (S.n == 1)
    hipLaunchKernelGGL((proj_fwd_mfma_k<T, 1, OPT>), dim3((D + 15) / 16), block, 0, st, S, bias, temporal, raw, (T*)tok, R, F, D);
  else
    hipLaunchKernelGGL((proj_fwd_mfma_k<T, 2, OPT>), dim3((D + 15) / 16), block, 0, st, S, bias, temporal, raw, (T*)tok, R, F, D);
}
static void proj_fwd_launch(const ProjSrcs& S, bool mfma_ok, const float* bias, const float* temporal, float* raw, void* tok,
                            int R, int F, int D, int dtype, hipStream_t st) {
  const bool mfma = mfma_ok && R <= 128;
  const bool opt = bias || !tok;                            // OPT = false: no bias, tokens written, nothing asked at run time
  if (dtype == FVQA_H16 && opt) proj_fwd_launch_t<bf16_t, true>(S, mfma, bias, temporal, raw, tok, R, F, D, st);
  else if (dtype == FVQA_H16) proj_fwd_launch_t<bf16_t, false>(S, mfma, bias, temporal, raw, tok, R, F, D, st);
  else if (opt) proj_fwd_launch_t<float, true>(S, mfma, bias, temporal, raw, tok, R, F, D, st);
  else proj_fwd_launch_t<float, false>(S, mfma, bias, temporal, raw, tok, R, F, D, st);
}

// The backward launch of every projection entry (each K_s <= 2048, checked by the entry). Every source <= 1024 columns: one
// launch, the sources on grid.y, 4 features per wave (4 x 16 accumulators), 4 waves per CU at D = 4096; else one <32, 2, 4>
// launch per source. dbias rides on the first source only (blockIdx.y == 0 of the first launch).
template <int KMAX, int DB, int RT>
static void proj_bwd_launch_one(const float* g0, const float* g1, const ProjSrcs& S, int ny, int R, int D, int ldg, float* dbias,
                                hipStream_t st) {
  const dim3 grid((D + 4 * DB - 1) / (4 * DB), ny), block(256);
  if (dbias) hipLaunchKernelGGL((proj_bwd_k<KMAX, DB, RT, true>), grid, block, 0, st, g0, g1, S, R, D, ldg, dbias);
  else hipLaunchKernelGGL((proj_bwd_k<KMAX, DB, RT, false>), grid, block, 0, st, g0, g1, S, R, D, ldg, dbias);
}
static void proj_bwd_launch(const float* g0, const float* g1, const ProjSrcs& S, int R, int D, int ldg, float* dbias,
                            hipStream_t st) {
  bool narrow = true;
  for (int s = 0; s < S.n; ++s) narrow = narrow && S.s[s].k <= 1024;
  if (narrow) {
    proj_bwd_launch_one<16, 4, 8>(g0, g1, S, S.n, R, D, ldg, dbias, st);
    return;
  }
  for (int s = 0; s < S.n; ++s) {
    ProjSrcs one = S;
    one.s[0] = S.s[s];
    one.n = 1;
    proj_bwd_launch_one<32, 2, 4>(g0, g1, one, 1, R, D, ldg, s == 0 ? dbias : nullptr, st);
  }
}

}  // namespace

extern "C" int fvqa_visual_proj_fwd(const float* video, const float* W, const float* temporal, float* vf_raw,
                                    void* vf_tok, int n_frames_total, int max_feats, int in_dim, int dim, int dtype,
                                    void* stream) {
  if (!video || !W || !temporal || !vf_raw || !vf_tok) return FVQA_EINVAL;
  if (!fvqa_dtype_ok(dtype)) return FVQA_EINVAL;
  if (n_frames_total <= 0 || max_feats <= 0 || in_dim <= 0 || in_dim % 4 || in_dim > 2048 || dim <= 0)
    return FVQA_ESHAPE;
  // both kernels read video and W 16 bytes at a time; the outputs and the temporal table are element accesses
  if (!fvqa_aligned(16, video, W) || !fvqa_aligned(4, temporal, vf_raw) || !fvqa_aligned(fvqa_dtype_size(dtype), vf_tok))
    return FVQA_EALIGN;
  const ProjSrc one{video, W, in_dim, in_dim, in_dim};      // one contiguous source, no bias
  proj_fwd_launch(ProjSrcs{{one, one}, 1}, in_dim % 64 == 0, nullptr, temporal, vf_raw, vf_tok, n_frames_total, max_feats, dim,
                  dtype, (hipStream_t)stream);
  FVQA_CHECK_LAUNCH();
  return FVQA_OK;
}

extern "C" int fvqa_visual_proj_bwd(const float* d_tok, const float* d_qav, const float* video, float* dW,
                                    float* dtemporal, int n_frames_total, int max_feats, int in_dim, int dim,
                                    void* stream) {
  if (!d_tok || !video || !dW || !dtemporal) return FVQA_EINVAL;
  if (n_frames_total <= 0 || max_feats <= 0 || n_frames_total % max_feats || in_dim <= 0 || in_dim % 4 ||
      in_dim > 2048 || dim <= 0)
    return FVQA_ESHAPE;
  if (!fvqa_aligned(16, video, dW) || !fvqa_aligned(4, d_tok, d_qav, dtemporal)) return FVQA_EALIGN;
  hipStream_t st = (hipStream_t)stream;
  const ProjSrc one{video, dW, in_dim, in_dim, in_dim};     // one contiguous source, gradient pitch = dim, no dbias
  proj_bwd_launch(d_tok, d_qav, ProjSrcs{{one, one}, 1}, n_frames_total, dim, dim, nullptr, st);
  hipLaunchKernelGGL(temporal_bwd_k, dim3((max_feats * dim + 255) / 256), dim3(256), 0, st, d_tok, dtemporal,
                     n_frames_total / max_feats, max_feats, dim);
  FVQA_CHECK_LAUNCH();
  return FVQA_OK;
}

extern "C" int fvqa_av_proj_fwd(const fvqa_proj_src* src, int n_src, const float* bias, const float* temporal,
                                float* out_raw, void* out_tok, int rows, int max_feats, int dim, int dtype, void* stream) {
  if (!out_raw || (temporal != nullptr) != (out_tok != nullptr)) return FVQA_EINVAL;
  if (!fvqa_dtype_ok(dtype)) return FVQA_EINVAL;
  if (rows <= 0 || dim <= 0 || (temporal && max_feats <= 0)) return FVQA_ESHAPE;
  ProjSrcs S;
  bool mfma_ok;
  if (int rc = proj_pack(src, n_src, &S, &mfma_ok)) return rc;
  proj_fwd_launch(S, mfma_ok, bias, temporal, out_raw, out_tok, rows, max_feats > 0 ? max_feats : 1, dim, dtype,
                  (hipStream_t)stream);
  FVQA_CHECK_LAUNCH();
  return FVQA_OK;
}

extern "C" int fvqa_av_cross_attn_fwd(const float* q, const float* k, const float* v, float* x, int n_samples, int n_query,
                                      int n_key, int dim, int ldq, int ldk, int ldv, float scale, void* stream) {
  if (!q || !k || !v || !x) return FVQA_EINVAL;
  if (n_samples <= 0 || n_query <= 0 || n_key <= 0 || n_key > 16 || dim <= 0 || dim % 4 || ldq < dim || ldk < dim || ldv < dim)
    return FVQA_ESHAPE;
  if (ldq % 4 || ldk % 4 || ldv % 4 || (((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)x) & 15)) return FVQA_EALIGN;
  hipLaunchKernelGGL(av_cross_attn_fwd_k, dim3(n_samples * n_query), dim3(256), 0, (hipStream_t)stream, q, k, v, x, n_query,
                     n_key, dim, ldq, ldk, ldv, scale);
  FVQA_CHECK_LAUNCH();
  return FVQA_OK;
}

extern "C" int fvqa_av_proj_bwd(const float* d_tok, const float* d_qav, const fvqa_proj_src* src, int n_src, float* dtemporal,
                                int rows, int max_feats, int dim, void* stream) {
  if (!d_tok || !dtemporal) return FVQA_EINVAL;
  if (rows <= 0 || max_feats <= 0 || rows % max_feats || dim <= 0) return FVQA_ESHAPE;
  hipStream_t st = (hipStream_t)stream;
  if (n_src) {                                              // (audio_only has no trainable projection: the temporal sum alone)
    ProjSrcs S;
    bool mfma_ok;
    if (int rc = proj_pack(src, n_src, &S, &mfma_ok)) return rc;
    for (int s = 0; s < n_src; ++s)
      if (src[s].k > 2048) return FVQA_ESHAPE;
    proj_bwd_launch(d_tok, d_qav, S, rows, dim, dim, nullptr, st);
  }
  hipLaunchKernelGGL(temporal_bwd_k, dim3((max_feats * dim + 255) / 256), dim3(256), 0, st, d_tok, dtemporal,
                     rows / max_feats, max_feats, dim);
  FVQA_CHECK_LAUNCH();
  return FVQA_OK;
}

extern "C" int fvqa_av_cross_attn_bwd(const float* q, const float* k, const float* v, const float* dx, float* dq, float* dk,
                                      float* dv, int n_samples, int n_query, int n_key, int dim, int ldq, int ldk, int ldv,
                                      int lddq, int lddk, int lddv, float scale, void* stream) {
  if (!q || !k || !v || !dx || !dq || !dk || !dv) return FVQA_EINVAL;
  if (n_samples <= 0 || n_query <= 0 || n_key <= 0 || n_key > 16 || dim <= 0 || dim % 4 || ldq < dim || ldk < dim ||
      ldv < dim || lddq < dim || lddk < dim || lddv < dim)
    return FVQA_ESHAPE;
  if (ldq % 4 || ldk % 4 || ldv % 4 || lddq % 4 || lddk % 4 || lddv % 4 ||
      (((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)dx | (uintptr_t)dq | (uintptr_t)dk | (uintptr_t)dv) & 15))
    return FVQA_EALIGN;
  hipLaunchKernelGGL(av_cross_attn_bwd_k, dim3(n_samples), dim3(256), 0, (hipStream_t)stream, q, k, v, dx, dq, dk, dv,
                     n_query, n_key, dim, ldq, ldk, ldv, lddq, lddk, lddv, scale);
  FVQA_CHECK_LAUNCH();
  return FVQA_OK;
}

extern "C" int fvqa_av_proj_dx(const float* g0, const float* g1, const float* w, float* dx, int rows, int dim, int k,
                               int ldg, int ldw, int lddx, void* stream) {
  if (!g0 || !w || !dx) return FVQA_EINVAL;
  if (rows <= 0 || dim <= 0 || dim % 64 || k <= 0 || k % 4 || ldg < dim || ldw < k || lddx < k) return FVQA_ESHAPE;
  if (ldg % 4 || ldw % 4 || lddx % 4 || (((uintptr_t)g0 | (uintptr_t)g1 | (uintptr_t)w | (uintptr_t)dx) & 15))
    return FVQA_EALIGN;
  hipLaunchKernelGGL(av_proj_dx_k, dim3((k + 15) / 16, (rows + 15) / 16), dim3(256), 0, (hipStream_t)stream, g0, g1, w, dx,
                     rows, dim, k, ldg, ldw, lddx);
  FVQA_CHECK_LAUNCH();
  return FVQA_OK;
}

extern "C" int fvqa_av_linear_bwd(const float* g, int ldg, const fvqa_proj_src* src, int n_src, float* dbias, int rows,
                                  int dim, void* stream) {
  if (!g) return FVQA_EINVAL;
  if (rows <= 0 || dim <= 0 || ldg < dim) return FVQA_ESHAPE;
  // (no condition on ldg: proj_bwd_k reads g and dbias element by element — fvqa_av_proj_bwd runs it at ldg = dim, any dim)
  if ((((uintptr_t)g | (uintptr_t)dbias) & 15)) return FVQA_EALIGN;
  ProjSrcs S;
  bool mfma_ok;
  if (int rc = proj_pack(src, n_src, &S, &mfma_ok)) return rc;
  for (int s = 0; s < n_src; ++s)
    if (src[s].k > 2048) return FVQA_ESHAPE;
  proj_bwd_launch(g, nullptr, S, rows, dim, ldg, dbias, (hipStream_t)stream);
  FVQA_CHECK_LAUNCH();
  return FVQA_OK;
}

extern "C" int fvqa_ce_fwd(const float* logits, const int64_t* labels, float* lse, float* rowloss, float* loss_sum,
                           int n_seq, int seq_len, int vocab, int64_t ignore_index, void* stream) {
  if (!logits || !labels || !lse || !rowloss || !loss_sum) return FVQA_EINVAL;
  if (n_seq <= 0 || seq_len < 2 || vocab <= 0 || vocab % 4) return FVQA_ESHAPE;
  if (!fvqa_aligned(16, logits) || !fvqa_aligned(8, labels) || !fvqa_aligned(4, lse, rowloss, loss_sum)) return FVQA_EALIGN;
  hipStream_t st = (hipStream_t)stream;
  const int rows = n_seq * seq_len;
  hipLaunchKernelGGL(ce_fwd_k, dim3(rows), dim3(1024), 0, st, logits, labels, lse, rowloss, seq_len, vocab,
                     ignore_index);
  hipLaunchKernelGGL(loss_reduce_k, dim3(1), dim3(256), 0, st, rowloss, labels, loss_sum, rows, seq_len,
                     ignore_index, (int64_t)vocab);
  FVQA_CHECK_LAUNCH();
  return FVQA_OK;
}

extern "C" int fvqa_ce_bwd(const float* logits, const int64_t* labels, const float* lse, const float* loss_sum,
                           const float* gscale, void* dlogits, int n_seq, int seq_len, int vocab,
                           int64_t ignore_index, int dtype, void* stream) {
  if (!logits || !labels || !lse || !loss_sum || !gscale || !dlogits) return FVQA_EINVAL;
  if (!fvqa_dtype_ok(dtype)) return FVQA_EINVAL;
  if (n_seq <= 0 || seq_len < 2 || vocab <= 0 || vocab % 4) return FVQA_ESHAPE;
  if (!fvqa_aligned(16, logits) || !fvqa_aligned(fvqa_vec4_bytes(dtype), dlogits) || !fvqa_aligned(8, labels) ||
      !fvqa_aligned(4, lse, loss_sum, gscale))
    return FVQA_EALIGN;
  hipStream_t st = (hipStream_t)stream;
  const int rows = n_seq * seq_len;
  if (dtype == FVQA_H16)
    hipLaunchKernelGGL(ce_bwd_k<bf16_t>, dim3(rows), dim3(1024), 0, st, logits, labels, lse, loss_sum, gscale,
                       (bf16_t*)dlogits, seq_len, vocab, ignore_index);
  else
    hipLaunchKernelGGL(ce_bwd_k<float>, dim3(rows), dim3(1024), 0, st, logits, labels, lse, loss_sum, gscale,
                       (float*)dlogits, seq_len, vocab, ignore_index);
  FVQA_CHECK_LAUNCH();
  return FVQA_OK;
}

extern "C" int fvqa_qav_head_fwd(const void* xn, const float* vf_raw, const int64_t* labels, float* probs,
                                 float* rowloss, float* loss_sum, int n_seq, int seq_len, int dim, int max_feats,
                                 float tau, int dtype, void* stream) {
  if (!xn || !vf_raw || !labels || !probs || !rowloss || !loss_sum) return FVQA_EINVAL;
  if (!fvqa_dtype_ok(dtype)) return FVQA_EINVAL;
  if (n_seq <= 0 || seq_len < 2 || dim <= 0 || dim % 4 || max_feats <= 0 || max_feats > 16 || tau == 0.f)
    return FVQA_ESHAPE;
  if (!fvqa_aligned(fvqa_vec4_bytes(dtype), xn) || !fvqa_aligned(16, vf_raw) || !fvqa_aligned(8, labels) ||
      !fvqa_aligned(4, probs, rowloss, loss_sum))
    return FVQA_EALIGN;
  hipStream_t st = (hipStream_t)stream;
  const int rows = n_seq * seq_len;
  dim3 grid((rows + 3) / 4), block(256);
  if (dtype == FVQA_H16)
    hipLaunchKernelGGL((qav_fwd_k<bf16_t, 16>), grid, block, 0, st, (const bf16_t*)xn, vf_raw, labels, probs, rowloss,
                       rows, seq_len, dim, max_feats, 1.f / tau);
  else
    hipLaunchKernelGGL((qav_fwd_k<float, 16>), grid, block, 0, st, (const float*)xn, vf_raw, labels, probs, rowloss,
                       rows, seq_len, dim, max_feats, 1.f / tau);
  hipLaunchKernelGGL(loss_reduce_k, dim3(1), dim3(256), 0, st, rowloss, labels, loss_sum, rows, seq_len,
                     (int64_t)-1, (int64_t)max_feats);
  FVQA_CHECK_LAUNCH();
  return FVQA_OK;
}

extern "C" int fvqa_qav_head_bwd(const void* xn, const float* vf_raw, const int64_t* labels, const float* probs,
                                 const float* loss_sum, const float* gscale, void* dxn, float* d_raw, int n_seq,
                                 int seq_len, int dim, int max_feats, float tau, int dtype, void* stream) {
  if (!xn || !vf_raw || !labels || !probs || !loss_sum || !gscale || !dxn || !d_raw) return FVQA_EINVAL;
  if (!fvqa_dtype_ok(dtype)) return FVQA_EINVAL;
  if (n_seq <= 0 || seq_len < 2 || dim <= 0 || dim % 4 || max_feats <= 0 || max_feats > 16 || tau == 0.f)
    return FVQA_ESHAPE;
  if (!fvqa_aligned(fvqa_vec4_bytes(dtype), xn, dxn) || !fvqa_aligned(16, vf_raw, d_raw) || !fvqa_aligned(8, labels) ||
      !fvqa_aligned(4, probs, loss_sum, gscale))
    return FVQA_EALIGN;
  hipStream_t st = (hipStream_t)stream;
  const int rows = n_seq * seq_len;
  dim3 grid((rows + 3) / 4), block(256);
  if (dtype == FVQA_H16) {
    hipLaunchKernelGGL((qav_bwd_x_k<bf16_t, 16>), grid, block, 0, st, vf_raw, labels, probs, loss_sum, gscale,
                       (bf16_t*)dxn, rows, seq_len, dim, max_feats, 1.f / tau);
    hipLaunchKernelGGL(qav_bwd_v_k<bf16_t>, dim3(n_seq * max_feats), block, 0, st, (const bf16_t*)xn, labels, probs,
                       loss_sum, gscale, d_raw, seq_len, dim, max_feats, 1.f / tau);
  } else {
    hipLaunchKernelGGL((qav_bwd_x_k<float, 16>), grid, block, 0, st, vf_raw, labels, probs, loss_sum, gscale,
                       (float*)dxn, rows, seq_len, dim, max_feats, 1.f / tau);
    hipLaunchKernelGGL(qav_bwd_v_k<float>, dim3(n_seq * max_feats), block, 0, st, (const float*)xn, labels, probs,
                       loss_sum, gscale, d_raw, seq_len, dim, max_feats, 1.f / tau);
  }
  FVQA_CHECK_LAUNCH();
  return FVQA_OK;
}
