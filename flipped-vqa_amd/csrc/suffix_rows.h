// Device code the suffix-row attention kernels share (csrc/score.hip fvqa_attn_suffix*, csrc/flipped.hip fvqa_attn_suffix_wide):
// the tile geometry, 16 head dims of a row in and out of registers, RoPE of those 16 at a position, the half-wave reductions of
// the online softmax. Included inside the kernels' anonymous namespace, after attn_decode_body.h.
#pragma once

constexpr int QT = 32;                   // queries per tile
constexpr int KC = 32;                   // keys per chunk
constexpr int KLD = DH + 4;              // LDS row stride of q / k (floats): 16-byte rows, lanes of a key column on distinct banks

// 16 consecutive head dims [d0, d0 + 16) of a row as floats
template <typename T> __device__ __forceinline__ void load16(const T* p, float (&v)[16]);
template <> __device__ __forceinline__ void load16<bf16_t>(const bf16_t* p, float (&v)[16]) {
  float a[8], b[8];
  Chunk<bf16_t>::load(p, a);
  Chunk<bf16_t>::load(p + 8, b);
#pragma unroll
  for (int e = 0; e < 8; ++e) { v[e] = a[e]; v[8 + e] = b[e]; }
}
template <> __device__ __forceinline__ void load16<float>(const float* p, float (&v)[16]) {
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    float a[4];
    Chunk<float>::load(p + 4 * u, a);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[4 * u + e] = a[e];
  }
}

// rotate 16 head dims starting at d0 (a multiple of 16) of a row at position p, rounded to the storage type
template <typename T>
__device__ __forceinline__ void rope16(float (&v)[16], const float* cs, const float* sn, int p, int d0) {
  const float4* cp = reinterpret_cast<const float4*>(cs + (size_t)p * HP + d0 / 2);
  const float4* sp = reinterpret_cast<const float4*>(sn + (size_t)p * HP + d0 / 2);
  const float4 c0 = cp[0], c1 = cp[1], s0 = sp[0], s1 = sp[1];
  const float c[8] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w};
  const float s[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float a = v[2 * e], b = v[2 * e + 1];
    v[2 * e] = round_to<T>(a * c[e] - b * s[e]);
    v[2 * e + 1] = round_to<T>(a * s[e] + b * c[e]);
  }
}

__device__ __forceinline__ void store16(float* dst, const float (&v)[16]) {
#pragma unroll
  for (int u = 0; u < 4; ++u)
    *reinterpret_cast<float4*>(dst + 4 * u) = make_float4(v[4 * u], v[4 * u + 1], v[4 * u + 2], v[4 * u + 3]);
}

__device__ __forceinline__ float half_max(float v) {       // over the 32 lanes of an aligned half wave
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ float half_sum(float v) {
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
