// The store of a raw key / value row into the KV cache, as the kernels that append behind a pass do it (csrc/score.hip: the APPEND
// instantiation of attn_suffix_k; csrc/treespec.hip: kv_tree_commit_k). One text, so that both store the bits fvqa_attn_decode
// stores for the same raw row and position.
#pragma once
#include "common.h"

namespace {

// RoPE of one pair (a, b) of a key that goes into the cache, operation by operation what fvqa_attn_decode's store of the new
// token's key evaluates (csrc/attn_decode_body.h: `a * c - b * s`, `a * s + b * c`, as hipcc contracts them there: the second
// always into one fma on the rounded a * s; the first into an fma on the rounded b * s in the 16-bit kernels and not at all in
// the fp32 kernel). Spelled out with contraction off so that an appended row has the bits the one-row kernel stores for the same
// raw row and position — in fp32 the last bit shows; tests/test_lookahead_gpu.py and tests/test_treedraft_gpu.py compare them.
template <typename T> __device__ __forceinline__ void rope_pair_as_decode(float a, float b, float c, float s, float& ra, float& rb) {
#pragma clang fp contract(off)
  const float bs = b * s, as = a * s;
  if constexpr (sizeof(T) == 4) ra = a * c - bs;
  else ra = __builtin_fmaf(a, c, -bs);
  rb = __builtin_fmaf(b, c, as);
}

// N consecutive elements of a row (whole 16-byte words on 16-byte boundaries), bit for bit
template <int N, typename T> __device__ __forceinline__ void copy_bits(T* dst, const T* src) {
  static_assert(N * sizeof(T) % 16 == 0, "whole 16-byte words");
#pragma unroll
  for (int u = 0; u < (int)(N * sizeof(T) / 16); ++u) reinterpret_cast<uint4*>(dst)[u] = reinterpret_cast<const uint4*>(src)[u];
}

}  // namespace
