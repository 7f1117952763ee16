// Option scoring by all three flipped tasks (fvqa/flipped.py): the answer options of a sample are ranked by the VQA loss, by the
// VAQ loss (the question predicted from the clip and each candidate answer) and by the QAV loss (the frame order predicted from
// the question and each candidate answer). A VAQ option differs at its answer and the scored question follows it, a QAV option
// has its frame slots behind the answer: the suffix rows of these streams are many more than fvqa_attn_suffix's 16, and they are
// not all token embeddings. Their attention is fvqa_attn_suffix_wide (csrc/score.hip, with the other suffix attentions); two
// kernels here serve the rest:
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
