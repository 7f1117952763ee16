// fvqa_sample_vote — self-consistency over the n samples of a prompt (generate(num_return_sequences=n, vote=True)): the samples
// whose token rows are equal in every column form a group, the largest group wins. One launch per call, behind the token loop;
// one 256-thread workgroup per prompt. include/fvqa.h states the rule.
//   group    thread a < n compares its row with the rows 0 .. a in order, all `steps` columns (padding included): the first equal
//            one is its group's representative — itself if none in front of it is. At most 64 * 64 * steps int32 compares.
//   votes    the representative counts the samples that name it; every other sample holds 0.
//   winner   one thread walks the representatives in index order: more votes win, then the larger score (a NaN counts as -inf),
//            then — nothing replaces on a full tie — the lower index.
// Integer compares and one float compare, a fixed order, no atomics: two launches give the same bits.
#include "common.h"

namespace {

constexpr int VOTE_SAMPLES_MAX = 64;

__global__ __launch_bounds__(256) void sample_vote_k(const int32_t* __restrict__ tokens, const float* __restrict__ score,
                                                     int32_t* __restrict__ group, int32_t* __restrict__ votes,
                                                     int32_t* __restrict__ winner, int32_t* __restrict__ n_groups,
                                                     float* __restrict__ share, int n, int steps) {
  __shared__ int grp[VOTE_SAMPLES_MAX], cnt[VOTE_SAMPLES_MAX];
  const int b = blockIdx.x, a = threadIdx.x;
  const int32_t* tk = tokens + (size_t)b * n * steps;
  if (a < n) {
    const int32_t* mine = tk + (size_t)a * steps;
    int g = a;
    for (int j = 0; j < a; ++j) {
      const int32_t* other = tk + (size_t)j * steps;
      bool eq = true;
      for (int c = 0; c < steps && eq; ++c) eq = mine[c] == other[c];
      if (eq) { g = j; break; }
    }
    grp[a] = g;
  }
  __syncthreads();
  if (a < n) {
    int c = 0;
    if (grp[a] == a)
      for (int j = a; j < n; ++j) c += grp[j] == a ? 1 : 0;
    cnt[a] = c;
    group[(size_t)b * n + a] = grp[a];
    votes[(size_t)b * n + a] = c;
  }
  __syncthreads();
  if (a == 0) {
    int best = 0, ng = 0;                                          // (sample 0 is always a representative)
    float best_s = -INFINITY;
    for (int j = 0; j < n; ++j) {
      if (cnt[j] == 0) continue;
      ng += 1;
      float s = score[(size_t)b * n + j];
      if (s != s) s = -INFINITY;
      if (j == 0 || cnt[j] > cnt[best] || (cnt[j] == cnt[best] && s > best_s)) { best = j; best_s = s; }
    }
    winner[b] = best;
    n_groups[b] = ng;
    share[b] = (float)cnt[best] / (float)n;
  }
}

}  // namespace

extern "C" int fvqa_sample_vote(const int32_t* tokens, const float* score, int32_t* group, int32_t* votes, int32_t* winner,
                                int32_t* n_groups, float* share, int n_seq, int n_samples, int steps, void* stream) {
  if (!tokens || !score || !group || !votes || !winner || !n_groups || !share) return FVQA_EINVAL;
  if (n_seq <= 0 || n_seq > 65535 || n_samples < 1 || n_samples > VOTE_SAMPLES_MAX || steps < 1) return FVQA_ESHAPE;
  if ((long long)n_seq * n_samples * steps > 0x7fffffffLL) return FVQA_ESHAPE;
  if (!fvqa_aligned(4, tokens, score, group, votes, winner, n_groups, share)) return FVQA_EALIGN;
  hipLaunchKernelGGL(sample_vote_k, dim3(n_seq), dim3(256), 0, (hipStream_t)stream, tokens, score, group, votes, winner, n_groups,
                     share, n_samples, steps);
  FVQA_CHECK_LAUNCH();
  return FVQA_OK;
}
