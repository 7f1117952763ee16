// fvqa_slot_seat — in-flight batching (fvqa/stream.py): a prefilled prompt takes a freed slot of the decode batch, one launch per
// admission, one 256-thread workgroup per admitted slot. Entry j copies row src[j] of the prefill — its id row, where its answer
// starts, where its frames start, the logits row its first token is picked from — into slot slot[j] of the per-slot state, names
// request[j] as the slot's tenant and lowers its `done` flag. The k / v rows of the prompt travel by fvqa_kv_beam_move; rows of the
// previous tenant behind the newcomer's prefix stay in the cache, where fvqa_attn_decode writes position pos before it reads it
// and reads nothing behind it.
//
// A slot index outside [0, n_slots), a source row outside [0, n_src) and a slot that still holds a running request (done == 0 and
// req >= 0) are refused: nothing of the entry is written and bit 0 of the caller's error word is raised. The occupancy test reads
// the slot's own words only and every entry names another slot (the host wrapper refuses duplicates), so no workgroup reads what
// another writes.
//
// The logits row moves in 16-byte words when both matrices lie on 16-byte boundaries and a row is a whole number of them
// (V % 4 == 0: then every row of both is aligned), else in 4-byte words — V = 509 rows are 2036 bytes.
#include "common.h"

namespace {

constexpr int NT = 256;

__global__ __launch_bounds__(NT) void slot_seat_k(const int32_t* __restrict__ slot_p, const int32_t* __restrict__ src_p,
                                                  const int32_t* __restrict__ request_p, const int64_t* __restrict__ prompt_ids,
                                                  const int64_t* __restrict__ prefix_p, const int32_t* __restrict__ vstart_src,
                                                  const float* __restrict__ logits_src, const int32_t* __restrict__ root,
                                                  int64_t* __restrict__ ids, int32_t* __restrict__ pos,
                                                  int64_t* __restrict__ pos64, int32_t* __restrict__ done,
                                                  int32_t* __restrict__ gen_start, int32_t* __restrict__ vstart,
                                                  int32_t* __restrict__ req, int32_t* __restrict__ node, float* __restrict__ lg,
                                                  unsigned* __restrict__ err, int n_src, int n_slots, int S, int V, int vec16) {
  const int j = blockIdx.x, tid = threadIdx.x;
  const int s = slot_p[j], m = src_p[j];
  bool refuse = s < 0 || s >= n_slots || m < 0 || m >= n_src;
  if (!refuse) refuse = done[s] == 0 && req[s] >= 0;               // the slot still holds a running request
  __syncthreads();                                                 // (every read of done / req above is over)
  if (refuse) {
    if (tid == 0) err[0] = err[0] | 1u;
    return;
  }
  const int64_t pf = prefix_p[m];
  const bool room = pf >= 1 && pf <= (int64_t)S;                   // else: done at once, zero tokens
  const int64_t* ids_src = prompt_ids + (size_t)m * S;
  int64_t* ids_dst = ids + (size_t)s * S;
  for (int i = tid; i < S; i += NT) ids_dst[i] = ids_src[i];
  if (room) {
    const float* l_src = logits_src + ((size_t)m * S + (size_t)(pf - 1)) * V;
    float* l_dst = lg + (size_t)s * V;
    if (vec16) {
      const uint4* s4 = reinterpret_cast<const uint4*>(l_src);
      uint4* d4 = reinterpret_cast<uint4*>(l_dst);
      for (int i = tid; i < V / 4; i += NT) d4[i] = s4[i];
    } else {
      for (int i = tid; i < V; i += NT) l_dst[i] = l_src[i];
    }
  }
  if (tid == 0) {
    const int at = room ? (int)(pf - 1) : 0;
    pos[s] = at;
    pos64[s] = at;
    gen_start[s] = room ? (int)pf : 0;
    vstart[s] = vstart_src[m];
    req[s] = request_p[j];
    if (node) node[s] = root[m];
    done[s] = room ? 0 : 1;
  }
}

}  // namespace

extern "C" int fvqa_slot_seat(const int32_t* slot, const int32_t* src, const int32_t* request, int n_admit,
                              const int64_t* prompt_ids, const int64_t* prefix, const int32_t* vstart_src,
                              const float* logits_src, const int32_t* root, int n_src, int64_t* ids, int32_t* pos, int64_t* pos64,
                              int32_t* done, int32_t* gen_start, int32_t* vstart, int32_t* req, int32_t* node, float* lg,
                              uint32_t* err, int n_slots, int seq_len, int vocab, void* stream) {
  if (!slot || !src || !request || !prompt_ids || !prefix || !vstart_src || !logits_src || !ids || !pos || !pos64 || !done ||
      !gen_start || !vstart || !req || !lg || !err)
    return FVQA_EINVAL;
  if ((root == nullptr) != (node == nullptr)) return FVQA_EINVAL;  // the trie roots and the slots' nodes come together
  if (n_admit <= 0 || n_src <= 0 || n_slots <= 0 || seq_len <= 0 || vocab <= 0) return FVQA_ESHAPE;
  if (n_admit > n_slots || n_slots > 65535) return FVQA_ESHAPE;
  if (!fvqa_aligned(4, slot, src, request, vstart_src, logits_src, root, pos, done, gen_start, vstart, req, node, lg, err) ||
      !fvqa_aligned(8, prompt_ids, prefix, ids, pos64))
    return FVQA_EALIGN;
  const int vec16 = vocab % 4 == 0 && fvqa_aligned(16, logits_src, lg);
  hipLaunchKernelGGL(slot_seat_k, dim3(n_admit), dim3(NT), 0, (hipStream_t)stream, slot, src, request, prompt_ids, prefix,
                     vstart_src, logits_src, root, ids, pos, pos64, done, gen_start, vstart, req, node, lg, err, n_src, n_slots,
                     seq_len, vocab, vec16);
  FVQA_CHECK_LAUNCH();
  return FVQA_OK;
}
