// Tree-shaped draft verification (fvqa/generate.py: generate(lookahead=R, draft_answers=C)): the likely answers of a sample are a
// trie whose internal nodes, in pre-order, are the sample's PLAN (fvqa/vocab.py _plan_one); a pass feeds a pre-order prefix of the
// subtree under the row's node through the layers (fvqa_attn_suffix_tree: a row sees the cache and its ancestors), and the two
// entries here do what lies between two such passes (include/fvqa.h states both rules):
//
// fvqa_tree_spec_step — one launch where fvqa_spec_step sits, one 256-thread workgroup per sequence.
//   walk     from local row 0: the largest logit of the row (csrc/token_step.h row_verify, with fvqa_spec_step: lowest index on
//            exact ties, the lse for the log-probability fused) is committed whatever the trie says; the child of the row's plan
//            node under that token is looked for by the whole workgroup (rows r of the node's subtree with parent[r] == node and
//            token[r] == g: on a sound plan the one the end chain G + 1, end[G + 1], ... reaches; the lowest r on a broken one),
//            and the walk goes on at the child's row if this pass fed it. A row's logits are scanned only if the walk reaches it.
//   cut      the next pass is the plan rows [node, e): a prefix of the node's subtree, cut by the rows of a pass, by the depth a
//            tile's ancestor chain may have, by the budget and by the end of the sequence. A prefix of a pre-order range is closed
//            under ancestors, so it is a tree again.
//   outputs  the next pass's rows and the tree attention's operands (local depth / end, the chain of each tile's first row over
//            `parent`), the path of local rows the walk took (what fvqa_kv_tree_commit appends), tokens, log-probabilities and the
//            two counts across workgroups (running rows; running rows still on their trie) through two ticket words.
// fvqa_kv_tree_commit — the cache append of the accepted path: ONE launch over all layers copies the k | v of the stashed raw rows
//   path[n, i] to cache row start_old[n] + i, k in the cache's convention (csrc/cache_row.h: the store fvqa_attn_suffix_append
//   does, so the bits are its bits).
// fvqa_tree_spec_step_sample — the step kernel with SAMPLE = true (false in fvqa_tree_spec_step, whose instantiation holds none
//   of the sampling code): every commit of the walk is csrc/row_sample.h's sampled pick (the one fvqa_decode_next_ex runs) with
//   the draw of its token index, and the walk moves
//   to the child under the sampled token (csrc/spec.hip says why that gives the plain sampled call's ids).
// No float atomics, fixed summation orders: two launches give the same bits. Every index read from the plan, node, ids or path is
// clamped or skipped before it is used.
#include "cache_row.h"
#include "row_sample.h"
#include "token_step.h"

namespace {

constexpr int RMAX = 64;                 // rows of a sequence per pass (two tiles of fvqa_attn_suffix_tree)
constexpr int WALK = 32;                 // tokens one step commits at the most: the relative depths 0 .. 31 of a pass
constexpr int TILE = 32;                 // rows per tile of the tree attention (csrc/score.hip QT)
constexpr int DREL = FVQA_TREE_DEPTH_MAX;
constexpr int NONE = 0x7fffffff;

template <typename T, bool SAMPLE>
__global__ __launch_bounds__(NT) void tree_spec_step_k(
    const float* __restrict__ logits, const T* __restrict__ emb, const int32_t* __restrict__ plan_n,
    const int32_t* __restrict__ plan_token, const int32_t* __restrict__ plan_depth, const int32_t* __restrict__ plan_end,
    const int32_t* __restrict__ plan_parent, int plan_rows, int plan_stride, int eos_id, int stop_at_eos, int max_new,
    int64_t* __restrict__ ids, int32_t* __restrict__ pos, int32_t* __restrict__ done, int32_t* __restrict__ n_generated,
    int32_t* __restrict__ node_p, int32_t* __restrict__ len_p, int32_t* __restrict__ start_p, T* __restrict__ x_next,
    int32_t* __restrict__ depth_o, int32_t* __restrict__ end_o, int32_t* __restrict__ anc_o, int32_t* __restrict__ path_o,
    int32_t* __restrict__ n_path, int32_t* __restrict__ start_old, int32_t* __restrict__ token_out,
    float* __restrict__ logprob_out, int32_t* __restrict__ n_committed, int32_t* __restrict__ n_drafted,
    int32_t* __restrict__ n_active, int32_t* __restrict__ n_on_trie, unsigned* __restrict__ counter,
    int64_t* __restrict__ pos64, int B, int Rin, int Rout, int V, int D, int S, int vec16, SampleArgs sa) {
  extern __shared__ __attribute__((aligned(16))) float erow[];     // SAMPLE: the row's e_i (row_in_lds), then the bitmap
  __shared__ float redf[4];
  __shared__ int redi[4];
  __shared__ float wtotf[4];             // (SAMPLE: the scans of the walk)
  __shared__ int wtoti[4];
  __shared__ int cm[WALK];               // the tokens committed by this step, in order
  __shared__ int wn[RMAX];               // the input tokens of the next pass's rows
  const int b = blockIdx.x, tid = threadIdx.x;
  int64_t* row_ids = ids + (size_t)b * S;
  const size_t po = (size_t)b * plan_stride;
  const int32_t* ptok = plan_token + po;
  const int32_t* pdep = plan_depth + po;
  const int32_t* pend = plan_end + po;
  const int32_t* ppar = plan_parent + po;
  int NP = plan_n[plan_stride ? b : 0];
  NP = NP < 0 ? 0 : (NP > plan_rows ? plan_rows : NP);
  const int p0 = pos[b];
  int ngen = n_generated[b];
  int a = node_p[b];
  if (a < 0 || a >= NP) a = -1;          // (a node outside the plan: the row has left the trie)
  int m = verify_rows(len_p[b], Rin);
  m = a < 0 ? 1 : min(m, NP - a);
  const bool live = verify_live(done[b], p0, S, ngen, max_new);
  int now_done = live ? 0 : 1;
  int p = p0, nc = 0, nd = a;
  // ---- SAMPLE: the picks' scratch; under a penalty the bitmap of the ids generated before this step
  SampleLds sl{};
  bool pen = false;
  if constexpr (SAMPLE) {
    sl = SampleLds{erow, sample_bitmap_at(erow, V, sa.row_in_lds), redf, wtotf, redi, wtoti};
    pen = sa.rep != 1.f;
    if (live && pen) sample_bitmap_build(sl.bm, row_ids, sa.gen_start[b], p0, V);
  }

  // ---- walk: scan local row j, commit its arg-max (SAMPLE: its sampled pick), move to the child under that token while this
  // pass fed it
  if (live) {
    int j = 0;
    for (;;) {
      const float* lg = logits + ((size_t)b * Rin + j) * V;
      float lse;
      int g, kept = 1;
      if constexpr (SAMPLE)                                        // the sampled pick, with the draw of this token's index
        g = row_sample(lg, V, sample_draw(sa.u, ngen, max_new, B, b), sa, pen, sl, kept, lse);
      else
        g = row_verify(lg, V, redf, redi, lse);
      p += 1;
      ngen += 1;
      if (tid == 0) {
        cm[nc] = g;
        row_ids[p] = g;                                            // (p <= S - 1: checked before every commit)
        token_out[(size_t)b * WALK + nc] = g;
        logprob_out[(size_t)b * WALK + nc] = lg[g] - lse;
        path_o[(size_t)b * WALK + nc] = j;
        if constexpr (SAMPLE) sa.n_kept[(size_t)b * WALK + nc] = kept;
      }
      if constexpr (SAMPLE) {
        if (pen) sample_bitmap_add(sl.bm, g);                      // the next row of the walk sees what this one committed
      }
      nc += 1;
      if ((stop_at_eos && g == eos_id) || ngen >= max_new) { now_done = 1; nd = -1; break; }
      if (p + 1 >= S) { nd = -1; break; }                          // no room: m' = 0, done at the next step
      if (nd < 0) break;                                           // off the trie: one token per pass
      const int G = a + j;                                         // (a <= G < a + m <= NP)
      const int e = min(pend[G], NP);
      int c = NONE;
      for (int r = G + 1 + tid; r < e; r += NT)
        if (ppar[r] == G && ptok[r] == g) { c = r; break; }
      c = block_min_int(c, redi);
      if (c == NONE) { nd = -1; break; }
      nd = c;
      if (c - a >= m || nc >= WALK) break;                         // the child was cut from this pass: the next one's root
      j = c - a;
    }
  }
  __syncthreads();                                                 // (cm is published; every read of pos / done / len / node is over)

  // ---- the next pass: the plan rows [nd, nd + m2)
  const int P = p;
  const int at = valid_pos(P, S);
  int m2 = 0;
  if (!now_done) {
    const int dmax = min(DREL, min(max_new - ngen - 1, S - 2 - P));
    if (dmax >= 0 && nd < 0) m2 = 1;
    if (dmax >= 0 && nd >= 0) {
      int e = min(min(pend[nd], nd + Rout), NP);
      if (e < nd + 1) e = nd + 1;
      const int d0 = pdep[nd];
      int cut = NONE;
      for (int r = nd + 1 + tid; r < e; r += NT)
        if ((long long)pdep[r] - d0 > dmax) { cut = r; break; }
      cut = block_min_int(cut, redi);
      m2 = min(e, cut) - nd;
    }
  }
  for (int j = tid; j < Rout; j += NT) {                           // local depth / end; padding rows: depth 0, end = own index + 1
    int dl = 0, el = j + 1;
    if (nd >= 0 && j < m2) {
      const int r = nd + j;
      const long long d = (long long)pdep[r] - pdep[nd], e = (long long)pend[r] - nd;
      dl = d < 0 ? 0 : (d > DREL ? DREL : (int)d);
      el = e < j + 1 ? j + 1 : (e > m2 ? m2 : (int)e);
      if (j >= 1) wn[j] = valid_token(ptok[r], V);
    }
    depth_o[(size_t)b * Rout + j] = dl;
    end_o[(size_t)b * Rout + j] = el;
  }
  const int tiles = (Rout + TILE - 1) / TILE;
  if (tid < tiles) {                                               // the chain of each tile's first row, root first, over `parent`
    int32_t* anc = anc_o + ((size_t)b * tiles + tid) * TILE;
    for (int i = 0; i < TILE; ++i) anc[i] = -1;
    const int q = tid * TILE;
    if (nd >= 0 && q > 0 && q < m2) {
      const long long d = (long long)pdep[nd + q] - pdep[nd];
      int k = d < 0 ? 0 : (d > DREL ? DREL : (int)d);
      int r = nd + q;
      while (k > 0) {
        const int pr = ppar[r];
        if (pr < nd || pr >= r) break;                             // (a parent lies in front of its child, inside the pass)
        anc[--k] = pr - nd;
        r = pr;
      }
    }
  }
  if (tid == 0) {
    wn[0] = live ? cm[nc - 1] : valid_token(row_ids[at], V);
    // ---- the row's state (a row that committed nothing keeps its ids, pos, n_generated and node) and the step's results
    if (live) {
      pos[b] = p;
      n_generated[b] = ngen;
      node_p[b] = nd;
    }
    done[b] = now_done;
    len_p[b] = m2;
    start_p[b] = at;
    if (pos64) pos64[b] = at;
    verify_pad(token_out, logprob_out, (size_t)b * WALK, nc, WALK);
    if constexpr (SAMPLE) {
      for (int j = nc; j < WALK; ++j) sa.n_kept[(size_t)b * WALK + j] = 0;
    }
    for (int j = nc; j < WALK; ++j) path_o[(size_t)b * WALK + j] = 0;
    n_path[b] = nc;
    start_old[b] = valid_pos(p0, S);
    n_committed[b] = nc;
    n_drafted[b] = live ? m - 1 : 0;
    ticket_arrive(counter, n_active, B, !now_done);
    ticket_arrive(counter + 1, n_on_trie, B, !now_done && nd >= 0);
  }
  __syncthreads();
  // ---- the next pass's input rows: emb of the last committed token, then of the plan rows' tokens; zeros behind
  next_pass_rows(x_next, emb, b, Rout, D, vec16, tid, m2 < 1 ? 1 : m2, [&](int j) { return wn[j]; });
}

// grid (WALK, n_seq, n_layers): workgroup (i, n, l) appends path entry i of sequence n in layer l, 8 elements per thread and turn
template <typename T>
__global__ __launch_bounds__(NT) void kv_tree_commit_k(T* __restrict__ cache, const T* __restrict__ rows,
                                                       const int32_t* __restrict__ path, const int32_t* __restrict__ n_path,
                                                       const int32_t* __restrict__ start_old, const float* __restrict__ cs,
                                                       const float* __restrict__ sn, int B, int R, int S, int D, int A, int rot) {
  const int i = blockIdx.x, n = blockIdx.y, l = blockIdx.z, tid = threadIdx.x;
  const int np = n_path[n];
  if (i >= (np > WALK ? WALK : np)) return;
  const int st = start_old[n], j = path[(size_t)n * WALK + i];
  if (st < 0 || st + i >= S || j < 0 || j >= R) return;            // (an entry that leads outside an operand appends nothing)
  const int at = st + i;
  const size_t ld = (size_t)3 * D;
  const T* src = rows + (((size_t)l * B + n) * R + j) * ld;
  T* dst = cache + ((size_t)l * ((size_t)B * S + A) + (size_t)n * S + at) * ld;
  constexpr int HP = 64;                                           // rotation pairs of a head (head_dim 128)
  for (int d = tid * 8; d < D; d += NT * 8) {
    if (rot) {
#pragma unroll
      for (int u = 0; u < 2; ++u) {                                // two pairs a turn: one Vec4 in, one out
        float k[4], kr[4];
        Vec4<T>::load(src + D + d + 4 * u, k);
        const size_t t0 = (size_t)at * HP + (d & 127) / 2 + 2 * u;
        rope_pair_as_decode<T>(k[0], k[1], cs[t0], sn[t0], kr[0], kr[1]);
        rope_pair_as_decode<T>(k[2], k[3], cs[t0 + 1], sn[t0 + 1], kr[2], kr[3]);
        Vec4<T>::store(dst + D + d + 4 * u, kr);
      }
    } else {
      copy_bits<8>(dst + D + d, src + D + d);
    }
    copy_bits<8>(dst + 2 * D + d, src + 2 * D + d);
  }
}

// the operand checks and the launch of both step entries; sa: the operands fvqa_tree_spec_step_sample adds (SAMPLE = true), else
// NULL
int tree_spec_step_launch(const float* logits, const void* emb, const int32_t* plan_n, const int32_t* plan_token,
                          const int32_t* plan_depth, const int32_t* plan_end, const int32_t* plan_parent, int plan_rows,
                          int plan_stride, int eos_id, int stop_at_eos, int max_new_tokens, int64_t* ids, int32_t* pos,
                          int32_t* done, int32_t* n_generated, int32_t* node, int32_t* len, int32_t* start, void* x_next,
                          int32_t* depth, int32_t* end, int32_t* tile_anc, int32_t* path, int32_t* n_path, int32_t* start_old,
                          int32_t* token, float* logprob, int32_t* n_committed, int32_t* n_drafted, int32_t* n_active,
                          int32_t* n_on_trie, uint32_t* counter, int64_t* pos64, int n_seq, int rows_in, int rows_out, int vocab,
                          int dim, int seq_len, int dtype, void* stream, const SampleArgs* sa) {
  if (!logits || !emb || !plan_n || !plan_token || !plan_depth || !plan_end || !plan_parent || !ids || !pos || !done ||
      !n_generated || !node || !len || !start || !x_next || !depth || !end || !tile_anc || !path || !n_path || !start_old ||
      !token || !logprob || !n_committed || !n_drafted || !n_active || !n_on_trie || !counter)
    return FVQA_EINVAL;
  if (!fvqa_dtype_ok(dtype)) return FVQA_EINVAL;
  if (const int rc = fvqa_sample_args_ok(sa); rc != FVQA_OK) return rc;
  if (n_seq <= 0 || rows_in <= 0 || rows_out <= 0 || vocab <= 0 || dim <= 0 || seq_len <= 0 || max_new_tokens <= 0 ||
      plan_rows <= 0)
    return FVQA_ESHAPE;
  if (plan_stride != 0 && plan_stride != plan_rows) return FVQA_ESHAPE;
  if (rows_in > RMAX || rows_out > RMAX || n_seq > 65535 || (int64_t)n_seq * rows_in > 65535 ||
      (int64_t)n_seq * rows_out > 65535 || (int64_t)n_seq * plan_rows > 0x7fffffffLL)
    return FVQA_ESHAPE;                                            // (the tickets count arrivals in 16 bits)
  if (!fvqa_aligned(fvqa_dtype_size(dtype), emb, x_next) ||
      !fvqa_aligned(4, logits, plan_n, plan_token, plan_depth, plan_end, plan_parent, pos, done, n_generated, node, len, start,
                    depth, end, tile_anc, path, n_path, start_old, token, logprob, n_committed, n_drafted, n_active, n_on_trie,
                    counter) ||
      !fvqa_aligned(8, ids, pos64))
    return FVQA_EALIGN;
  hipStream_t st = (hipStream_t)stream;
  SampleArgs s;
  size_t lds;
  if (const int rc = fvqa_sample_launch_args(sa, vocab, &s, &lds); rc != FVQA_OK) return rc;
  fvqa_by_dtype(dtype, [&](auto* t) {
    using T = std::remove_pointer_t<decltype(t)>;
    const int vec16 = fvqa_vec16(dim * sizeof(T), emb, x_next);
    auto launch = [&](auto sample) {                               // SAMPLE = sample.value
      constexpr bool SAMPLE = decltype(sample)::value;
      if constexpr (SAMPLE) fvqa_sample_lds_limit<tree_spec_step_k<T, true>>(true);
      hipLaunchKernelGGL((tree_spec_step_k<T, SAMPLE>), dim3(n_seq), dim3(NT), lds, st, logits, (const T*)emb, plan_n, plan_token,
                         plan_depth, plan_end, plan_parent, plan_rows, plan_stride, eos_id, stop_at_eos, max_new_tokens, ids, pos,
                         done, n_generated, node, len, start, (T*)x_next, depth, end, tile_anc, path, n_path, start_old, token,
                         logprob, n_committed, n_drafted, n_active, n_on_trie, counter, pos64, n_seq, rows_in, rows_out, vocab,
                         dim, seq_len, vec16, s);
    };
    if (sa) launch(std::true_type{});
    else launch(std::false_type{});
  });
  FVQA_CHECK_LAUNCH();
  return FVQA_OK;
}

}  // namespace

extern "C" int fvqa_tree_spec_step(const float* logits, const void* emb, const int32_t* plan_n, const int32_t* plan_token,
                                   const int32_t* plan_depth, const int32_t* plan_end, const int32_t* plan_parent, int plan_rows,
                                   int plan_stride, int eos_id, int stop_at_eos, int max_new_tokens, int64_t* ids, int32_t* pos,
                                   int32_t* done, int32_t* n_generated, int32_t* node, int32_t* len, int32_t* start, void* x_next,
                                   int32_t* depth, int32_t* end, int32_t* tile_anc, int32_t* path, int32_t* n_path,
                                   int32_t* start_old, int32_t* token, float* logprob, int32_t* n_committed, int32_t* n_drafted,
                                   int32_t* n_active, int32_t* n_on_trie, uint32_t* counter, int64_t* pos64, int n_seq,
                                   int rows_in, int rows_out, int vocab, int dim, int seq_len, int dtype, void* stream) {
  return tree_spec_step_launch(logits, emb, plan_n, plan_token, plan_depth, plan_end, plan_parent, plan_rows, plan_stride, eos_id,
                               stop_at_eos, max_new_tokens, ids, pos, done, n_generated, node, len, start, x_next, depth, end,
                               tile_anc, path, n_path, start_old, token, logprob, n_committed, n_drafted, n_active, n_on_trie,
                               counter, pos64, n_seq, rows_in, rows_out, vocab, dim, seq_len, dtype, stream, nullptr);
}

extern "C" int fvqa_tree_spec_step_sample(const float* logits, const float* u, const void* emb, const int32_t* plan_n,
                                          const int32_t* plan_token, const int32_t* plan_depth, const int32_t* plan_end,
                                          const int32_t* plan_parent, int plan_rows, int plan_stride, float temperature,
                                          float top_p, int top_k, float repetition_penalty, int eos_id, int stop_at_eos,
                                          int max_new_tokens, int64_t* ids, int32_t* pos, int32_t* done, int32_t* n_generated,
                                          const int32_t* gen_start, int32_t* node, int32_t* len, int32_t* start, void* x_next,
                                          int32_t* depth, int32_t* end, int32_t* tile_anc, int32_t* path, int32_t* n_path,
                                          int32_t* start_old, int32_t* token, int32_t* n_kept, float* logprob,
                                          int32_t* n_committed, int32_t* n_drafted, int32_t* n_active, int32_t* n_on_trie,
                                          uint32_t* counter, int64_t* pos64, int n_seq, int rows_in, int rows_out, int vocab,
                                          int dim, int seq_len, int dtype, void* stream) {
  const SampleArgs sa{u, temperature, top_p, top_k, repetition_penalty, gen_start, n_kept, 0};
  return tree_spec_step_launch(logits, emb, plan_n, plan_token, plan_depth, plan_end, plan_parent, plan_rows, plan_stride, eos_id,
                               stop_at_eos, max_new_tokens, ids, pos, done, n_generated, node, len, start, x_next, depth, end,
                               tile_anc, path, n_path, start_old, token, logprob, n_committed, n_drafted, n_active, n_on_trie,
                               counter, pos64, n_seq, rows_in, rows_out, vocab, dim, seq_len, dtype, stream, &sa);
}

extern "C" int fvqa_kv_tree_commit(void* qkv_cache, const void* qkv_rows, const int32_t* path, const int32_t* n_path,
                                   const int32_t* start_old, const float* cos_t, const float* sin_t, int n_seq, int rows,
                                   int seq_len, int n_heads, int head_dim, int adapter_len, int n_layers, int cache_rotated,
                                   int dtype, void* stream) {
  if (!qkv_cache || !qkv_rows || !path || !n_path || !start_old || qkv_cache == qkv_rows) return FVQA_EINVAL;
  if (cache_rotated && (!cos_t || !sin_t)) return FVQA_EINVAL;
  if (!fvqa_dtype_ok(dtype)) return FVQA_EINVAL;
  if (n_seq <= 0 || n_seq > 65535 || rows <= 0 || rows > RMAX || seq_len <= 0 || n_heads <= 0 || head_dim != 128 ||
      adapter_len < 0 || n_layers <= 0 || n_layers > 65535)
    return FVQA_ESHAPE;
  if (!fvqa_aligned(16, qkv_cache, qkv_rows) || !fvqa_aligned(4, path, n_path, start_old, cos_t, sin_t)) return FVQA_EALIGN;
  hipStream_t st = (hipStream_t)stream;
  fvqa_by_dtype(dtype, [&](auto* t) {
    using T = std::remove_pointer_t<decltype(t)>;
    hipLaunchKernelGGL(kv_tree_commit_k<T>, dim3(WALK, n_seq, n_layers), dim3(NT), 0, st, (T*)qkv_cache, (const T*)qkv_rows, path,
                       n_path, start_old, cos_t, sin_t, n_seq, rows, seq_len, n_heads * head_dim, adapter_len,
                       cache_rotated ? 1 : 0);
  });
  FVQA_CHECK_LAUNCH();
  return FVQA_OK;
}
