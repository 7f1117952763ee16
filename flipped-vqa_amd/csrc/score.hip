// Answer-option scoring (reference engine.py:86-93 + llama/model_my_original_mod.py:332-377: every option of a sample is run
// through the model, per-token cross-entropy with ignore_index 0, the option with the lowest mean loss is chosen).
//
// The O option sequences of a sample are equal up to the first answer token, and with causal attention so are their hidden
// states: the prompt is run ONCE (the training forward, which leaves every layer's k / v in the arena = the KV cache) and
// each option only recomputes its last T rows, the "suffix" (fvqa/score.py). One kernel template, attn_suffix_k, behind five entries:
//
// fvqa_attn_suffix — Attention.forward (llama/model.py:87-128) at the suffix rows. Query row (n, c, j) sits at position
//   start[n] + j and attends to
//     * the cached keys / values [0, start[n]) of sample n (read, never written: O continuations share one cache),
//     * rows 0..j of its OWN option's suffix (rotated here and rounded to the storage type, as the prefill holds them),
//     * the A adapter keys (no RoPE, own softmax scaled by tanh(gate1[h])),
//   with gate2[h] added on the frame keys [vs, vs+F) when the query position is >= vs+F, wherever that window lies — in the
//   cache, across start[n] or inside the suffix; vs < 0: no window.
//   One 256-thread workgroup per (head, sample): each cached key / value row is loaded ONCE for all O*T queries of the sample
//   (a workgroup per option would read the prompt O times). Queries are taken in tiles of 32, keys in chunks of 32 staged in
//   LDS as fp32; a running (max, sum) per query carries the softmax across chunks — the sums run in one fixed order, there
//   are no atomics, two launches give the same bits. No matrix cores: 20..80 query rows per (head, sample) against <= 128 keys
//   is a few hundred kFLOP next to the weight streams of the projections around it.
//   Rows j >= len[n] are padding: never loaded (a NaN there reaches nothing), their output rows are written as zeros.
//
// fvqa_attn_suffix_append — the same kernel template with APPEND = true (fvqa_attn_suffix instantiates APPEND = false, in which
//   none of the following exists), for ONE continuation per sample (draft-and-verify decoding, fvqa/generate.py): the suffix
//   rows join the cache. The (head, sample) workgroup already stages its head's slice of every suffix key and value once; the
//   threads that stage row j < len[n] also store it to cache row n*S + start[n] + j — k rotated and rounded when the cache holds
//   rotated keys (csrc/cache_row.h rope_pair_as_decode: the bits fvqa_attn_decode stores for that row and position), the raw bits
//   otherwise; v as it is. Nothing reads those rows in this launch: a workgroup reads the cache rows [0, start[n]) only.
//
// fvqa_attn_suffix_mass — the same body with MASS = true (APPEND = false): o_suf bit for bit, and per query row the summary of its
//   text softmax over the frame window (include/fvqa.h); score_options(frame_attention=True), fvqa/score.py.
//
// fvqa_attn_suffix_wide — the same tile with WIDE = true, for 1 <= suffix_len <= 64 (fvqa/flipped.py: a VAQ option differs at its
//   answer and the scored question follows it, a QAV option has its frame slots behind the answer). One workgroup per (head,
//   sample, option x tile of 32 queries): the (head, sample) workgroup would walk O * T / 32 = 10 tiles in a row at five options
//   of 64 rows; here the tiles run side by side and the prompt's keys are read once per tile, from L2 after the first. A tile
//   stages the suffix keys of its own option up to its last query only. The tile is written in the kernel, not in a function of
//   its own: which products hipcc contracts into fmas in the score and value passes changes when the same text is inlined from
//   a __device__ function, and with it the last bit of the output (profiles/suffix_refactor.log).
//
// fvqa_attn_suffix_tree — the same tile with TREE = true: the suffix rows of a sample are the nodes of a tree, a row sees the cache
//   and its ancestors-or-self (fvqa/vocab.py: every allowed answer in one pass; fvqa/generate.py: a trie of drafts). WIDE's grid
//   with one "option"; what differs is where a key row and its position come from (depth, the chain of a tile's first row) and who
//   sees it (the pre-order interval test) — stated at the template.
//
// fvqa_option_pick — the per-option reduction: compact per-row losses (fvqa_ce_fwd) -> individual_losses (B, O, S-1) with
//   zeros wherever no row was scored, per option sum / count of non-zero entries / mean, and argmin over options with torch's
//   rule (first NaN wins, ties to the lowest index). One workgroup per sample, fixed summation order.
#include "attn_decode_body.h"
#include "cache_row.h"

namespace {
using namespace fvqa_decode;

constexpr int TMAX = 16;                 // suffix rows per option (fvqa_attn_suffix, _mass, _append)
constexpr int TWIDE = 64;                // suffix rows per option (fvqa_attn_suffix_wide)
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

// 16 values to 16 consecutive elements of a row, rounded to the storage type
template <typename T> __device__ __forceinline__ void store16_as(T* dst, const float (&v)[16]) {
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const float q[4] = {v[4 * u], v[4 * u + 1], v[4 * u + 2], v[4 * u + 3]};
    Vec4<T>::store(dst + 4 * u, q);
  }
}

// element I of a parameter pack
template <int I, typename P, typename... Ps> __device__ __forceinline__ auto pack_at(P p, Ps... ps) {
  if constexpr (I == 0) return p;
  else return pack_at<I - 1>(ps...);
}

constexpr int MFMAX = 64;                // max_feats under MASS (include/fvqa.h fvqa_attn_suffix_mass): F + 2 <= MLD
constexpr int MLD = 72;                  // LDS row stride of the summary accumulators (floats): lanes (4 queries) x (8 entries) of a
                                         // half wave on 32 distinct banks (72 = 8 mod 32); 32 x 72 x 4 B = 9 KiB, 62.6 KiB in all

// MASS: each query row's frame-attention summary goes to mass (n_seq * n_options * suffix_len, n_heads, F + 2) fp32 as well
// (include/fvqa.h fvqa_attn_suffix_mass states the quantity). The online softmax keeps no probabilities, so the F + 2 entries are
// running accumulators per query of the tile (Ms), carried like acc: rescaled by alpha[q] in every text chunk, the chunk's Ps
// added — a frame entry has at most one key per chunk that its query sees; the two sums in front of and behind the window run
// over the half wave's butterfly in the score pass (fb) —, multiplied by 1 / lrun[q] and stored in the adapter chunk, where the
// text softmax has closed. Thread (q = tid / 8, e = tid % 8 + 8 m) owns entry e of query q from the first chunk to the store.
// false compiles none of it; the summary's pointer is an operand of the MASS instantiations only (M: `float` there, an empty
// pack otherwise), so the other kernels keep their operands and their code.
//
// TREE (fvqa_attn_suffix_tree): the Tn suffix rows of a sample (O = 1, len[n] of them real) are the nodes of a tree in pre-order
// (fvqa/vocab.py: the internal nodes of a trie of allowed answers). Row r sits at position start[n] + depth[r] and sees the cache
// rows [0, start[n]), the rows that are its ancestors-or-self and the adapter keys. In pre-order, a is an ancestor-or-self of q
// iff a <= q < end[a], and every ancestor of a row of the 32-row tile from q0 lies in the tile or is an ancestor of q0: the tile's
// suffix keys are ONE chunk of q0's ancestors (anc, root first: depth[q0] <= 31 of them; none for a root) and ONE chunk of the
// tile's own rows, both under the interval test. One tile per workgroup, as WIDE has them. depth, end (n_seq, Tn) and the tiles'
// chains anc (n_seq, tiles, 32) are operands of this instantiation only (M: three `const int32_t`); every index read from them is
// clamped before it is used.
constexpr int TREE_DEPTH = FVQA_TREE_DEPTH_MAX;      // deepest row under TREE: a tile's ancestor chain fits one chunk
static_assert(TREE_DEPTH < KC, "the chain of a tile's first row is one chunk of keys");

template <typename T, bool APPEND = false, bool MASS = false, bool WIDE = false, bool TREE = false, typename... M>
__global__ __launch_bounds__(256) void attn_suffix_k(const T* __restrict__ suf, const T* __restrict__ cache,
                                                     T* __restrict__ o_suf, const float* __restrict__ gate1,
                                                     const float* __restrict__ gate2, const int32_t* __restrict__ vstart,
                                                     const int32_t* __restrict__ start_p, const int32_t* __restrict__ len_p,
                                                     const float* __restrict__ cs, const float* __restrict__ sn, int B, int O,
                                                     int Tn, int S, int H, int A, int F, int cache_rot,
                                                     M* __restrict__... more) {
  static_assert(APPEND + MASS + WIDE + TREE <= 1 && sizeof...(M) == (MASS ? 1 : TREE ? 3 : 0),
                "one switch at a time; mass: one fp32 pointer under MASS; depth, end, anc under TREE");
  constexpr bool TILED = WIDE || TREE;                           // one tile per workgroup, named by blockIdx.z
  __shared__ __attribute__((aligned(16))) float Qs[QT][KLD];     // the tile's queries: rotated, rounded
  __shared__ __attribute__((aligned(16))) float Ks[KC][KLD];     // the chunk's keys, as the prefill holds them
  __shared__ __attribute__((aligned(16))) float Vs[KC][DH];
  __shared__ __attribute__((aligned(16))) float Ps[QT][KC];      // the chunk's probabilities (unnormalised)
  __shared__ float mrun[QT], lrun[QT], alpha[QT];
  __shared__ float Ms[MASS ? QT : 1][MASS ? MLD : 1];            // (MASS) the summary's running accumulators
  __shared__ float fb[MASS ? QT : 1][2];                         // (MASS) the chunk's sums in front of / behind the window
  const int tid = threadIdx.x;
  const int h = blockIdx.x, n = blockIdx.y;
  const int D = H * DH;
  const size_t ld = (size_t)3 * D;
  int start = start_p[n];
  const int start_max = TREE ? S - 1 : S;                  // (TREE: the root's position is inside the sequence)
  start = start < 0 ? 0 : (start > start_max ? start_max : start);
  int len = len_p[n];
  len = len < 0 ? 0 : (len > Tn ? Tn : len);
  if constexpr (!TREE)
    if (len > S - start) len = S - start;
  const int NQ = O * Tn;
  const T* seq = cache + (size_t)n * S * ld + h * DH;
  const T* arow = cache + (size_t)B * S * ld + h * DH;
  const T* sufn = suf + (size_t)n * NQ * ld + h * DH;
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

  // The sample's O * Tn suffix rows are numbered row-major ("flattened" row r is suffix row r % Tn of option r / Tn). A tile is
  // 32 flattened rows from q0, its queries those below q_end; the flattened rows [s_lo, s_hi) are staged as its suffix keys, in
  // chunks of KC from s_lo. A query sees a suffix key iff both are rows of one option, the key's suffix row is not behind the
  // query's and is < len.
  //   narrow: the workgroup walks the tiles of all NQ rows; a tile may run across options and stages the options it touches.
  //   WIDE: the workgroup has the one tile blockIdx.z names, 32 rows from suffix row w_j0 of the option whose first row is w_lo,
  //         and stages that option's rows up to its last query: suffix rows are differences, the option test is compiled out.
  //   TREE: WIDE's tile of the one option (w_lo = 0); it stages its own rows only, behind the chunk of q0's chain, and a row's
  //         position and who sees it come from depth / end.
  int w_lo = 0, w_j0 = 0;
  if constexpr (TILED) {
    const int NT = (Tn + QT - 1) / QT;
    w_lo = TREE ? 0 : (blockIdx.z / NT) * Tn;
    w_j0 = TREE ? blockIdx.z * QT : (blockIdx.z % NT) * QT;
    if (w_j0 >= len) {                                   // a tile of padding rows (the whole workgroup takes this branch)
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        const int j = w_j0 + 16 * qh + u;
        if (j < Tn) o_suf[((size_t)n * NQ + w_lo + j) * D + h * DH + vd] = from_f32<T>(0.f);
      }
      return;
    }
  }
  const auto row_j = [&](int r) { return TILED ? r - w_lo : r % Tn; };                 // a flattened row's suffix row,
  const auto row_c = [&](int r) { return TILED ? 0 : r / Tn; };                        // its option,
  const auto row_first = [&](int r) { return TILED ? w_lo : (r / Tn) * Tn; };          // its option's first row
  // (TREE) the depth and the subtree's end of a real row r < len, clamped: a position stays inside the sequence, end in (r, len]
  const int32_t *depth = nullptr, *end = nullptr, *anc = nullptr;
  int dmax = 0;
  if constexpr (TREE) {
    depth = pack_at<0>(more...) + (size_t)n * Tn;
    end = pack_at<1>(more...) + (size_t)n * Tn;
    anc = pack_at<2>(more...) + ((size_t)n * gridDim.z + blockIdx.z) * KC;
    dmax = S - 1 - start < TREE_DEPTH ? S - 1 - start : TREE_DEPTH;
  }
  const auto depth_of = [&](int r) { const int d = depth[r]; return d < 0 ? 0 : (d > dmax ? dmax : d); };
  const auto end_of = [&](int r) { const int e = end[r]; return e < r + 1 ? r + 1 : (e > len ? len : e); };
  const auto row_pos = [&](int r) { return start + (TREE ? depth_of(r) : row_j(r)); };  // a (TREE: real) row's position
  const int q_first = TILED ? w_lo + w_j0 : 0, q_last = TILED ? q_first + 1 : NQ, q_end = TILED ? w_lo + Tn : NQ;
  for (int q0 = q_first; q0 < q_last; q0 += QT) {
    // ---- the tile's queries
    {
      const int qi = q0 + srow;
      const int j = row_j(qi);
      float v[16];
      if (qi < q_end && j < len) {
        load16<T>(sufn + (size_t)qi * ld + sd0, v);
        rope16<T>(v, cs, sn, row_pos(qi), sd0);
      } else {
#pragma unroll
        for (int e = 0; e < 16; ++e) v[e] = 0.f;
      }
      store16(&Qs[srow][sd0], v);
      if (tid < QT) { mrun[tid] = -1e30f; lrun[tid] = 0.f; }
      if constexpr (MASS)
        for (int e = tid & 7; e < F + 2; e += 8) Ms[srow][e] = 0.f;
    }
    float acc[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) acc[u] = 0.f;
    // what this thread's four score queries are
    int qj[4], qc[4], qpos[4];
    bool qok[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int qi = q0 + 4 * qg + u;
      qc[u] = row_c(qi);
      qj[u] = row_j(qi);
      qok[u] = qi < q_end && qj[u] < len;
      qpos[u] = !TREE || qok[u] ? row_pos(qi) : start;
    }
    const int s_lo = TREE ? q0 : row_first(q0);
    int s_hi = ((q0 + QT - 1) / Tn + 1) * Tn;
    if (s_hi > NQ) s_hi = NQ;
    if constexpr (TILED) s_hi = w_lo + (w_j0 + QT < len ? w_j0 + QT : len);
    int n_anc = 0;                                       // (TREE) q0's proper ancestors: the keys of the chain chunk
    if constexpr (TREE) n_anc = depth_of(q0);
    const int n_chain = n_anc > 0 ? 1 : 0;
    const int n_pre = (start + KC - 1) / KC, n_suf = n_chain + (s_hi - s_lo + KC - 1) / KC;
    // chunks: [0, n_pre) cached prompt keys, [n_pre, n_pre + n_suf) suffix keys (TREE: the chain of q0 if it has one, then the
    // tile's own rows), then the adapter keys (own softmax)
    for (int ch = 0; ch <= n_pre + n_suf; ++ch) {
      const int kind = ch < n_pre ? 0 : (ch < n_pre + n_suf ? 1 : 2);
      const int k0 = kind == 0 ? ch * KC : (kind == 1 ? s_lo + (ch - n_pre - n_chain) * KC : 0);
      const bool chain = TREE && kind == 1 && ch < n_pre + n_chain;
      // r: the suffix row that key column c of a suffix chunk holds, if it holds one (the chain's rows come from anc, the others
      // lie in order)
      const auto key_row = [&](int c, int& r) {
        r = k0 + c;
        if (chain) {
          r = c < n_anc ? anc[c] : -1;
          return r >= 0 && r < q0;                       // (an ancestor of q0 lies in front of it)
        }
        return r < s_hi && row_j(r) < len;
      };
      __syncthreads();                                   // the previous chunk's readers are done (and Qs / mrun are written)
      if (kind == 2 && tid < QT) {                       // text softmax closed: o = acc / l, then the adapter's share is added
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
          int r;
          if (key_row(srow, r)) { row = sufn + (size_t)r * ld; pos = row_pos(r); rot = true; }
        } else if (ki < A) {
          row = arow + (size_t)ki * ld;
        }
        if (row) {
          load16<T>(row + D + sd0, k);
          load16<T>(row + 2 * D + sd0, v);
          if constexpr (APPEND) {                        // (O == 1: one tile, one suffix chunk — each row is staged once)
            if (kind == 1) {
              T* crow = const_cast<T*>(seq) + (size_t)pos * ld;      // pos = start + j < S: len <= S - start
              if (cache_rot) {
                float kr[16];
#pragma unroll
                for (int e = 0; e < 8; ++e)
                  rope_pair_as_decode<T>(k[2 * e], k[2 * e + 1], cs[(size_t)pos * HP + sd0 / 2 + e],
                                         sn[(size_t)pos * HP + sd0 / 2 + e], kr[2 * e], kr[2 * e + 1]);
                store16_as<T>(crow + D + sd0, kr);
              } else {
                copy_bits<16>(crow + D + sd0, row + D + sd0);
              }
              copy_bits<16>(crow + 2 * D + sd0, row + 2 * D + sd0);
            }
          }
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
      int kpos = ki, kc = -1, kj = 0, kend = 0;
      bool kok;
      if (kind == 0) {
        kok = ki < start;
      } else if (kind == 1) {
        int r;
        kok = key_row(kk, r);
        if constexpr (TREE) {
          kj = r;
          if (kok) { kpos = row_pos(r); kend = end_of(r); }
        } else {
          kc = row_c(ki);
          kj = row_j(ki);
          kpos = start + kj;
        }
      } else {
        kok = ki < A;
      }
      const bool frame_key = kind != 2 && vs >= 0 && kpos >= vs && kpos < vs + F;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        bool see = qok[u] && kok;                          // suffix keys: rows of one option (TREE: ancestor-or-self), not behind
        if (kind == 1) see = see && kj <= qj[u] && (TREE ? qj[u] < kend : kc == qc[u]);
        float x = s[u] * scale;
        if (frame_key && qpos[u] >= vs + F) x += g2;
        x = see ? x : -1e30f;
        const int q = 4 * qg + u;
        const float m_old = mrun[q];
        const float m_new = fmaxf(m_old, half_max(x));
        const float e = see ? __expf(x - m_new) : 0.f;
        const float sum = half_sum(e);
        if constexpr (MASS) {
          if (kind != 2) {                                 // (a key the query does not see has e = 0)
            const float fr = half_sum(vs >= 0 && kpos < vs ? e : 0.f);
            const float bk = half_sum(vs < 0 || kpos >= vs + F ? e : 0.f);
            if (kk == 0) { fb[q][0] = fr; fb[q][1] = bk; }
          }
        }
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
        if (kk == 0) mrun[q] = m_new;      // (read above by this half wave only: each query belongs to one)
      }
      __syncthreads();
      if constexpr (MASS) {
        float* __restrict__ mass = pack_at<0>(more...);
        // ---- the summary: Ms[q][e] = Ms[q][e] * alpha[q] + the chunk's weight on entry e; closed and stored in the adapter chunk
        const int q = srow, qi = q0 + q;
        const float al = alpha[q];
        const int k1 = row_first(qi) - start - k0;        // suffix chunk: the key at position kpos of the query's own option
        for (int e = tid & 7; e < F + 2; e += 8) {
          const float m = Ms[q][e] * al;
          if (kind == 2) {
            if (qi < q_end) mass[(((size_t)n * NQ + qi) * H + h) * (F + 2) + e] = row_j(qi) < len ? m : 0.f;
          } else {
            float add = e == F ? fb[q][0] : fb[q][1];
            if (e < F) {
              const int kp = vs + e;                       // the frame key's position
              const int k = kind == 0 ? kp - k0 : kp + k1;
              const bool in = kind == 0 ? kp < start : (kp >= start && kp < start + Tn);
              add = vs >= 0 && in && k >= 0 && k < KC ? Ps[q][k] : 0.f;
            }
            Ms[q][e] = m + add;
          }
        }
      }
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
      const int qi = q0 + 16 * qh + u;
      if (qi < q_end) {
        const bool ok = row_j(qi) < len;
        o_suf[((size_t)n * NQ + qi) * D + h * DH + vd] = from_f32<T>(ok ? acc[u] : 0.f);
      }
    }
    if constexpr (!TILED) __syncthreads();               // Qs / mrun are rewritten by the next tile
  }
}

// one workgroup per sample: clear, scatter, reduce per option, pick
__global__ __launch_bounds__(256) void option_pick_k(const float* __restrict__ rowloss, const int32_t* __restrict__ map, int M,
                                                     float* __restrict__ il, float* __restrict__ sum_o,
                                                     int64_t* __restrict__ cnt_o, float* __restrict__ mean_o,
                                                     int64_t* __restrict__ pred, int O, int S1) {
  __shared__ float means[64];
  const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int per = O * S1;
  float* mine = il + (size_t)n * per;
  for (int i = tid; i < per; i += 256) mine[i] = 0.f;
  __syncthreads();
  for (int r = tid; r < M; r += 256) {
    const int at = map[r] - n * per;                     // (a row listed twice would race: the host lists each once)
    if (map[r] >= 0 && at >= 0 && at < per) mine[at] = rowloss[r];
  }
  __syncthreads();
  for (int c = w; c < O; c += 4) {
    float s = 0.f;
    int k = 0;
    for (int t = lane; t < S1; t += 64) {
      const float x = mine[c * S1 + t];
      s += x;
      k += (x != 0.f) ? 1 : 0;                           // reference engine.py:88 (a NaN counts, an exact 0 does not)
    }
    s = wave_sum(s);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) k += __shfl_xor(k, o, 64);
    if (lane == 0) {
      const float m = s / (float)k;                      // 0 / 0 = NaN, as torch
      sum_o[n * O + c] = s;
      cnt_o[n * O + c] = k;
      mean_o[n * O + c] = m;
      means[c] = m;
    }
  }
  __syncthreads();
  if (tid == 0) {
    int best = 0;
    for (int c = 0; c < O; ++c) {
      const float x = means[c], b = means[best];
      if (x != x) { best = c; break; }                   // torch.argmin: the first NaN wins
      if (x < b) best = c;                               // ties stay with the lowest index
    }
    pred[n] = best;
  }
}

// validates and launches the five entries: WIDE and TREE differ in the row limit and the grid, TREE in its operand limits too.
// more: the operands of one instantiation (MASS: the summary; TREE: depth, end, tile_anc)
template <bool APPEND, bool MASS = false, bool WIDE = false, bool TREE = false, typename... M>
int suffix_launch(const void* qkv_suf, const void* qkv_cache, void* o_suf, const float* gate1, const float* gate2,
                  const int32_t* vstart, const int32_t* start, const int32_t* len, const float* cos_t, const float* sin_t,
                  int n_seq, int n_options, int suffix_len, int seq_len, int n_heads, int head_dim, int adapter_len,
                  int max_feats, int cache_rotated, int dtype, void* stream, M*... more) {
  static_assert(APPEND + MASS + WIDE + TREE <= 1 && sizeof...(M) == (MASS ? 1 : TREE ? 3 : 0), "one switch at a time");
  if (!qkv_suf || !qkv_cache || !o_suf || !gate1 || !gate2 || !vstart || !start || !len || !cos_t || !sin_t)
    return FVQA_EINVAL;
  if ((... || !more)) return FVQA_EINVAL;
  if (!fvqa_dtype_ok(dtype)) return FVQA_EINVAL;
  if (n_seq <= 0 || n_options <= 0 || suffix_len <= 0 || suffix_len > (TREE ? FVQA_TREE_ROWS_MAX : WIDE ? TWIDE : TMAX) ||
      seq_len <= 0 || n_heads <= 0 || head_dim != DH || adapter_len < 0 || adapter_len > 16 || max_feats < 0)
    return FVQA_ESHAPE;
  if (seq_len > SMAX || n_heads > 65535 || n_seq > 65535 || n_options > 4096) return FVQA_ESHAPE;
  if (TREE && (long long)n_seq * suffix_len > FVQA_TREE_TOTAL_ROWS_MAX) return FVQA_ESHAPE;
  if (APPEND && n_options != 1) return FVQA_ESHAPE;      // (options share one cache: only a single continuation may join it)
  if (MASS && max_feats > MFMAX) return FVQA_ESHAPE;     // (the accumulators' LDS rows)
  if (((uintptr_t)qkv_suf | (uintptr_t)qkv_cache | (uintptr_t)o_suf) & 15) return FVQA_EALIGN;
  if ((0 | ... | (uintptr_t)more) & 3) return FVQA_EALIGN;
  if (TREE && (((uintptr_t)vstart | (uintptr_t)start | (uintptr_t)len) & 3)) return FVQA_EALIGN;
  const int tiles = (suffix_len + QT - 1) / QT;          // (WIDE: n_options * tiles <= 8192, TREE: 128, inside the grid's third axis)
  const dim3 grid(n_heads, n_seq, WIDE || TREE ? n_options * tiles : 1), block(256);
  hipStream_t st = (hipStream_t)stream;
  const auto launch = [&](auto* t) {                     // t: the storage type
    using T = std::remove_pointer_t<decltype(t)>;
    hipLaunchKernelGGL((attn_suffix_k<T, APPEND, MASS, WIDE, TREE, M...>), grid, block, 0, st, (const T*)qkv_suf,
                       (const T*)qkv_cache, (T*)o_suf, gate1, gate2, vstart, start, len, cos_t, sin_t, n_seq, n_options,
                       suffix_len, seq_len, n_heads, adapter_len, max_feats, cache_rotated, more...);
  };
  if (dtype == FVQA_H16) launch((bf16_t*)nullptr);
  else launch((float*)nullptr);
  FVQA_CHECK_LAUNCH();
  return FVQA_OK;
}

}  // namespace

extern "C" int fvqa_attn_suffix(const void* qkv_suf, const void* qkv_cache, void* o_suf, const float* gate1,
                                const float* gate2, const int32_t* vstart, const int32_t* start, const int32_t* len,
                                const float* cos_t, const float* sin_t, int n_seq, int n_options, int suffix_len,
                                int seq_len, int n_heads, int head_dim, int adapter_len, int max_feats, int cache_rotated,
                                int dtype, void* stream) {
  return suffix_launch<false>(qkv_suf, qkv_cache, o_suf, gate1, gate2, vstart, start, len, cos_t, sin_t, n_seq, n_options,
                              suffix_len, seq_len, n_heads, head_dim, adapter_len, max_feats, cache_rotated, dtype, stream);
}

extern "C" int fvqa_attn_suffix_mass(const void* qkv_suf, const void* qkv_cache, void* o_suf, const float* gate1,
                                     const float* gate2, const int32_t* vstart, const int32_t* start, const int32_t* len,
                                     const float* cos_t, const float* sin_t, int n_seq, int n_options, int suffix_len,
                                     int seq_len, int n_heads, int head_dim, int adapter_len, int max_feats,
                                     int cache_rotated, int dtype, void* stream, float* mass) {
  return suffix_launch<false, true>(qkv_suf, qkv_cache, o_suf, gate1, gate2, vstart, start, len, cos_t, sin_t, n_seq,
                                    n_options, suffix_len, seq_len, n_heads, head_dim, adapter_len, max_feats, cache_rotated,
                                    dtype, stream, mass);
}

extern "C" int fvqa_attn_suffix_append(const void* qkv_suf, void* qkv_cache, void* o_suf, const float* gate1,
                                       const float* gate2, const int32_t* vstart, const int32_t* start, const int32_t* len,
                                       const float* cos_t, const float* sin_t, int n_seq, int suffix_len, int seq_len,
                                       int n_heads, int head_dim, int adapter_len, int max_feats, int cache_rotated, int dtype,
                                       void* stream) {
  return suffix_launch<true>(qkv_suf, qkv_cache, o_suf, gate1, gate2, vstart, start, len, cos_t, sin_t, n_seq, 1, suffix_len,
                             seq_len, n_heads, head_dim, adapter_len, max_feats, cache_rotated, dtype, stream);
}

extern "C" int fvqa_attn_suffix_wide(const void* qkv_suf, const void* qkv_cache, void* o_suf, const float* gate1,
                                     const float* gate2, const int32_t* vstart, const int32_t* start, const int32_t* len,
                                     const float* cos_t, const float* sin_t, int n_seq, int n_options, int suffix_len,
                                     int seq_len, int n_heads, int head_dim, int adapter_len, int max_feats, int cache_rotated,
                                     int dtype, void* stream) {
  return suffix_launch<false, false, true>(qkv_suf, qkv_cache, o_suf, gate1, gate2, vstart, start, len, cos_t, sin_t, n_seq,
                                           n_options, suffix_len, seq_len, n_heads, head_dim, adapter_len, max_feats,
                                           cache_rotated, dtype, stream);
}

extern "C" int fvqa_attn_suffix_tree(const void* qkv_suf, const void* qkv_cache, void* o_suf, const float* gate1,
                                     const float* gate2, const int32_t* vstart, const int32_t* start, const int32_t* n_rows,
                                     const int32_t* depth, const int32_t* end, const int32_t* tile_anc, const float* cos_t,
                                     const float* sin_t, int n_seq, int rows, int seq_len, int n_heads, int head_dim,
                                     int adapter_len, int max_feats, int cache_rotated, int dtype, void* stream) {
  return suffix_launch<false, false, false, true>(qkv_suf, qkv_cache, o_suf, gate1, gate2, vstart, start, n_rows, cos_t, sin_t,
                                                  n_seq, 1, rows, seq_len, n_heads, head_dim, adapter_len, max_feats,
                                                  cache_rotated, dtype, stream, depth, end, tile_anc);
}

extern "C" int fvqa_option_pick(const float* rowloss, const int32_t* row_map, int n_rows, float* individual_losses,
                                float* option_sum, int64_t* option_count, float* option_mean, int64_t* prediction,
                                int n_seq, int n_options, int seq_len, void* stream) {
  if (!rowloss || !row_map || !individual_losses || !option_sum || !option_count || !option_mean || !prediction)
    return FVQA_EINVAL;
  if (n_rows < 0 || n_seq <= 0 || n_seq > 65535 || n_options <= 0 || n_options > 64 || seq_len < 2) return FVQA_ESHAPE;
  if ((long long)n_seq * n_options * (seq_len - 1) > 0x7fffffffLL) return FVQA_ESHAPE;
  hipLaunchKernelGGL(option_pick_k, dim3(n_seq), dim3(256), 0, (hipStream_t)stream, rowloss, row_map, n_rows,
                     individual_losses, option_sum, option_count, option_mean, prediction, n_options, seq_len - 1);
  FVQA_CHECK_LAUNCH();
  return FVQA_OK;
}
