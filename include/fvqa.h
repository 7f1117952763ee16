/*
 * fvqa.h — C ABI of libfvqa_hip.so: the MI355X (gfx950) kernels behind the Flipped-VQA
 * training hot path.
 *
 * The reference (inesriahi/Flipped-VQA) is pure Python/PyTorch: its hot path has no FFI of
 * its own — every entry below replaces an *implicit* torch op group of
 * llama/model.py:31-365, engine.py:10-56 and util/misc.py:253-294 (file:line cited per
 * entry, relative to the reference root). The Python host (flipped-vqa_amd/fvqa/_lib.py)
 * binds them with ctypes; INTEGRATION.md shows the stub a reference maintainer would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller (PyTorch caching allocator);
 *     the library never allocates, frees, synchronises or throws;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream);
 *   - `dtype` selects the storage type of activations / frozen weights:
 *       FVQA_F32  — exact-fp32 validation build of every kernel (fp32-in MFMA),
 *       FVQA_BF16 — production build (bf16 storage, fp32 accumulate);
 *       FVQA_F16  — the same with IEEE fp16 storage (libfvqa_hip_f16.so; wherever an entry below says "bf16" / FVQA_BF16 for
 *                   the 16-bit build, that library reads it as fp16 / FVQA_F16);
 *     trainable parameters, their gradients, softmax statistics and losses are always fp32;
 *   - matrices are row-major; `rows` = sequences*seq_len flattened (n*S + s);
 *   - return value: 0 (FVQA_OK) or a negative FVQA_E* code / -(1000+hipError_t).
 */
#ifndef FVQA_H
#define FVQA_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FVQA_F32 0
#define FVQA_BF16 1
#define FVQA_F16 2 /* IEEE fp16 storage — the reference's own (llama_vqa.py:63 builds the model under torch.cuda.HalfTensor). Served by
                      libfvqa_hip_f16.so: the same sources compiled with the 16-bit storage type switched (csrc/common.h), same
                      entry points; libfvqa_hip.so serves FVQA_BF16. Each library rejects the other's 16-bit code (FVQA_EINVAL),
                      both serve FVQA_F32. The host (fvqa/_lib.py) binds the library of the model's storage dtype. */

#define FVQA_OK 0
#define FVQA_EINVAL (-1) /* null pointer / bad enum            */
#define FVQA_ESHAPE (-2) /* dimension not supported by kernels */
#define FVQA_EALIGN (-3) /* pointer or leading dim misaligned  */

/* GEMM epilogue selector */
#define FVQA_EPI_NONE 0
#define FVQA_EPI_RESIDUAL 1 /* C = acc + R                                  */
#define FVQA_EPI_SWIGLU_BWD 3 /* acc = dz (M,N): R = ab (M,2N), C = dab (M,2N) <- d/d(a,b) of silu(a)*b
                                (llama/model.py:142 backward), both in the AB16 layout below; ldc must be 2N */
#define FVQA_EPI_SWIGLU_FWD 4 /* fvqa_gemm_nt_swiglu_fwd only: C = ab (M,N) AND z = silu(a)*b (M,N/2) */
#define FVQA_EPI_SWIGLU_FWD_ST 5 /* fvqa_gemm_nt_swiglu_fwd_st only: as 4, but C receives, in the a and b slots of the AB16
                                   layout, s = silu(a) = dz/db and t = b*sigma(a)*(1 + a*(1 - sigma(a))) = dz/da: what
                                   the backward of llama/model.py:142 multiplies by */
#define FVQA_EPI_SWIGLU_BWD_ST 6 /* as 3 with R = that (s, t) buffer: C = dab = (acc * t, acc * s) */
#define FVQA_EPI_ROPE 7          /* fvqa_gemm_nt_rope only: RoPE of the q | k columns of the QKV projection in the epilogue */
/* AB16: the layout of every (rows, 2*hidden) buffer that holds the W1 and W3 projections (or their gradients) side by
 * side: column 32k + c is a[16k + c], column 32k + 16 + c is b[16k + c] (c < 16), i.e. the rows of W1 and W3 are
 * interleaved in blocks of 16 in the packed W1|W3 matrix. One MFMA wave of the W1|W3 GEMM then holds a and b of the
 * same hidden unit in the same lane, and SwiGLU becomes that GEMM's epilogue. hidden % 16 == 0. */

int fvqa_version(void);      /* ABI version, bumped on any signature change: an entry that is only ADDED (no existing signature,
                              * message or order of outcomes moves) leaves it where it is */
/* sha256 (hex) of the kernel sources (csrc/ *.hip, *.h, include/fvqa.h) this library was compiled from, "unknown" for a build
 * outside fvqa/build.py. The host binding compares it with the sources next to the library and refuses a stale binary. */
const char* fvqa_source_hash(void);
const char* fvqa_arch(void); /* "gfx950"                                     */

/* ---- dense projections: F.linear with frozen weights ---------------------------------
 * C[M,N] = A[M,K] · B[N,K]^T (+ R[M,N]).  Replaces torch F.linear at llama/model.py:89
 * (wq/wk/wv), :99-100 (adapter k/v), :127-128 (wo), :142 (w1,w3,w2), :348 (output) and the
 * autograd dX = dY·W of each (W frozen ⇒ no dW GEMM; the host keeps a transposed copy of
 * every frozen weight so dX is the same NT form).  A and B have `dtype`; C has `out_dtype`
 * (FVQA_F32 for LM-head logits). Rows m >= m_split (if tail != NULL) are written as fp32 to
 * tail[(m - m_split)*N + n] (ACCUMULATED, +=) instead of C (adapter-query gradient rows).
 * Needs K % 64 == 0 (bf16) / K % 32 == 0 (fp32), 16-byte aligned rows.
 * variant 0 picks the kernel: the persistent 256x256-tile LDS-DMA ring kernel (M >= 192, N >= 256, N % 8 == 0, no
 * tail rows, workspace given; also 16 < M < 192 against >= 16 M weights: the projections of the tail rows, see
 * fvqa_row_segs), the weight-streaming kernel of the generation path for bf16 M <= 16, K % 256 == 0 (one
 * new token per sequence, llama/model.py:439-447 run row-wise; with C == NULL, m_split == 0 it accumulates every row
 * into `tail`: the adapter-query gradient rows), else the 128x128-tile kernel. Other variant codes force a kernel
 * (1 / 2 = 128x128 register- / DMA-staged, 12 = weight-streaming, 13 = persistent; tests, tuning). */
int fvqa_gemm_nt(const void* A, const void* B, void* C, const void* R, float* tail,
                 int M, int N, int K, int lda, int ldb, int ldc, int m_split,
                 int dtype, int out_dtype, int epilogue, int variant,
                 void* workspace, size_t workspace_bytes, void* stream);
/* ab[M, 2*hidden] = A[M,K] · B13[2*hidden,K]^T and z[M, hidden] = silu(a) * b in ONE launch of the persistent
 * kernel (llama/model.py:142: w1(x), w3(x) and their product; `ab` is what the backward needs). B13 is W1|W3 with rows
 * interleaved in blocks of 16 (AB16). Needs the fvqa_gemm_sk_workspace() workspace. */
int fvqa_gemm_nt_swiglu_fwd(const void* A, const void* B13, void* ab, void* z, int M, int hidden, int K, int lda,
                            int ldb, int dtype, void* workspace, size_t workspace_bytes, void* stream);
/* The training step's form: same product and the same z, but `st` (M, 2*hidden, AB16) receives the two factors of the
 * SwiGLU backward (FVQA_EPI_SWIGLU_FWD_ST) instead of a and b — nothing else on the training path reads a or b, and the
 * dH·W2^T GEMM's epilogue (FVQA_EPI_SWIGLU_BWD_ST) then is two multiplies per element instead of an exponential, a
 * reciprocal and a dozen operations (llama/model.py:142 and its autograd). */
int fvqa_gemm_nt_swiglu_fwd_st(const void* A, const void* B13, void* st, void* z, int M, int hidden, int K, int lda,
                               int ldb, int dtype, void* workspace, size_t workspace_bytes, void* stream);
/* fvqa_gemm_workspace: bytes of `workspace` the kernel variant 0 picks for the problem needs (0: none).
 * Its FIRST 4096 BYTES are the epoch flags of the persistent kernel (csrc/gemm_sk.hip): the caller zeroes them ONCE
 * after allocating the buffer (256-byte aligned); no call ever needs them reset. One workspace serves one stream at
 * a time. The first 64-bit word is an ERROR word: a workgroup whose bounded wait (~1 s) for a partner of a split tile
 * ran out sets it to non-zero and lets the grid drain — the outputs of that launch are then invalid. It is sticky; hand
 * its address to fvqa_grad_unscale_norm (the optimizer step of such a step is then skipped on the device) and read it
 * back at a convenient point (fvqa.ops.gemm_error / StepEngine.check_gemm_error; engine.train_one_epoch every iteration).
 * The bounded wait presumes that every workgroup of the grid is resident: the kernel asks for all 160 KiB of a CU's LDS and
 * launches at most one workgroup per CU of the CURRENT device, so the device must be this process's alone while a launch
 * runs (another process's persistent grid, or any kernel holding LDS on many CUs, can displace a partner: a 1 s stall and
 * the error word, not a hang). Launches into a stream under capture are refused (FVQA_EINVAL): the epoch number is a
 * host-side argument, and a replayed graph would reuse it. */
size_t fvqa_gemm_workspace(int M, int N, int K, int dtype);
/* The persistent kernel (variant 0 for M >= 192, N >= 256, N % 8 == 0, no tail rows; variant 13 forces it): a grid of
 * at most one workgroup per CU walks whole 256x256 output tiles, or — outputs with few tiles — one K range of a tile
 * each; a tile shared by several workgroups is reduced inside the launch (fixed order: bitwise repeatable) and stored
 * once with the epilogue.
 * fvqa_gemm_sk_workspace: 4096 flag bytes + one 256 KiB fp32 partial-tile slab per workgroup.
 * fvqa_gemm_sk_describe (host only, no GPU touched): the partition for a problem on n_cu compute units —
 * plan_out[12] = {tm, tn, wide stages per tile, stages per granule, granules per tile, team size, m groups, teams,
 * rounds of whole tiles, tiles of the last (split) round, pieces per tile there, team distance between the pieces of a
 * tile}; for team >= 0 also its segments, 5 ints each
 * {tile, k0, k1, pieces n, piece c} (up to max_segs written); returns the team's segment count. */
size_t fvqa_gemm_sk_workspace(void);

/* A second, independent product of at most 16 rows, C2[M2,N2] = A2[M2,K2] · B2[N2,K2]^T (operands in the main
 * problem's `dtype`), that rides on the compute units a projection leaves idle: the 10 adapter rows of
 * llama/model.py:98-100 (their K/V projections beside the QKV GEMM; their gradient rows into adapter_query.grad
 * beside the W2^T GEMM of the next layer walked). accumulate_f32 == 0: C2 has the storage dtype and is overwritten;
 * != 0: C2 is fp32 and the product is ADDED (ldc2 must then equal N2). */
typedef struct fvqa_sk_rider {
  const void* A; const void* B; void* C;
  int32_t M, N, K, lda, ldb, ldc;
  int32_t accumulate_f32;
} fvqa_sk_rider;
/* C = A·B^T (+ epilogue) exactly as fvqa_gemm_nt variant 0 (no tail rows), plus `rider`: inside the same launch when the
 * persistent kernel takes the main problem and leaves >= 16 CUs idle (bf16, M2 <= 16, K2 % 256 == 0), else as its
 * own launch right after it. The arithmetic of the rider is the same in both cases (bitwise-equal results). */
int fvqa_gemm_nt_rider(const void* A, const void* B, void* C, const void* R, int M, int N, int K, int lda, int ldb,
                       int ldc, int dtype, int out_dtype, int epilogue, const fvqa_sk_rider* rider,
                       void* workspace, size_t workspace_bytes, void* stream);
/* fvqa_gemm_nt_swiglu_fwd_st plus a rider (may be NULL), as fvqa_gemm_nt_rider: inside the launch when the kernel that takes
 * the main problem has workgroups to spare in its last round, else as its own launch right after. The step puts the NEXT
 * layer's adapter K/V rows here (they depend on parameters only): the W1|W3 launch of 1.8 rounds of 192-column tiles has 52
 * workgroups without a tile in its second round, the QKV launch of 256 such tiles none. */
int fvqa_gemm_nt_swiglu_fwd_st_rider(const void* A, const void* B13, void* st, void* z, int M, int hidden, int K, int lda,
                                     int ldb, int dtype, const fvqa_sk_rider* rider, void* workspace,
                                     size_t workspace_bytes, void* stream);
/* The QKV projection with RoPE where it is produced (bf16; reference llama/model.py:61-67 applied to wq(x), wk(x) :89-93):
 * C[M, N] = A · B^T with columns [0, rope->cols) — the q | k heads, rope->cols = 2 * n_heads * head_dim — rotated by the
 * tables (rows of head_dim / 2 floats per position, as fvqa_rope_qk takes them) of position (row % seq_len): value rounded to
 * bf16, rotated in fp32, rounded again, i.e. what fvqa_gemm_nt followed by fvqa_rope_qk leaves (which is what this entry runs
 * for shapes the persistent kernel does not take; ldc must then be 3 * n_heads * head_dim). M % seq_len == 0. The attention
 * kernels then read finished operands (cos_t == NULL) and no key tile is rotated once per query block; the backward takes
 * fvqa_attn_bwd_rotated. `rider` may be NULL. */
typedef struct fvqa_sk_rope {
  const float* cos_t; const float* sin_t;
  int32_t seq_len, head_dim, cols;
} fvqa_sk_rope;
int fvqa_gemm_nt_rope(const void* A, const void* B, void* C, int M, int N, int K, int lda, int ldb, int ldc,
                      const fvqa_sk_rope* rope, const fvqa_sk_rider* rider, void* workspace, size_t workspace_bytes,
                      void* stream);
int fvqa_gemm_sk_describe(int M, int N, int K, int dtype, int n_cu, int32_t* plan_out, int team,
                          int32_t* segs_out, int max_segs);
/* The whole-tile bf16 projections (outputs wide enough to fill the chip: q|k|v, w1|w3, dH·W2^T, LM head) run on tiles of
 * 256 rows x 16*nbt columns, nbt in {16, 14, 13, 12, 11} chosen per problem by a cost model so that the tile count lands on the
 * CU count. fvqa_gemm4w_choose (host only): the nbt the model picks for a problem on n_cu compute units, 0 when the problem is
 * not that kernel's (fp32 build, K % 64, M < 192, N < 256, an epilogue it does not have). `rider` may be NULL.
 * fvqa_gemm4w_force: tests / tuning — every following projection call OF THE CALLING HOST THREAD uses tiles of 16*nbt columns
 * where the kernel is eligible at all (odd nbt never with FVQA_EPI_SWIGLU_FWD_ST: (a, b) column blocks pair up); 0 restores the
 * cost model. Returns the previous setting, FVQA_EINVAL for a width that does not exist. */
int fvqa_gemm4w_choose(int M, int N, int K, int dtype, int out_dtype, int epilogue, const fvqa_sk_rider* rider, int n_cu);
int fvqa_gemm4w_force(int nbt);
/* Measurement probe (bench.py roofline; no reference counterpart): while enabled, launches of the persistent
 * 256x256 GEMM kernel are bracketed by HIP events on THEIR launch stream. enable(n): n = 1 brackets every launch, n > 1
 * every n-th launch (the others are only counted) — an event pair idles the chip for ~5 us, and a stream with one after
 * each of its 258 launches per step runs at a lighter duty cycle (on a power-limited chip: a higher clock) than the
 * un-instrumented step; a co-prime stride samples every launch position over a few steps at 1/n of that disturbance.
 * fvqa_gemm_timing_read synchronises, returns the number of launches recorded since enable and fills up to `max`
 * entries: duration (us; -2 = counted but not bracketed, -1 = event error), algorithmic FLOPs (2*M*N*K of that launch)
 * and kind = epilogue | split_k << 4 | out_is_f32 << 5 | in_is_f32 << 6 | four_wave_kernel << 7; it then clears the record (max <= 0: size query
 * only, nothing cleared). enable(0) stops recording and frees the probe. Launches from any host thread are recorded (the
 * step's backward runs on the autograd thread); switch it while no launch is in flight. */
int fvqa_gemm_timing_enable(int on);
int fvqa_gemm_timing_read(int max, float* us, double* flops, int* kind);

/* ---- RMSNorm (llama/model.py:37-42; used :185,186,347) -------------------------------- */
int fvqa_rmsnorm_fwd(const void* x, const void* w, void* y, float* rstd, int rows, int dim,
                     float eps, int dtype, void* stream);
/* dx = (resid ? resid : 0) + rmsnorm_bwd(g; x, w, rstd)   (no dw here: fvqa_rmsnorm_dw below, when the weight trains) */
int fvqa_rmsnorm_bwd(const void* g, const void* x, const void* w, const float* rstd,
                     const void* resid, void* dx, int rows, int dim, int dtype, void* stream);
/* The gradient of an RMSNorm's weight (--train_norm; the reference's autograd of llama/model.py:41-42 with the weight
 * unfrozen). Operands as fvqa_rmsnorm_bwd: g (rows, dim) the gradient w.r.t. the norm's output, x (rows, dim) its input,
 * rstd (rows) fp32 as fvqa_rmsnorm_fwd left it; dw (dim) fp32:
 *     dw[c] (+)= sum_r  g[r,c] * round_to<T>(x[r,c] * rstd[r])
 * — the rounding of the normalised value to the storage type T is the forward's own (`.type_as(x) * weight`) and part of
 * the definition (identity in the fp32 build). accumulate != 0: +=, else =. Products and sums are fp32 in one fixed order
 * without atomics: two launches give the same bits. The rows are split into chunks whose partial sums go through
 * `workspace` (>= fvqa_rmsnorm_dw_workspace(rows, dim) bytes, 16-byte aligned, caller-owned, no initial state); a second
 * launch adds the chunks in order. Shapes as fvqa_rmsnorm_bwd: dim % 8 == 0, dim <= 8192 (the workspace query returns 0
 * for a shape the entry refuses). */
size_t fvqa_rmsnorm_dw_workspace(int rows, int dim);
int fvqa_rmsnorm_dw(const void* g, const void* x, const float* rstd, float* dw, void* workspace,
                    size_t workspace_bytes, int rows, int dim, int accumulate, int dtype, void* stream);

/* ---- RoPE on the q and k column blocks of a fused qkv buffer (llama/model.py:61-67,96).
 * qkv is (rows, 3*dim) with q at cols [0,dim), k at [dim,2dim). cos/sin are (S, head_dim/2)
 * fp32 tables (llama/model.py:45-50). inverse != 0 applies the conjugate rotation (backward).
 * In place. */
int fvqa_rope_qk(void* qkv, const float* cos_t, const float* sin_t, int n_seq, int seq_len,
                 int n_heads, int head_dim, int inverse, int dtype, void* stream);

/* ---- SwiGLU (llama/model.py:142). ab is (rows, 2*hidden) in the AB16 layout (top of this file). */
int fvqa_swiglu_fwd(const void* ab, void* z, int rows, int hidden, int dtype, void* stream);
/* dab (rows, 2*hidden) <- d/d(a,b) of silu(a)*b given dz (rows, hidden) */
int fvqa_swiglu_bwd(const void* dz, const void* ab, void* dab, int rows, int hidden, int dtype,
                    void* stream);

/* ---- adapter-gated prefix attention + causal attention (llama/model.py:98-126) --------
 * qkv: (n_seq*S + A, 3*dim) — sequence rows then the A adapter rows (whose k and v column
 * blocks are adapter·Wk^T, adapter·Wv^T, no RoPE). o: (n_seq*S, dim).
 * gate1, gate2: (H) fp32. vstart: (n_seq) int32, -1 ⇒ no gate2 bias for that sequence
 * (the QAV stream, llama/model.py:121-122). lse_a/lse_t: (n_seq, H, S) fp32 log-sum-exp of
 * the adapter softmax and of the causal softmax, saved for the backward. */
/* cos_t/sin_t (both NULL or both given): when given, q and k in `qkv` are the RAW projections and the
 * kernel rotates them on the fly with the tables of fvqa_rope_qk (identical values to the separate
 * pass; llama/model.py:96); only builds for which fvqa_attn_rope_fused(dtype) == 1 accept them. */
int fvqa_attn_rope_fused(int dtype);
/* 1 when the step schedule computes the adapter K/V rows of layer i+1 as the rider of layer i's W1|W3 launch (and layer 0's as
 * a launch of its own before the walk) instead of beside layer i+1's QKV projection: bf16 build with the (s, t) SwiGLU form.
 * fvqa_swiglu_st: 1 unless FVQA_SWIGLU_AB=1 (tuning switch: a, b saved and the full SwiGLU' arithmetic in the W2^T epilogue). */
int fvqa_kv_rider_ahead(int dtype);
int fvqa_swiglu_st(void);
/* 1 when the step schedule (fvqa_layers_forward / _backward) rotates q, k in the QKV projection's epilogue (fvqa_gemm_nt_rope):
 * the arena's qkv rows — the KV cache of the generation path — then hold ROTATED q, k (bf16 MFMA build; FVQA_ROPE_IN_GEMM=0
 * keeps raw q, k rotated inside the attention kernels). */
int fvqa_rope_in_gemm(int dtype);
int fvqa_attn_fwd(const void* qkv, void* o, float* lse_a, float* lse_t, const float* gate1,
                  const float* gate2, const int32_t* vstart, const float* cos_t, const float* sin_t,
                  int n_seq, int seq_len, int n_heads, int head_dim, int adapter_len, int max_feats,
                  int dtype, void* stream);
/* One-query-row attention of the generation path (llama/model.py:428-470 re-runs the whole sequence per new token; this
 * evaluates Attention.forward :87-128 at the new row only). qkv_row (n_seq, 3*dim): RAW q | k | v projections of each
 * sequence's new token, whose position is pos[n] (int64, device). qkv_cache: the layer's (n_seq*S + A, 3*dim) buffer of
 * fvqa_attn_fwd, holding the keys / values of positions < pos[n] and the adapter rows. cache_rotated says what the cache
 * holds: 1 = ROTATED k (the fp32 build; the bf16 build when the QKV projection rotates in its epilogue, fvqa_rope_in_gemm —
 * the default), 0 = RAW k (bf16 build with FVQA_ROPE_IN_GEMM=0, rotated on the fly); the rule for a caller is
 * cache_rotated = !fvqa_attn_rope_fused(dtype) || fvqa_rope_in_gemm(dtype) — passing 0 for a rotated cache would rotate the
 * cached keys twice. The kernel rotates the new q and k with the tables (rounded to the storage type, as the prefill holds
 * them), writes o_row (n_seq, dim) and stores the new token's k (in the cache's convention) and v into cache row
 * n*S + pos[n]. seq_len <= 4096. */
int fvqa_attn_decode(const void* qkv_row, void* qkv_cache, void* o_row, const float* gate1, const float* gate2,
                     const int32_t* vstart, const int64_t* pos, const float* cos_t, const float* sin_t, int n_seq,
                     int seq_len, int n_heads, int head_dim, int adapter_len, int max_feats, int cache_rotated,
                     int dtype, void* stream);
/* fvqa_attn_decode that also reports where each row looked (the same body with one more compile-time switch, csrc/
 * attn_decode_body.h; generate(frame_attention=True)). Operands, limits and errors of fvqa_attn_decode; o_row and the cache stores
 * come out bit for bit as fvqa_attn_decode writes them. In addition mass (n_seq, n_heads, max_feats + 2) fp32 receives, per
 * sequence n and head h, the summary of P_t = the causal softmax over the text keys 0..p, p = pos[n] (the second softmax of
 * Attention.forward, llama/model.py:120, gate2[h] on the window when p >= vs + F; the adapter softmax is not part of it), with
 * vs = vstart[n], F = max_feats:
 *   mass[f]     = P_t[vs + f] for f < F if vs >= 0 and vs + f <= p, else 0;
 *   mass[F]     = sum of P_t[j] over j < vs, j <= p (0 when vs < 0): the weight in front of the window;
 *   mass[F + 1] = sum of P_t[j] over vs + F <= j <= p (vs < 0: the whole row, 1): the weight behind it.
 * The entries sum to 1 up to rounding. Each sum runs in one fixed order (per-thread strides of 256, the wave's butterfly, four
 * wave partials added pairwise), no atomics: two launches give the same bits. The probabilities are the ones the value pass
 * multiplies with (already in LDS): no key is read a second time. mass on a 4-byte boundary; max_feats <= 4096. */
int fvqa_attn_decode_mass(const void* qkv_row, void* qkv_cache, void* o_row, const float* gate1, const float* gate2,
                          const int32_t* vstart, const int64_t* pos, const float* cos_t, const float* sin_t, float* mass,
                          int n_seq, int seq_len, int n_heads, int head_dim, int adapter_len, int max_feats,
                          int cache_rotated, int dtype, void* stream);
/* The same summary for rows that ALREADY sit in an arena a forward left behind (the first generated token is picked from the
 * prefill's logits row prefix - 1, which no decode pass computes). qkv: one layer's (n_seq*S + A, 3*dim) buffer holding the q | k |
 * v thirds of every row, q and k in ONE convention: both rotated (cache_rotated = 1) or both raw (0, rotated here and rounded to
 * the storage type) — the rule of fvqa_attn_decode. Row r (of n_rows) is the query at position pos[r] of sequence seq[r] (int32
 * device arrays; both are clamped into range); it is scored against the keys 0..pos[r] of its sequence, key pos[r] read from the
 * arena as well. gate2 (n_heads), vstart (n_seq). Writes mass (n_rows, n_heads, max_feats + 2) as defined above and NOTHING else:
 * no values are loaded, the arena is read-only. One workgroup per (head, row), fvqa_attn_decode's score pass; no atomics, bitwise
 * repeatable. head_dim 128, seq_len <= 4096, n_rows <= 65535, max_feats <= 4096. */
int fvqa_attn_row_mass(const void* qkv, const int32_t* seq, const int32_t* pos, const float* gate2, const int32_t* vstart,
                       const float* cos_t, const float* sin_t, float* mass, int n_rows, int n_seq, int seq_len, int n_heads,
                       int head_dim, int adapter_len, int max_feats, int cache_rotated, int dtype, void* stream);
/* Attention of the option-scoring path (fvqa/score.py) at the SUFFIX rows: the O answer options of a sample share their prompt,
 * which is run once and left in qkv_cache exactly as fvqa_attn_decode takes it (same cache_rotated rule, adapter rows behind the
 * n_seq*S sequence rows); each option recomputes only its last rows. qkv_suf (n_seq*n_options*suffix_len, 3*dim): RAW q | k | v
 * of suffix row j of option c of sample n — row (n*n_options + c)*suffix_len + j, sequence position start[n] + j. A query row
 * attends to the cache rows [0, start[n]) of its sample, to rows 0..j of its OWN option's suffix (rotated here, rounded to the
 * storage type) and to the adapter keys (own softmax x tanh(gate1)); gate2 is added on the frame keys when the query position is
 * >= vstart[n] + max_feats. start, len: int32 device arrays (n_seq); rows j >= len[n] are padding — never read, their o rows are
 * zeros. Writes o_suf (n_seq*n_options*suffix_len, dim) and NOTHING else: the cache is read-only here. One launch, no atomics,
 * bitwise repeatable. head_dim 128, seq_len <= 4096, suffix_len <= 16. */
int fvqa_attn_suffix(const void* qkv_suf, const void* qkv_cache, void* o_suf, const float* gate1, const float* gate2,
                     const int32_t* vstart, const int32_t* start, const int32_t* len, const float* cos_t,
                     const float* sin_t, int n_seq, int n_options, int suffix_len, int seq_len, int n_heads, int head_dim,
                     int adapter_len, int max_feats, int cache_rotated, int dtype, void* stream);
/* fvqa_attn_suffix that also reports where each suffix row looked (the same kernel template in csrc/score.hip with one more
 * compile-time switch; score_options(frame_attention=True), fvqa/score.py). Operands, limits and errors of fvqa_attn_suffix; o_suf
 * comes out bit for bit as fvqa_attn_suffix writes it. In addition mass (n_seq*n_options*suffix_len, n_heads, max_feats + 2) fp32,
 * row index as o_suf's, receives the summary fvqa_attn_decode_mass defines, of the query row (n, c, j) at p = start[n] + j: P_t =
 * its softmax over the cached prompt keys [0, start[n]) and rows 0..j of its own option (gate2[h] on the window when p >= vs + F;
 * the adapter softmax is not part of it), vs = vstart[n], F = max_feats, and a key at position kpos counts for entry kpos - vs if
 * vs >= 0 and vs <= kpos < vs + F, for entry F if kpos < vs, for entry F + 1 otherwise (vs < 0: every key). The entries of a row
 * sum to 1 up to rounding; the rows j >= len[n] are zeros. The kernel's online softmax keeps no probabilities: the F + 2 entries
 * are running accumulators per query in LDS, rescaled in every key chunk by the factor the output accumulator takes, each chunk's
 * unnormalised weights added in one fixed order (a frame entry meets at most one key per chunk; the two outer sums run over the
 * half wave's butterfly), and multiplied by 1 / the softmax's sum once the last text chunk is in. No atomics, no key is read a
 * second time: two launches give the same bits. mass is required, on a 4-byte boundary. The accumulators take 32 x 72 floats of
 * LDS next to the kernel's 53.4 KiB (62.6 KiB of the 64 KiB a static allocation may take): max_feats <= 64 here, FVQA_ESHAPE
 * beyond. There is no form that writes the cache and the summary. */
int fvqa_attn_suffix_mass(const void* qkv_suf, const void* qkv_cache, void* o_suf, const float* gate1, const float* gate2,
                          const int32_t* vstart, const int32_t* start, const int32_t* len, const float* cos_t,
                          const float* sin_t, int n_seq, int n_options, int suffix_len, int seq_len, int n_heads, int head_dim,
                          int adapter_len, int max_feats, int cache_rotated, int dtype, void* stream, float* mass);
/* fvqa_attn_suffix for ONE continuation per sequence whose rows JOIN the cache (the same kernel template in csrc/score.hip with one
 * more compile-time switch; the draft-and-verify pass of generate(lookahead=T), fvqa_spec_step below). The operands, limits and
 * errors of fvqa_attn_suffix hold with n_options == 1: qkv_suf (n_seq*suffix_len, 3*dim), row n*suffix_len + j at sequence
 * position start[n] + j; o_suf comes out bit for bit as fvqa_attn_suffix writes it. In addition the (head, sample) workgroup
 * stores its head's slice of the rows j < len[n] (len clamped to seq_len - start[n]) into cache row n*seq_len + start[n] + j: k in
 * the cache's convention — rotated at position start[n] + j and rounded to the storage type when cache_rotated is set, the raw
 * bits otherwise —, v as it is: the bits fvqa_attn_decode stores for the same raw row and position. The q third of the cache,
 * the rows j >= len[n], every other row of the cache and the adapter rows are not written. A query never reads a row this launch
 * writes (it reads the cache rows [0, start[n]) and the suffix rows themselves), so rows left behind start[n] by an earlier call —
 * rejected drafts — are overwritten or ignored, never read. */
int fvqa_attn_suffix_append(const void* qkv_suf, void* qkv_cache, void* o_suf, const float* gate1, const float* gate2,
                            const int32_t* vstart, const int32_t* start, const int32_t* len, const float* cos_t,
                            const float* sin_t, int n_seq, int suffix_len, int seq_len, int n_heads, int head_dim,
                            int adapter_len, int max_feats, int cache_rotated, int dtype, void* stream);
/* The per-option reduction of the multiple-choice protocol (reference engine.py:86-93). rowloss: n_rows compact per-row losses
 * (fvqa_ce_fwd); row_map[r] = (n*n_options + c)*(seq_len-1) + t, the entry of individual_losses row r belongs to (< 0: a pad
 * row; each entry listed at most once). Writes individual_losses (n_seq, n_options, seq_len-1) fp32 — zero wherever no row was
 * scored —, per option the sum, the count of entries != 0 (int64; a scored row whose loss is exactly 0 is not counted, a NaN is)
 * and mean = sum / count, and prediction (n_seq) int64 = argmin over options of the mean with torch's rule: the first NaN
 * wins, ties go to the lowest index. Fixed summation order. n_options <= 64. */
int fvqa_option_pick(const float* rowloss, const int32_t* row_map, int n_rows, float* individual_losses,
                     float* option_sum, int64_t* option_count, float* option_mean, int64_t* prediction, int n_seq,
                     int n_options, int seq_len, void* stream);
/* ---- option scoring by all three flipped tasks (fvqa/flipped.py score_flipped; csrc/flipped.hip, the attention in csrc/score.hip) ----
 * fvqa_attn_suffix for suffixes of up to 64 rows (the same kernel template in csrc/score.hip with the tiles on a third grid axis): the operands, semantics and errors of fvqa_attn_suffix with 1 <= suffix_len <= 64.
 * The query at (n, c, j) sits at position start[n] + j; it sees the cache rows [0, start[n]), rows 0..j of its own option and the
 * adapter keys under tanh(gate1). gate2 is added on the frame keys [vs, vs + max_feats), vs = vstart[n], for query positions
 * >= vs + max_feats wherever the window lies — in the cache, across start[n] or inside the suffix (the QAV stream's frame rows
 * follow its answer); vs < 0: no window. Rows j >= len[n] are never loaded and written as zeros. One workgroup per (head, sample,
 * option x tile of 32 queries). Fixed summation order, no atomics: two launches give
 * the same bits. Writes o_suf and nothing else. */
int fvqa_attn_suffix_wide(const void* qkv_suf, const void* qkv_cache, void* o_suf, const float* gate1, const float* gate2,
                          const int32_t* vstart, const int32_t* start, const int32_t* len, const float* cos_t,
                          const float* sin_t, int n_seq, int n_options, int suffix_len, int seq_len, int n_heads, int head_dim,
                          int adapter_len, int max_feats, int cache_rotated, int dtype, void* stream);
/* The inputs of the suffix rows: x (n_seq*n_options*suffix_len, dim) storage type, row r = (n*n_options + c)*suffix_len + j:
 *   j >= len[n]           zeros (a padding row);
 *   slot && slot[r] >= 0  the bits of vf_tok[n, slot[r]] (vf_tok (n_seq, max_feats, dim), storage type): a frame row of the QAV
 *                         stream (llama/model.py:335-336 zeroes the token row and adds the frame token);
 *   else                  emb[ids[r]] (emb (vocab, dim)).
 * ids (rows) int64, slot (rows) int32 or NULL (then vf_tok may be NULL), len (n_seq) int32. dim * element size % 16 == 0. */
int fvqa_suffix_embed(const int64_t* ids, const int32_t* slot, const void* emb, const void* vf_tok, const int32_t* len, void* x,
                      int n_seq, int n_options, int suffix_len, int dim, int vocab, int max_feats, int dtype, void* stream);
/* The pick over the tasks' per-option means. mean_t (n_seq, n_options) fp32 and count_t (n_seq, n_options) int64 for t = vqa,
 * vaq, qav; a task that was not requested passes NULL for both (at least one is given). Writes
 *   total (n_seq, n_options) fp32 = sum over the given tasks of w_t * mean_t, added in the order vqa, vaq, qav to +0, each product
 *       and each sum rounded to fp32 (no fused multiply-add);
 *   prediction (n_seq) int64 = argmin of total over the ELIGIBLE options — those with count_t > 0 for every given task — with
 *       fvqa_option_pick's rule: the first NaN wins, ties go to the lowest index; 0 when no option is eligible;
 *   prediction_t (3, n_seq) int64 = the same argmin of mean_t over the options with count_t > 0 (0 when none; -1 for a task not given);
 *   gold_loss (n_seq, 3) fp32 = mean_t[n, answer[n]] (NaN for a task not given or an answer outside [0, n_options)) when answer
 *       (n_seq) int64 is given; answer and gold_loss are both NULL otherwise.
 * One workgroup per sample; n_options <= 64. */
int fvqa_flipped_pick(const float* mean_vqa, const float* mean_vaq, const float* mean_qav, const int64_t* count_vqa,
                      const int64_t* count_vaq, const int64_t* count_qav, float w_vqa, float w_vaq, float w_qav,
                      const int64_t* answer, float* total, int64_t* prediction, int64_t* prediction_t, float* gold_loss,
                      int n_seq, int n_options, void* stream);
/* ---- exact answer-vocabulary scoring (fvqa/vocab.py score_vocab; the attention in csrc/score.hip, the reduction in csrc/tree.hip) ----
 * The allowed answers of a sample form a trie; its INTERNAL nodes are the suffix rows of the sample, numbered in pre-order (children
 * in ascending token order), the root — whose input is the prompt's last token — first. Limits of a plan: */
#define FVQA_TREE_DEPTH_MAX 31         /* depth of a row (root 0): the ancestors of a tile's first row fit one chunk of 32 keys */
#define FVQA_TREE_ROWS_MAX 4096        /* rows per sample (and members per sample) */
#define FVQA_TREE_TOTAL_ROWS_MAX 65536 /* n_seq * rows of one pass */
/* fvqa_attn_suffix_wide's semantics with ONE change: who sees whom among the suffix rows. qkv_suf (n_seq*rows, 3*dim): RAW q | k | v
 * of row r of sample n — row n*rows + r, sequence position start[n] + depth[n*rows + r]. A query row attends to the cache rows
 * [0, start[n]) of its sample, to the suffix rows that are its ancestors-or-self (rotated here at their own positions, rounded to
 * the storage type) and to the adapter keys (own softmax x tanh(gate1)); gate2 on the frame window, cache_rotated and the output
 * are as the other fvqa_attn_suffix* entries have them. The plan's arrays, int32 on the device:
 *   n_rows (n_seq)           live rows of the sample; rows r >= n_rows[n] are padding — never loaded, their o rows are zeros;
 *   depth, end (n_seq*rows)  end[r] = the exclusive end of r's subtree in pre-order: a is an ancestor-or-self of q iff
 *                            a <= q < end[a];
 *   tile_anc (n_seq * ceil(rows / 32) * 32)  per tile of 32 rows from q0 the proper ancestors of q0, root first (depth[q0] entries
 *                            are read): every ancestor of a row of the tile lies in the tile or in this chain.
 * Every index read from them is clamped (depth to [0, min(31, seq_len - 1 - start[n])], end[r] to [r + 1, n_rows[n]], a chain
 * entry outside [0, q0) is skipped): a wrong plan gives wrong numbers, never an access outside the operands. One workgroup per
 * (head, sample, tile); key chunks: the prompt's, the chain's, the tile's own rows, the adapter's. Fixed summation order, no
 * atomics: two launches give the same bits. Writes o_suf (n_seq*rows, dim) and nothing else. head_dim 128, seq_len <= 4096,
 * rows <= FVQA_TREE_ROWS_MAX, n_seq*rows <= FVQA_TREE_TOTAL_ROWS_MAX. */
int fvqa_attn_suffix_tree(const void* qkv_suf, const void* qkv_cache, void* o_suf, const float* gate1, const float* gate2,
                          const int32_t* vstart, const int32_t* start, const int32_t* n_rows, const int32_t* depth,
                          const int32_t* end, const int32_t* tile_anc, const float* cos_t, const float* sin_t, int n_seq, int rows,
                          int seq_len, int n_heads, int head_dim, int adapter_len, int max_feats, int cache_rotated, int dtype,
                          void* stream);
/* The reduction of the tree pass. An EDGE e of sample n is (edge_parent, edge_token)[n*max_edges + e], e < n_edges[n]: the token
 * that leads from row edge_parent on. A MEMBER m < n_members[n] is the path member_path[(n*max_members + m)*32 ..] of member_len
 * edges (root first, its EOS edge last) and lands in column member_index of the (n_seq, n_columns) outputs (the member's index in
 * the caller's list; each column at most once, in ascending order of m).
 *   edges    (logits given) lp[e] = logits[g - row0][edge_token] - lse[g - row0] for the edges whose parent row g = n*rows +
 *            edge_parent lies in [row0, row0 + n_block_rows): logits (n_block_rows, vocab) fp32 and lse (fvqa_ce_fwd's) are one
 *            block of the head's rows; a launch per block fills edge_lp (n_seq*max_edges) fp32. logits == lse == NULL: edge_lp is
 *            taken as it stands.
 *   members  (reduce != 0, the last launch) sum = lp along the path added in that order in fp32, count (int64) = member_len, mean
 *            = sum / count, log_posterior = sum - logsumexp of the sample's sums; ranking (n_seq, top) int64 = the columns of the
 *            best `top` <= 8 members, best first, by mean (by_mean != 0) or by sum — the larger wins, a NaN beats every number,
 *            equal keys and NaNs go to the lower column; -1 behind the sample's last member —, prediction (n_seq) int64 =
 *            ranking[:, 0]. Columns that are no member's: sum = mean = log_posterior = -inf, count = 0.
 * One workgroup per sample; fixed order, no float atomics: two launches give the same bits. Indices read from the arrays are clamped. */
int fvqa_trie_score(const float* logits, const float* lse, int row0, int n_block_rows, const int32_t* edge_parent,
                    const int32_t* edge_token, const int32_t* n_edges, float* edge_lp, const int32_t* member_path,
                    const int32_t* member_len, const int32_t* member_index, const int32_t* n_members, float* sum, int64_t* count,
                    float* mean, float* log_posterior, int64_t* ranking, int64_t* prediction, int n_seq, int rows, int max_edges,
                    int max_members, int n_columns, int vocab, int top, int by_mean, int reduce, void* stream);
/* The token step of the generation API (csrc/sample.hip; reference llama/generation.py:17-68 and llama/model.py:438-470): one
 * launch per generated token, one workgroup per sequence, between the LM head and the next token's first RMSNorm.
 * In: logits (n_seq, vocab) fp32, finite; u (n_seq) fp32 in [0, 1) (may be NULL when temperature == 0); emb (vocab, dim) in the
 * storage type. In/out: ids (n_seq, seq_len) int64, pos (n_seq) int32 (the position the logits were computed at, >= -1),
 * done (n_seq) int32. Out: x_next (n_seq, dim) storage type, token (n_seq) int32 (-1 where none was picked), n_kept (n_seq)
 * int32, n_active (ONE int32: rows with done == 0 after this step), pos64 (n_seq) int64 or NULL: each row's position after the
 * step, the form fvqa_attn_decode reads. Per row:
 *   - done != 0, or pos + 1 >= seq_len (no room: the row becomes done): ids and pos are not written, n_kept = 0, token = -1,
 *     x_next = the embedding of the row's current token (a valid row: the batch stays rectangular through the layers);
 *   - temperature == 0: token = the index of the largest logit, the lowest index on exact ties; n_kept = 1;
 *   - temperature > 0: p = softmax(logits / temperature) (maximum subtracted, fp32); order by p descending, ties by index
 *     ascending; a token is kept iff the total p in front of it is <= top_p (n_kept of them, kept mass M); token = the first
 *     kept token IN INDEX ORDER whose running kept mass exceeds u * M — the reference's distribution (it draws with
 *     torch.multinomial from the re-normalised kept set);
 *   - then ids[pos + 1] = token, pos += 1, x_next = emb[token]; done = 1 if stop_at_eos and token == eos_id (the EOS is written).
 * Fixed summation orders, no float atomics: bitwise repeatable. n_active is counted through one device-resident ticket word of
 * the library: calls on one device must be ordered against each other (one stream, or events) — nothing enforces it, and two
 * unordered calls corrupt each other's count. Only the last workgroup of a call puts the ticket back to zero: a launch that
 * does not complete (a fault, a reset queue) leaves it non-zero, and every later n_active of that process is wrong until the
 * library is loaded afresh. n_seq <= 65535.
 * FVQA_EINVAL: a null pointer (u only when temperature > 0), temperature < 0 or NaN, top_p outside (0, 1], a bad dtype code;
 * FVQA_ESHAPE: a dimension <= 0. */
int fvqa_decode_next(const float* logits, const float* u, const void* emb, float temperature, float top_p, int eos_id,
                     int stop_at_eos, int64_t* ids, int32_t* pos, int32_t* done, void* x_next, int32_t* token,
                     int32_t* n_kept, int32_t* n_active, int64_t* pos64, int n_seq, int vocab, int dim, int seq_len,
                     int dtype, void* stream);
/* fvqa_decode_next with a repetition penalty, top-k, the picked token's log-probability and a caller-owned ticket word (the
 * same kernel template in csrc/sample.hip; generate(top_k / repetition_penalty / return_logprobs / num_return_sequences)). The
 * operands, the row stepping and the errors of fvqa_decode_next hold; in addition: top_k >= 0 (0, or >= vocab: off),
 * repetition_penalty r >= 1, gen_start (n_seq) int32 in, logprob (n_seq) fp32 out, counter (ONE 32-bit word owned by the
 * caller and zeroed by the caller before the first call, as fvqa_beam_step's: every completed call leaves it zero again; calls
 * that share a counter must be ordered against each other; the library keeps no state for this entry). Per live row, fp32:
 *   1. R = the distinct ids at positions max(gen_start, 0) .. pos of the row's id matrix — the tokens generated so far, NOT the
 *      prompt; ids outside [0, vocab) are ignored; empty when pos < gen_start. l1_i = l_i / r if l_i > 0 else l_i * r for i in
 *      R (once, however often i occurs), l1_i = l_i elsewhere (the CTRL rule). r == 1: l1 is l bit for bit. The logits are read
 *      only.
 *   2. temperature == 0: token = the largest l1_i, lowest index on ties; n_kept = 1; top_k and top_p are ignored.
 *      temperature > 0: e_i = exp((l1_i - max l1) / temperature).
 *   3. Order by e descending, index ascending. k = top_k if 1 <= top_k < vocab, else vocab; Z_k = the mass of the first k
 *      tokens. The token at rank j is kept iff j < k and the mass in front of it is <= top_p * Z_k (n_kept of them: a prefix of
 *      the order). With k == vocab this is fvqa_decode_next's rule, and with r == 1 as well its results bit for bit.
 *   4. token = the first kept token IN INDEX ORDER whose running kept mass exceeds u * M, else the last kept token.
 *   5. logprob = l_token - (m + log(sum exp(l - m))) on the RAW logits (no penalty, temperature 1, no cut; fixed summation
 *      order, the same bits whatever the sampling parameters) — the quantity fvqa_beam_step sums into score. 0 for a row that
 *      picks nothing (token == -1).
 * FVQA_EINVAL also for a null gen_start / logprob / counter, repetition_penalty < 1 or NaN, top_k < 0; FVQA_ESHAPE also for a
 * vocab beyond 1216512 when repetition_penalty != 1 (the bitmap of R lives in LDS). */
int fvqa_decode_next_ex(const float* logits, const float* u, const void* emb, float temperature, float top_p, int top_k,
                        float repetition_penalty, int eos_id, int stop_at_eos, int64_t* ids, int32_t* pos, int32_t* done,
                        const int32_t* gen_start, void* x_next, int32_t* token, int32_t* n_kept, float* logprob,
                        int32_t* n_active, uint32_t* counter, int64_t* pos64, int n_seq, int vocab, int dim, int seq_len,
                        int dtype, void* stream);
/* fvqa_decode_next_ex with three more pick rules (the same kernel template in csrc/sample.hip with one more compile-time switch;
 * generate(min_p / no_repeat_ngram_size / min_new_tokens)). The operands of fvqa_decode_next_ex in its order, then min_p in
 * [0, 1) (0: off), no_repeat_ngram n >= 0 (0: off), min_new_tokens m >= 0 (0: off; m > 0 needs stop_at_eos != 0). The row
 * stepping and the errors of fvqa_decode_next_ex hold. With g0 = max(gen_start, 0), p = pos, the row's generated tokens
 * ids[g0 .. p] and i = p + 1 - gen_start the index of the token being picked, per live row in fp32, in front of rules 1 to 5:
 *   0. The ban set X, built from the row's own ids once per step, before the penalty:
 *      - minimum length: eos_id is in X while i < m;
 *      - n-gram blocking: s = the last n - 1 generated tokens (empty for n == 1; fewer than n - 1 generated: nothing is banned);
 *        for every j with g0 <= j and j + n - 1 <= p and ids[j .. j + n - 2] == s, the token ids[j + n - 1] is in X. Only
 *        generated positions are scanned: a window that reaches into the prompt bans nothing — the prompt lists the answer
 *        options and the answer is meant to copy one (Hugging Face's processor scans the prompt too);
 *      - ids outside [0, vocab) are ignored.
 *      A banned token takes no part anywhere: not in the maximum, Z, the counts and sums of either bisection, the number top-k
 *      is cut against (the tokens NOT banned), the tie groups or the walk; it is never returned and n_kept never counts it; the
 *      greedy pick is the best token that is not banned. The penalty's set R is unaffected, and logprob stays l_token - lse of
 *      the raw, whole row. A row whose every token is banned ends as a trie row at a node without edges does: done, token -1,
 *      n_kept 0, logprob 0; ids and pos are not written.
 *   3'. min-p (ignored at temperature == 0): the largest token that is not banned has e = exp(0) = 1 exactly; a token is kept
 *      iff rule 3 keeps it AND e_i >= min_p, an fp32 comparison on the e_i every other pass sees. That is again a prefix of the
 *      one order (e descending, index ascending) made of whole tie groups, so the kept set is the shortest of three prefixes and
 *      holds the top token. It equals Hugging Face's warpers in sequence (top-k, then top-p, then min-p, each renormalising):
 *      the ratio of a probability to the largest one does not change under renormalisation, and every earlier cut keeps the
 *      largest.
 * min_p == 0, n == 0, m == 0: fvqa_decode_next_ex's results bit for bit. The method: X is a second bitmap of vocab bits in LDS
 * behind R's; min-p is one counting pass behind the nucleus cut. Fixed summation orders, no float atomics: bitwise repeatable.
 * FVQA_EINVAL also for min_p outside [0, 1) or NaN, n < 0, m < 0, m > 0 with stop_at_eos == 0; FVQA_ESHAPE also for a vocab
 * beyond 1216512 (one bitmap: repetition_penalty == 1) or beyond 626688 (both bitmaps: 2 * 4 * ceil(vocab / 32) bytes above
 * 156672). */
int fvqa_decode_next_rules(const float* logits, const float* u, const void* emb, float temperature, float top_p, int top_k,
                           float repetition_penalty, int eos_id, int stop_at_eos, int64_t* ids, int32_t* pos, int32_t* done,
                           const int32_t* gen_start, void* x_next, int32_t* token, int32_t* n_kept, float* logprob,
                           int32_t* n_active, uint32_t* counter, int64_t* pos64, int n_seq, int vocab, int dim, int seq_len,
                           int dtype, void* stream, float min_p, int no_repeat_ngram, int min_new_tokens);
/* A vote over the samples of a prompt (csrc/vote.hip; generate(num_return_sequences=n, vote=True)): self-consistency by exact
 * match of the token rows. In: tokens (n_seq, n_samples, steps) int32, -1 padded; score (n_seq, n_samples) fp32. Out: group and
 * votes (n_seq, n_samples) int32, winner and n_groups (n_seq) int32, share (n_seq) fp32. Per prompt:
 *   - two samples belong to one group iff their token rows are equal in every column, padding included; group[a] = the lowest
 *     sample index of a's group (its representative); votes = the group's size at the representative, 0 elsewhere; n_groups =
 *     the number of representatives;
 *   - winner = the representative with the most votes; ties go to the larger score of the representative (a NaN counts as
 *     -inf), remaining ties to the lower index; share = votes[winner] / n_samples.
 * One workgroup per prompt, integer compares and one float compare in a fixed order: bitwise repeatable.
 * FVQA_EINVAL: a null pointer; FVQA_ESHAPE: n_seq outside [1, 65535], n_samples outside [1, 64], steps < 1, more than 2^31 - 1
 * tokens; FVQA_EALIGN: a pointer off its 4-byte boundary. */
int fvqa_sample_vote(const int32_t* tokens, const float* score, int32_t* group, int32_t* votes, int32_t* winner,
                     int32_t* n_groups, float* share, int n_seq, int n_samples, int steps, void* stream);
/* fvqa_decode_next_ex under a trie of allowed answers (the same kernel template in csrc/sample.hip; generate(constraints=...);
 * fvqa/constrain.py builds the arrays). The operands, the row stepping and the errors of fvqa_decode_next_ex hold; in addition:
 * node (n_seq) int32, in and out — the trie node each row stands at, -1 for an unconstrained row —, and the trie in CSR form,
 * int32 device arrays that are only read: node_first (n_nodes + 1) edge offsets, edge_token (n_edges), edge_child (n_edges);
 * the edges of a node carry distinct tokens in ascending order, so that list order is the index order of rules 3 and 4.
 * Per live row:
 *   - node == -1: fvqa_decode_next_ex's rule, unchanged (every node -1: its results bit for bit).
 *   - 0 <= node < n_nodes: the row's vocabulary is the tokens on the edges of its node; an edge whose token lies outside
 *     [0, vocab) is skipped. Rules 1-4 hold with "every token" read as "every allowed token": the penalty applies to allowed
 *     tokens in R, the maximum that is subtracted is the largest allowed l1, Z sums the allowed e, k = min(top_k, number
 *     allowed) when top_k >= 1, Z_k is the mass of the first k allowed tokens in the order (e descending, token ascending), the
 *     walk runs over the kept tokens in token order, n_kept <= the number allowed. A token that is not allowed is never kept and
 *     never returned — not when it would tie at e == 0 with allowed tokens whose e underflowed, not when u * M rounds up to M
 *     (the last KEPT token is returned), not when top_k exceeds the number allowed (the cut is then off).
 *     Rule 5 is unchanged: logprob is taken on the raw WHOLE row — the model's own log-probability, what fvqa_beam_step sums.
 *     After the pick node = the child of the edge taken.
 *   - a live row whose node has no (usable) edge, or whose node lies outside [-1, n_nodes): picks nothing and becomes done, as
 *     a row with no room does (token -1, n_kept 0, logprob 0; ids, pos and node are not written).
 * A row that picks nothing keeps its node. No index read from the trie leads outside the arrays: an edge range is clamped into
 * [0, n_edges], and a child outside [0, n_nodes) is stored as n_nodes, which ends the row at its next step.
 * The method: the passes of a constrained row run over its node's edge list in place of the vocabulary, with the same fixed
 * summation orders; one launch, no float atomics, the caller-owned ticket word.
 * FVQA_EINVAL also for a null node / node_first / edge_token / edge_child; FVQA_ESHAPE also for n_nodes <= 0 or n_edges < 0;
 * FVQA_EALIGN also for one of them off its 4-byte boundary. */
int fvqa_decode_next_trie(const float* logits, const float* u, const void* emb, float temperature, float top_p, int top_k,
                          float repetition_penalty, int eos_id, int stop_at_eos, int64_t* ids, int32_t* pos, int32_t* done,
                          const int32_t* gen_start, void* x_next, int32_t* token, int32_t* n_kept, float* logprob,
                          int32_t* n_active, uint32_t* counter, int64_t* pos64, int32_t* node, const int32_t* node_first,
                          const int32_t* edge_token, const int32_t* edge_child, int n_nodes, int n_edges, int n_seq, int vocab,
                          int dim, int seq_len, int dtype, void* stream);
/* Contrastive decoding against a twin row (the same kernel template in csrc/sample.hip with one more compile-time switch;
 * generate(contrast=...)): fvqa_decode_next_ex, or with a trie fvqa_decode_next_trie, on PAIRS of rows. n_seq is the number of
 * pairs and the grid is one workgroup per pair. logits, ids, pos, done, pos64 and x_next hold 2 * n_seq rows, row b + n_seq the
 * twin of row b: row b is the positive row (logits l+: the prompt with its clip), row b + n_seq the negative one (l-: the same
 * ids and positions, the twin's features). u, gen_start, token, n_kept, n_plausible, logprob and node hold n_seq entries.
 * node == node_first == edge_token == edge_child == NULL: no trie (n_nodes, n_edges ignored); else all four as in
 * fvqa_decode_next_trie, one node per pair. alpha >= 0, 0 <= beta <= 1. The rule, per pair and token step, fp32, with
 * lp = l - lse(l), lse = m + log(sum exp(l - m)) over the whole raw row as in rule 5:
 *   - plausible set: P = { i allowed : l+_i - max_allowed l+ >= logf(beta) }. beta == 0 keeps everything (logf(0) = -inf),
 *     beta == 1 the maxima only. "Allowed" is the whole vocabulary, or the usable edges of the pair's node.
 *   - contrast: c_i = l+_i + alpha * (lp+_i - lp-_i) for i in P; a token outside P takes no part, as an edge outside [0, vocab)
 *     takes none. This is (1 + alpha) * lp+ - alpha * lp- up to a constant per row, written so that alpha == 0, or twin rows of
 *     the same bits, give c_i = l+_i bit for bit — then, with beta == 0, the positive half of every operand comes out as
 *     fvqa_decode_next_ex / _trie leaves it on the positive rows alone.
 *   - everything downstream sees c where it saw l and P where it saw the allowed tokens: the repetition penalty (rule 1 on c),
 *     the greedy pick with the lowest index on ties, the maximum, e_i, Z, top-k (cut against |P|), the nucleus cut, the walk,
 *     the trie child. n_kept <= n_plausible.
 *   - logprob stays lp+ of the token: the model's own log-probability with the clip, comparable to every other mode.
 *   - pair state: the pair is live iff the positive row is (done == 0 and room for a token): pos and done are READ from the
 *     positive row only. The token, the new pos, done, pos64 and x_next are WRITTEN to both rows (a pair that picks nothing
 *     leaves both id rows alone and gives both rows the positive row's pos, done = 1 and the embedding of the positive row's
 *     current token). R of rule 1 is read from the positive id row. n_active counts pairs, through `counter` as in _ex.
 *   - n_plausible (n_seq) int32 out: |P|, 0 for a pair that picks nothing. A pair whose P is empty (logits that are not
 *     finite) picks nothing and becomes done.
 * No logit is written, every sum keeps a fixed order (two launches give the same bits), LDS holds one row of e_i and the
 * bitmap as before — c is computed where a logit is read —, and when 4 * vocab exceeds the LDS row both rows are re-read per
 * pass. Not built: a contrastive beam step; negatives whose TEXT differs (the pair shares one id row position by position).
 * Errors of fvqa_decode_next_ex (and, with a trie, of _trie) hold; FVQA_EINVAL also for a null n_plausible, alpha < 0 or NaN,
 * beta outside [0, 1] or NaN, a trie given in part; FVQA_ESHAPE also for 2 * n_seq > 65535. */
int fvqa_decode_next_pair(const float* logits, const float* u, const void* emb, float temperature, float top_p, int top_k,
                          float repetition_penalty, float alpha, float beta, int eos_id, int stop_at_eos, int64_t* ids,
                          int32_t* pos, int32_t* done, const int32_t* gen_start, void* x_next, int32_t* token, int32_t* n_kept,
                          int32_t* n_plausible, float* logprob, int32_t* n_active, uint32_t* counter, int64_t* pos64,
                          int32_t* node, const int32_t* node_first, const int32_t* edge_token, const int32_t* edge_child,
                          int n_nodes, int n_edges, int n_seq, int vocab, int dim, int seq_len, int dtype, void* stream);
/* The token step of in-flight batching (the same kernel template in csrc/sample.hip with one more compile-time switch;
 * fvqa/stream.py generate_stream): fvqa_decode_next_ex, or with a trie fvqa_decode_next_trie, on SLOTS that hold requests. The
 * n_seq rows are the slots of the decode batch; the operands, the row stepping, n_active, the caller-owned ticket word and the
 * errors of fvqa_decode_next_ex hold. node == node_first == edge_token == edge_child == NULL: no trie (n_nodes, n_edges
 * ignored); else all four as in fvqa_decode_next_trie, one node per slot. In addition, int32 device arrays: req (n_seq) in — the
 * request each slot holds, -1: none —, budget (n_req) in — the tokens each request may generate —, out_tokens (n_req, width)
 * out, out_logprob (n_req, width) fp32 out or NULL, out_n_generated (n_req) out; u is (width, n_req) fp32: the draws of a
 * request are its own, wherever and whenever it is seated. Per slot b, with r = req[b] and i = pos + 1 - gen_start[b]:
 *   - r outside [0, n_req), or i outside [0, min(budget[r], width)): the slot is not live. It becomes done as a row with no
 *     room does (token -1, n_kept 0, logprob 0, x_next = the embedding of its current token), and nothing of any request's
 *     results is written. An empty slot is done = 1, req = -1, pos = 0 over an all-zero id row: a valid row for the layers.
 *   - otherwise the rule of fvqa_decode_next_ex / _trie picks the token, reading the draw at u[i * n_req + r]; the slot is
 *     stepped as there (token, n_kept and logprob are written per slot as well), and out_tokens[r, i] = token,
 *     out_logprob[r, i] = logprob, out_n_generated[r] = i + 1.
 *   - done = 1 also when i + 1 == budget[r]: the token is still written.
 * Every index read from req, budget and gen_start is range-checked before it is used. With req = 0 .. n_seq - 1, budgets out of
 * reach and width == 1 every operand fvqa_decode_next_ex / _trie writes comes out bit for bit. Two slots must not hold one
 * request. FVQA_EINVAL also for a null req / budget / out_tokens / out_n_generated, a trie given in part; FVQA_ESHAPE also for
 * n_req <= 0 or width <= 0. */
int fvqa_decode_next_stream(const float* logits, const float* u, const void* emb, float temperature, float top_p, int top_k,
                            float repetition_penalty, int eos_id, int stop_at_eos, int64_t* ids, int32_t* pos, int32_t* done,
                            const int32_t* gen_start, void* x_next, int32_t* token, int32_t* n_kept, float* logprob,
                            int32_t* n_active, uint32_t* counter, int64_t* pos64, int32_t* node, const int32_t* node_first,
                            const int32_t* edge_token, const int32_t* edge_child, int n_nodes, int n_edges, const int32_t* req,
                            const int32_t* budget, int n_req, int width, int32_t* out_tokens, float* out_logprob,
                            int32_t* out_n_generated, int n_seq, int vocab, int dim, int seq_len, int dtype, void* stream);
/* Seats prefilled prompts in freed slots of the decode batch (csrc/stream.hip; fvqa/stream.py), one launch per admission, one
 * workgroup per entry. In: slot, src, request (n_admit) int32 — entry j puts row src[j] of the prefill into slot slot[j] for
 * request request[j]; the slots of one call are distinct —; the prefill's prompt_ids (n_src, seq_len) int64, prefix (n_src)
 * int64 (where each answer starts), vstart_src (n_src) int32, logits_src (n_src, seq_len, vocab) fp32, root (n_src) int32 (the
 * trie root of each row) or NULL together with node. In/out, per slot: ids (n_slots, seq_len) int64, pos / done / gen_start /
 * vstart / req / node (n_slots) int32, pos64 (n_slots) int64, lg (n_slots, vocab) fp32. For entry j: ids[slot] =
 * prompt_ids[src], pos = pos64 = prefix - 1, gen_start = prefix, vstart = vstart_src[src], req = request, node = root[src],
 * lg[slot] = logits_src[src, prefix - 1] (the row the first token is picked from), done = 0. prefix < 1 or > seq_len: done = 1,
 * pos = pos64 = gen_start = 0 and lg is left alone — the request ends with zero tokens, as a row with no room.
 * Refused — nothing of the entry is written, bit 0 of err (ONE 32-bit word owned by the caller) is raised —: slot outside
 * [0, n_slots), src outside [0, n_src), a slot that holds a running request (done == 0 and req >= 0). The cached k / v of the
 * prompt are moved by fvqa_kv_beam_move. FVQA_EINVAL: a null pointer (root and node: both or neither); FVQA_ESHAPE: a dimension
 * <= 0, n_admit > n_slots, n_slots > 65535; FVQA_EALIGN: an int64 array off its 8-byte, another off its 4-byte boundary. */
int fvqa_slot_seat(const int32_t* slot, const int32_t* src, const int32_t* request, int n_admit, const int64_t* prompt_ids,
                   const int64_t* prefix, const int32_t* vstart_src, const float* logits_src, const int32_t* root, int n_src,
                   int64_t* ids, int32_t* pos, int64_t* pos64, int32_t* done, int32_t* gen_start, int32_t* vstart, int32_t* req,
                   int32_t* node, float* lg, uint32_t* err, int n_slots, int seq_len, int vocab, void* stream);
/* The token step of draft-and-verify greedy decoding (csrc/spec.hip; generate(lookahead=T); prompt-lookup / assisted generation
 * restricted to greedy): one launch between the LM head and the next pass's first RMSNorm, one 256-thread workgroup per sequence.
 * A pass feeds every sequence up to T = lookahead rows: the last committed token and a DRAFT of the tokens behind it. Every draft
 * token that equals the greedy choice is committed, so the ids are those of fvqa_decode_next at temperature 0, token for token.
 * Per row n, the pass was fed m = len[n] tokens w_0 .. w_{m-1} (1 <= m <= T; len is clamped into that range) at positions
 * q .. q + m - 1, q = pos[n]: w_0 is the last committed token — it is ids[n, q] and is not read from w —, w_1 .. are the drafts,
 * w[n, 1 .. m-1], which are NOT in ids. logits (n_seq*T, vocab) fp32: row n*T + j is L_j, computed at position q + j. (The first
 * step: len = 1 and L_0 = the prefill's row at prefix - 1, as for fvqa_decode_next.) A row is live iff done == 0, pos >= -1,
 * pos + 1 < seq_len and n_generated < max_new_tokens. Per live row:
 *   1. verify: a = the largest value in [0, m - 1] with w_i == argmax L_{i-1} for all 1 <= i <= a; argmax is the first index on
 *      exact ties (fvqa_decode_next's rule). Row L_i is scanned only if the drafts 1 .. i were accepted.
 *   2. commit: the candidates w_1 .. w_a, then the fresh token g = argmax L_a — candidate i is argmax L_{i-1} either way —, in order:
 *      ids[q + i] = candidate_i, pos += 1, n_generated += 1. Committing stops after a committed EOS when stop_at_eos is set, and
 *      when n_generated == max_new_tokens: the row is then done. It also stops when pos + 1 >= seq_len: the row then has m' = 0
 *      and becomes done at its next step, exactly as a full row does under fvqa_decode_next. The log-probability of a committed
 *      token is L[tok] - lse(L) on the raw row it was verified against, lse = max + log(sum exp(l - max)) with the fixed summation
 *      order of rule 5 of fvqa_decode_next_ex (the same bits).
 *   3. draft the next pass, P = pos after the commit: w'_0 = the last committed token; m' = min(T, max_new_tokens - n_generated,
 *      seq_len - 1 - P), 0 for a done row. With m' >= 2:
 *      - draft_tokens != NULL ((n_seq, max_new_tokens) int32, read only): w'_i = draft_tokens[n, n_generated + i - 1] for
 *        i = 1 .. m' - 1; the draft ends in front of the first entry outside [0, vocab) (a -1 ends it).
 *      - draft_tokens == NULL, prompt lookup with G = lookup_ngram, 1 <= G <= 4, over the committed ids[n, 0 .. P]: for g = G down
 *        to 1, e = the largest value with g - 1 <= e < P and ids[e-g+1 .. e] == ids[P-g+1 .. P]; the first g with a match wins
 *        and w'_i = ids[e + i] for i = 1 .. min(m' - 1, P - e); the draft ends in front of the first id outside [0, vocab).
 *      m' becomes 1 + the length of the draft (no match, an empty draft: 1 — a plain token step).
 *   4. outputs: x_next (n_seq*T, dim): row n*T + j = emb[w'_j] for j < m', zeros behind; start[n] = P, len[n] = m', w[n, j] = w'_j
 *      (-1 behind); token / logprob (n_seq, T): the tokens committed by this step in order and their log-probabilities, padded
 *      with -1 / 0; n_committed[n]; n_drafted[n] = m - 1; pos64[n] = P (may be NULL); done.
 * A row that is not live commits nothing and is done afterwards: ids, pos, n_generated and w are not written, token = -1,
 * logprob = 0, n_committed = n_drafted = 0, len = 0, start = pos64 = pos clamped into the sequence, and row n*T of x_next is the
 * embedding of the row's current token (a valid row: the batch stays rectangular; the same holds for a live row with m' = 0).
 * n_active = the rows with done == 0 after the step, counted through `counter` exactly as in fvqa_decode_next_ex (ONE 32-bit
 * word owned and zeroed once by the caller; every completed call leaves it zero; calls that share it must be ordered).
 * With T == 1 (and max_new_tokens never reached) token, ids, pos, pos64, done, x_next and n_active are those of fvqa_decode_next
 * at temperature 0, bit for bit.
 * Rejected drafts leave their k and v in cache rows behind pos; nothing may read them: the next pass reads [0, start) plus its
 * own rows and overwrites from start on (fvqa_attn_suffix_append).
 * No float atomics, fixed summation orders: bitwise repeatable. Every index read from ids or draft_tokens is clamped.
 * Limits: 1 <= lookahead <= 16, n_seq <= 65535, n_seq * lookahead <= 65535 (else FVQA_ESHAPE, as for a dimension <= 0).
 * FVQA_EINVAL: a null pointer (draft_tokens and pos64 may be NULL), a bad dtype code, lookup_ngram outside [1, 4] when
 * draft_tokens is NULL; FVQA_EALIGN: an operand off its element's boundary. */
int fvqa_spec_step(const float* logits, const void* emb, const int32_t* draft_tokens, int lookup_ngram, int eos_id,
                   int stop_at_eos, int max_new_tokens, int64_t* ids, int32_t* pos, int32_t* done, int32_t* n_generated,
                   int32_t* w, int32_t* len, int32_t* start, void* x_next, int32_t* token, float* logprob, int32_t* n_committed,
                   int32_t* n_drafted, int32_t* n_active, uint32_t* counter, int64_t* pos64, int n_seq, int lookahead, int vocab,
                   int dim, int seq_len, int dtype, void* stream);
/* fvqa_spec_step under sampling (the same kernel template in csrc/spec.hip with SAMPLE = true, the pick in csrc/row_sample.h;
 * generate(lookahead=T, temperature > 0)). Every draft of this project is deterministic, a point mass d; speculative sampling
 * then accepts d with probability p(d) and else draws from p with d removed and renormalised — the distribution of drawing
 * t ~ p ONCE with the plain sampler and accepting the draft iff t == d. So the step draws each token with fvqa_decode_next_ex's
 * rule and the draw the plain loop would have used for it, and the ids are those of the plain sampled call, token for token.
 * The operands, the liveness rule, the commit, the next pass's draft, the outputs and the errors of fvqa_spec_step hold; in
 * addition: u (max_new_tokens, n_seq) fp32 in [0, 1) — the plain loop's one array of draws, row t for token index t —,
 * temperature > 0, top_p, top_k, repetition_penalty and gen_start (n_seq) int32 as in fvqa_decode_next_ex, n_kept (n_seq, T) int32
 * out. Per live row, with g0 = n_generated before the step:
 *   1. the pick at row L_i, i = 0, 1, ..: rules 1 to 5 of fvqa_decode_next_ex on the raw row with the draw
 *      u[min(g0 + i, max_new_tokens - 1) * n_seq + n] — the draw belongs to the TOKEN INDEX, not to the step — and with R = the
 *      distinct ids at positions max(gen_start, 0) .. pos of the row INCLUDING the tokens rows 0 .. i - 1 of this step committed
 *      (the bitmap is built once per step and gains one bit per commit). The same summation orders and bisections as
 *      fvqa_decode_next_ex: e_i staged in LDS when 4 * vocab bytes fit, recomputed from the logits when not.
 *   2. verify: the draft w_{i+1} is accepted iff it equals the token sampled at row L_i (a draft outside the kept set has
 *      probability 0 and is never accepted); row L_{i+1} is picked from only then. The token committed at row i is the sampled
 *      one whether it was drafted or not. n_kept[n, i] = the size of the kept set of the i-th commit, 0 behind the commits;
 *      logprob is rule 5's, on the raw row.
 * With T == 1 (and max_new_tokens never reached) token, n_kept, logprob, ids, pos, pos64, done, x_next and n_active are those of
 * fvqa_decode_next_ex with u's row n_generated, bit for bit. No float atomics, fixed summation orders: bitwise repeatable.
 * FVQA_EINVAL also for a null u / gen_start / n_kept, temperature <= 0 or NaN, top_p outside (0, 1], top_k < 0,
 * repetition_penalty < 1 or NaN; FVQA_ESHAPE also for a vocab beyond 1216512 when repetition_penalty != 1 (the bitmap of R
 * lives in LDS); FVQA_EALIGN also for one of the three off its 4-byte boundary. */
int fvqa_spec_step_sample(const float* logits, const float* u, const void* emb, const int32_t* draft_tokens, int lookup_ngram,
                          float temperature, float top_p, int top_k, float repetition_penalty, int eos_id, int stop_at_eos,
                          int max_new_tokens, int64_t* ids, int32_t* pos, int32_t* done, int32_t* n_generated,
                          const int32_t* gen_start, int32_t* w, int32_t* len, int32_t* start, void* x_next, int32_t* token,
                          int32_t* n_kept, float* logprob, int32_t* n_committed, int32_t* n_drafted, int32_t* n_active,
                          uint32_t* counter, int64_t* pos64, int n_seq, int lookahead, int vocab, int dim, int seq_len, int dtype,
                          void* stream);
/* The token step of jump-forward constrained greedy decoding (csrc/jump.hip; generate(constraints=C, jump_forward=T)): one launch
 * where fvqa_spec_step sits, one 256-thread workgroup per sequence. Under the trie of fvqa_decode_next_trie a row whose node has a
 * single edge has nothing to decide, so a step picks ONE token from the logits and then commits the tokens the trie fixes behind
 * it, up to T = jump_forward per step; the next pass feeds all of them, so that their k / v join the cache
 * (fvqa_attn_suffix_append) without a pass of their own. Nothing is drafted and nothing is ever rejected.
 * logits (n_seq*T, vocab) fp32, read only: row n*T + j was computed on the token w[n, j] the previous step committed, of which
 * there were m = len[n] clamped into [1, T]. (The first step: len = 1 and row 0 = the prefill's row at prefix - 1.) The trie: node
 * (n_seq) int32 in and out, node_first / edge_token / edge_child as in fvqa_decode_next_trie; all four NULL: no trie, every row
 * is unconstrained. In/out: ids (n_seq, seq_len) int64, pos, done, n_generated, len (n_seq) int32, w (n_seq, T) int32. Per row n:
 *   1. live iff done == 0, pos >= -1, pos + 1 < seq_len and n_generated < max_new_tokens. A row that is not live commits nothing
 *      and is done afterwards: ids, pos, n_generated, node and w are not written, len = 0, start = pos64 = pos clamped into the
 *      sequence, row n*T of x_next = the embedding of the id at that position clamped into [0, vocab) (a valid row: the batch stays
 *      rectangular), zeros behind, token = -1, the log-probabilities 0, n_committed = 0.
 *   2. pick, on the LAST fed row L = logits[n*T + m - 1]. node == -1: argmax L over the vocabulary, the first index on exact ties
 *      (fvqa_decode_next's rule); no chain follows. node >= 0: the node's edge range clamped into [0, n_edges], edges whose token
 *      lies outside [0, vocab) skipped — no usable edge, or a node outside [0, n_nodes): the row ends, committing nothing, as in 1
 *      except that w becomes -1 —; else the largest logit among the usable edges, the lowest edge on ties, and node = the edge's
 *      child, n_nodes if that lies outside [0, n_nodes): fvqa_decode_next_trie's greedy pick. The token is committed: ids[pos + 1],
 *      pos += 1, n_generated += 1, token[n, 0]; logprob_pick[n] = L[token] - lse(L) over the whole raw row (rule 5 of
 *      fvqa_decode_next_ex, the same bits). The row is done if the token is eos_id or n_generated == max_new_tokens.
 *   3. chain, while the row is not done, fewer than T tokens were committed by this step, pos + 1 < seq_len, n_generated <
 *      max_new_tokens, the node lies inside [0, n_nodes), its clamped edge range holds EXACTLY ONE edge and that edge's token lies
 *      inside [0, vocab): if the token is eos_id and chain_eos == 0, stop in front of it; else commit it as in 2, move to the
 *      (clamped) child, and stop, done, if it was eos_id or the budget is now spent. A node with several edges of which one is
 *      usable is left to the next step's pick: the chain never scans a node.
 *   4. want_logprobs != 0: logprob_fed[n, j] for 1 <= j < m = logits[n*T + j - 1][w[n, j]] - lse of that row, for the INCOMING w
 *      of a row that is live by rule 1 (0 for a w outside [0, vocab)); entry 0 and every other entry 0. With want_logprobs == 0
 *      the whole array is 0 and the rows 0 .. m - 2 of the logits are never read. A caller that wants every token's
 *      log-probability passes chain_eos = 0: a row then ends by PICKING its EOS, at a step that reads what the row still owes.
 *   5. the next pass, nc = the tokens committed by this step: a row that goes on feeds them ALL — w[n, 0 .. nc) (-1 behind),
 *      len = nc, start = pos64 = the position of the first one, x_next rows n*T + j = their embeddings, zeros behind. A row that
 *      is done feeds as in 1: len = 0, start = its position, row n*T = the embedding of its last token. token (n_seq, T) = the
 *      committed tokens, -1 behind; n_committed = nc.
 * n_active = the rows with done == 0 after the step, counted through `counter` exactly as in fvqa_spec_step. pos64 may be NULL.
 * With T == 1 (and max_new_tokens never reached) ids, pos, done, node, token, x_next, pos64, n_active and logprob_pick are those of
 * fvqa_decode_next_trie at temperature 0 and repetition_penalty 1, bit for bit. No float atomics, fixed summation orders: bitwise
 * repeatable. No index read from the trie, ids or w leads outside an array.
 * Limits: 1 <= jump_forward <= 16, n_seq * jump_forward <= 65535, every size > 0, n_nodes > 0 and n_edges >= 0 with a trie (else
 * FVQA_ESHAPE). FVQA_EINVAL: a null pointer (pos64 may be NULL), a bad dtype code, a trie given in part; FVQA_EALIGN: an operand
 * off its element's boundary. */
int fvqa_trie_jump_step(const float* logits, const void* emb, const int32_t* node_first, const int32_t* edge_token,
                        const int32_t* edge_child, int n_nodes, int n_edges, int eos_id, int max_new_tokens, int chain_eos,
                        int want_logprobs, int64_t* ids, int32_t* pos, int32_t* done, int32_t* n_generated, int32_t* node,
                        int32_t* w, int32_t* len, int32_t* start, int64_t* pos64, void* x_next, int32_t* token,
                        float* logprob_pick, float* logprob_fed, int32_t* n_committed, int32_t* n_active, uint32_t* counter,
                        int n_seq, int jump_forward, int vocab, int dim, int seq_len, int dtype, void* stream);
/* The token step of TREE-shaped draft verification (csrc/treespec.hip; generate(lookahead=R, draft_answers=C)): one launch where
 * fvqa_spec_step sits, one 256-thread workgroup per sequence. The likely answers of a sample are a trie; its internal nodes in
 * pre-order (children in ascending token order; fvqa/vocab.py _plan_one) are the sample's PLAN, read only, int32: plan_n (the
 * rows of the plan), plan_token (a row's input token; the root's is not read), plan_depth, plan_end (the exclusive end of the
 * row's subtree: the subtree of g is the contiguous range [g, end[g]), and any prefix of it is closed under ancestors — the whole
 * design rests on that) and plan_parent, each (.., plan_rows). plan_stride is the sample stride of the four tables in elements:
 * 0 — ONE plan shared by every sequence, plan_n one word — or plan_rows — a plan per sequence, plan_n (n_seq). The trie is a
 * DRAFT, not a rule: the tokens committed are the plain greedy call's whatever the plan holds.
 * State per sequence, in and out: fvqa_spec_step's ids (n_seq, seq_len) int64, pos, done, n_generated, len (n_seq) int32 and
 * node (n_seq) int32: >= 0 the plan row whose input token is the last committed token (0 before the first step: the root, whose
 * input is the prompt's last token), -1 once the row has left the trie (a value outside [0, plan_n) reads as -1).
 * The incoming pass fed m = len[n] rows (clamped into [1, rows_in] and to the plan's end; 1 when node == -1): local row j is plan
 * row a + j, a the incoming node, at position q + depth[a + j] - depth[a], q = pos[n]; logits (n_seq*rows_in, vocab) fp32, row
 * n*rows_in + j. (The first step: len = 1 and row 0 = the prefill's row at prefix - 1.) A row is live under fvqa_spec_step's
 * condition. Per live row:
 *   1. walk, from j = 0: g = argmax L_j, the first index on exact ties; it is committed — ids[pos + 1] = g, pos += 1,
 *      n_generated += 1 — and j is the next entry of path. The row is done if stop_at_eos and g == eos_id, or if n_generated ==
 *      max_new_tokens; the walk also stops if pos + 1 >= seq_len (fvqa_spec_step's rule: m' = 0, done at the next step). In these
 *      three cases node becomes -1. Otherwise, with a >= 0, the child c of plan row G = a + j under g is the lowest row r in
 *      (G, min(end[G], plan_n)) with parent[r] == G and token[r] == g — on a sound plan the one the chain G + 1, end[G + 1], ...
 *      reaches; the workgroup looks at the rows side by side. None: node = -1, stop. Found: node = c; if c - a < m (the child was
 *      fed in this pass) and fewer than 32 tokens were committed, j = c - a and the walk goes on; else it stops: the child had been
 *      cut from the pass and is the next pass's root. Row L_j is scanned only if the walk reaches it. The log-probability of a
 *      committed token is L_j[g] - lse(L_j) in fvqa_spec_step's summation order (the same bits).
 *   2. the next pass, P = pos after the commit: Dmax = min(31, max_new_tokens - n_generated - 1, seq_len - 2 - P). A done row or
 *      Dmax < 0: m' = 0, as fvqa_spec_step has it. node == -1: m' = 1. Otherwise the plan rows [node, e), e = min(end[node], node +
 *      rows_out, plan_n), cut in front of the first row whose depth exceeds depth[node] + Dmax; m' = e - node >= 1.
 *   3. outputs. x_next (n_seq*rows_out, dim): row 0 = emb[last committed token], row j >= 1 = emb[token[node + j]] (clamped into
 *      the vocabulary), zeros behind m'. fvqa_attn_suffix_tree's operands for that pass: len[n] = m' (its n_rows), start[n] =
 *      pos64[n] = P, depth / end (n_seq*rows_out) — depth[node + j] - depth[node] clamped into [0, 31], end[node + j] - node
 *      clamped into [j + 1, m']; padding rows depth 0, end j + 1 —, tile_anc (n_seq * ceil(rows_out / 32) * 32): per tile the proper
 *      ancestors of its first row, root first, found by walking `parent` from that row for as many steps as its local depth (a
 *      parent outside [node, child) ends the walk), -1 elsewhere. For fvqa_kv_tree_commit: path (n_seq, 32) the local rows the
 *      walk took (0 behind), n_path = n_committed, start_old = the incoming pos clamped into the sequence (local row path[i] sat
 *      at start_old + i). token / logprob (n_seq, 32): the committed tokens and their log-probabilities, -1 / 0 behind;
 *      n_committed; n_drafted = m - 1; done.
 *   4. A row that is not live behaves as in fvqa_spec_step: nothing of its state is written but done = 1, len = 0, start = pos64
 *      = pos clamped; n_path = n_committed = n_drafted = 0, row n*rows_out of x_next is the embedding of its current token.
 * n_active = the rows with done == 0 after the step, n_on_trie = those of them with node >= 0 (it never rises: a node >= 0 can
 * only turn into -1), counted as fvqa_spec_step counts through TWO consecutive 32-bit words at `counter`, owned and zeroed once by
 * the caller: word 0 for n_active, word 1 for n_on_trie; calls that share them must be ordered.
 * With rows_in == rows_out == 1 (and max_new_tokens never reached) token, ids, pos, pos64, done, x_next and n_active are those of
 * fvqa_decode_next at temperature 0, bit for bit. No float atomics, fixed summation orders: bitwise repeatable. Every index read
 * from the plan, node or ids is clamped: a broken plan gives wrong drafts — which still give greedy's tokens — and never an
 * access outside an operand.
 * Limits: 1 <= rows_in, rows_out <= 64, n_seq * rows <= 65535, plan_rows >= 1, plan_stride 0 or plan_rows (else FVQA_ESHAPE).
 * FVQA_EINVAL: a null pointer (pos64 may be NULL), a bad dtype code; FVQA_EALIGN: an operand off its element's boundary. */
int fvqa_tree_spec_step(const float* logits, const void* emb, const int32_t* plan_n, const int32_t* plan_token,
                        const int32_t* plan_depth, const int32_t* plan_end, const int32_t* plan_parent, int plan_rows,
                        int plan_stride, int eos_id, int stop_at_eos, int max_new_tokens, int64_t* ids, int32_t* pos,
                        int32_t* done, int32_t* n_generated, int32_t* node, int32_t* len, int32_t* start, void* x_next,
                        int32_t* depth, int32_t* end, int32_t* tile_anc, int32_t* path, int32_t* n_path, int32_t* start_old,
                        int32_t* token, float* logprob, int32_t* n_committed, int32_t* n_drafted, int32_t* n_active,
                        int32_t* n_on_trie, uint32_t* counter, int64_t* pos64, int n_seq, int rows_in, int rows_out, int vocab,
                        int dim, int seq_len, int dtype, void* stream);
/* fvqa_tree_spec_step under sampling (the same kernel template in csrc/treespec.hip with SAMPLE = true;
 * generate(lookahead=R, draft_answers=C, temperature > 0)): what fvqa_spec_step_sample is to fvqa_spec_step. The operands, the
 * walk, the cut, the outputs and the errors of fvqa_tree_spec_step hold with "g = argmax L_j" read as "g = the token sampled at
 * L_j": the i-th commit of a step (i = 0, 1, .., at most 32) is rules 1 to 5 of fvqa_decode_next_ex on the raw row the walk
 * stands at, with the draw u[min(g0 + i, max_new_tokens - 1) * n_seq + n], g0 = n_generated before the step, and with R including
 * the step's earlier commits; the walk moves to the child under the SAMPLED token, so the ids are those of the plain sampled call
 * whatever the plan holds. In addition to fvqa_tree_spec_step's operands: u (max_new_tokens, n_seq) fp32, temperature > 0, top_p,
 * top_k, repetition_penalty, gen_start (n_seq) int32, n_kept (n_seq, 32) int32 out (0 behind the commits).
 * With rows_in == rows_out == 1, or every node -1, (and max_new_tokens never reached) token, n_kept, logprob, ids, pos, pos64,
 * done, x_next and n_active are those of fvqa_decode_next_ex, bit for bit. Bitwise repeatable.
 * The additional errors are fvqa_spec_step_sample's. */
int fvqa_tree_spec_step_sample(const float* logits, const float* u, const void* emb, const int32_t* plan_n,
                               const int32_t* plan_token, const int32_t* plan_depth, const int32_t* plan_end,
                               const int32_t* plan_parent, int plan_rows, int plan_stride, float temperature, float top_p,
                               int top_k, float repetition_penalty, int eos_id, int stop_at_eos, int max_new_tokens, int64_t* ids,
                               int32_t* pos, int32_t* done, int32_t* n_generated, const int32_t* gen_start, int32_t* node,
                               int32_t* len, int32_t* start, void* x_next, int32_t* depth, int32_t* end, int32_t* tile_anc,
                               int32_t* path, int32_t* n_path, int32_t* start_old, int32_t* token, int32_t* n_kept, float* logprob,
                               int32_t* n_committed, int32_t* n_drafted, int32_t* n_active, int32_t* n_on_trie, uint32_t* counter,
                               int64_t* pos64, int n_seq, int rows_in, int rows_out, int vocab, int dim, int seq_len, int dtype,
                               void* stream);
/* The cache append of the accepted path (csrc/treespec.hip). fvqa_attn_suffix_tree writes nothing but o — siblings share a
 * position, so a tree pass must not write its rows into the cache —; the pass keeps every layer's RAW q | k | v rows instead:
 * qkv_rows (n_layers, n_seq*rows, 3*dim). After the token step ONE launch over all layers copies, for sequence n and i <
 * n_path[n] (at most 32), the k and v thirds of row n*rows + path[n*32 + i] to row n*seq_len + start_old[n] + i of every layer of
 * qkv_cache (n_layers, n_seq*seq_len + adapter_len, 3*dim: fvqa_kv_beam_move's layout). k follows the cache's convention: with
 * cache_rotated != 0 rotated at position start_old[n] + i and rounded to the storage type — the operations fvqa_attn_suffix_append
 * performs, contraction off: the same bits —, raw otherwise; v as it is. Nothing else is written: not the rows behind n_path, the
 * q third, other sequences or the adapter rows. An entry with path outside [0, rows) or a position outside [0, seq_len) appends
 * nothing. 16-byte accesses. head_dim 128, rows <= 64, n_seq, n_layers <= 65535 (else FVQA_ESHAPE); FVQA_EINVAL: a null pointer
 * (cos_t / sin_t only when cache_rotated), qkv_cache == qkv_rows, a bad dtype code; FVQA_EALIGN: the buffers off a 16-byte
 * boundary, the tables off 4. */
int fvqa_kv_tree_commit(void* qkv_cache, const void* qkv_rows, const int32_t* path, const int32_t* n_path,
                        const int32_t* start_old, const float* cos_t, const float* sin_t, int n_seq, int rows, int seq_len,
                        int n_heads, int head_dim, int adapter_len, int n_layers, int cache_rotated, int dtype, void* stream);
/* One step of beam search (csrc/beam.hip; generate(num_beams > 1)): one launch per token where fvqa_decode_next sits in the greedy
 * loop, one workgroup per SAMPLE. A sample owns n_beams = K consecutive slots (rows b*K .. b*K + K-1 of every operand).
 * In: logits (n_samples*K, vocab) fp32 at each slot's position; emb (vocab, dim) storage type; ids_in (n_samples*K, seq_len)
 * int64. In/out, per slot: pos int32, score fp32 (the sum of the log-probabilities of the generated tokens; -inf: an empty slot),
 * done int32, n_generated int32. Out: ids_out (same shape as ids_in and NOT the same buffer: the caller ping-pongs the two),
 * pos64 int64 (pos after the step, clamped into the sequence: what fvqa_attn_decode reads), parent int32 (the slot of the SAME
 * sample each new slot descends from), token int32 (-1: carried without a token), x_next (n_samples*K, dim), n_active (ONE int32).
 * The rule, per sample: a slot with done != 0 — or with pos + 1 >= seq_len, which makes it done first — offers ONE candidate
 * (j, none) of value score[j]; a live slot j offers (j, v) of value score[j] + (l[j,v] - lse[j]) for every token v, lse[j] =
 * m + log(sum exp(l - m)) in fp32 with a fixed summation order. The new slots 0..K-1 are the K best candidates in the order
 * (value descending, parent ascending, token ascending). A child copies its parent's id row, writes v at pos + 1, advances, takes
 * the value as its score, counts one more generated token, and is done iff stop_at_eos and v == eos_id; a carried candidate is a
 * copy of slot j. x_next = emb[v], for a carried slot the embedding of its current token. No sort, no float atomics: bitwise
 * repeatable. n_active = the number of samples whose new slot 0 is not done (count_any_live == 0: with scores that only fall and
 * ties going to the lower parent nothing can overtake a finished slot 0) or that have any slot not done (count_any_live != 0).
 * It is counted through `counter`, ONE 32-bit word owned by the caller and zeroed by the caller before the first call; every
 * completed call leaves it zero again. Calls that share a counter must be ordered against each other.
 * Limits: 1 <= n_beams <= 8, n_beams <= vocab, n_beams * vocab < 2^31, n_samples <= 65535 (else FVQA_ESHAPE).
 * FVQA_EINVAL: a null pointer, ids_in == ids_out, a bad dtype code. */
int fvqa_beam_step(const float* logits, const void* emb, int eos_id, int stop_at_eos, int count_any_live,
                   const int64_t* ids_in, int64_t* ids_out, int32_t* pos, float* score, int32_t* done, int32_t* n_generated,
                   int64_t* pos64, int32_t* parent, int32_t* token, void* x_next, int32_t* n_active, uint32_t* counter,
                   int n_samples, int n_beams, int vocab, int dim, int seq_len, int dtype, void* stream);
/* fvqa_beam_step under a trie of allowed answers (the same kernel template in csrc/beam.hip; generate(num_beams > 1,
 * constraints=...)). The operands, limits and errors of fvqa_beam_step hold; in addition node (n_samples*K) int32, in and out,
 * per slot, and the trie of fvqa_decode_next_trie. The rule of fvqa_beam_step with these changes:
 *   - a live slot j at a node in [0, n_nodes) offers (j, v) only for the tokens v on the edges of its node (tokens outside
 *     [0, vocab) skipped), of value score[j] + (l[j,v] - lse[j]); lse is over the whole raw row, unchanged;
 *   - a slot with node == -1 offers every v;
 *   - a done slot, a slot with no room, and a live slot whose node has no usable edge or lies outside [-1, n_nodes) — which
 *     becomes done first — each offer their one carried candidate;
 *   - slots with score -inf offer their allowed tokens at -inf, as they offer everything in fvqa_beam_step;
 *   - a new slot takes the child of the edge (parent, token) it was made from, a carried slot keeps its parent's node; all K old
 *     nodes are read before any is written. A child outside [0, n_nodes) is stored as n_nodes (the slot is done at its next step).
 * The order (value descending, parent ascending, token ascending), the count and everything else are fvqa_beam_step's; with
 * every node -1 its results bit for bit.
 * FVQA_EINVAL also for a null node / node_first / edge_token / edge_child; FVQA_ESHAPE also for n_nodes <= 0 or n_edges < 0;
 * FVQA_EALIGN also for one of them off its 4-byte boundary. */
int fvqa_beam_step_trie(const float* logits, const void* emb, int eos_id, int stop_at_eos, int count_any_live,
                        const int64_t* ids_in, int64_t* ids_out, int32_t* pos, float* score, int32_t* done,
                        int32_t* n_generated, int64_t* pos64, int32_t* parent, int32_t* token, void* x_next, int32_t* n_active,
                        uint32_t* counter, int32_t* node, const int32_t* node_first, const int32_t* edge_token,
                        const int32_t* edge_child, int n_nodes, int n_edges, int n_samples, int n_beams, int vocab, int dim,
                        int seq_len, int dtype, void* stream);
/* Cached keys and values follow the beams (csrc/beam.hip). dst: (n_layers, n_dst_seq*seq_len + adapter_len, 3*dim), src:
 * (n_layers, n_src_seq*seq_len + adapter_len, 3*dim) — the layout fvqa_attn_decode takes, every layer, uniform layer stride.
 * For destination sequence n, the k and v thirds of rows [lo[n], hi[n]) (clamped to [0, seq_len)) are copied from source sequence
 * s = src_seq[n] (group == 0) or (n / group) * group + src_seq[n] (group > 0: src_seq holds the slot within the sample, as
 * fvqa_beam_step writes `parent`); an s outside [0, n_src_seq) moves nothing. src_seq, lo, hi: int32 device arrays (n_dst_seq) —
 * read on the device, the host never waits for them. The q third and every row outside the ranges are not written.
 *   scratch == NULL: dst != src (FVQA_EINVAL otherwise). One launch; the adapter_len adapter rows behind the sequence rows are
 *     copied too (k and v thirds). The fan-out of a prefill at n_src_seq sequences into a cache of n_dst_seq.
 *   scratch != NULL: the move inside one cache (dst == src allowed; n_dst_seq == n_src_seq). Sequences with s == n are skipped;
 *     the others go through the window — launch 1 gathers every moved row into scratch, launch 2 scatters them —, so cycles among
 *     the parents (a swap, a 3-cycle) come out right. hi[n] - lo[n] <= window_rows is the caller's contract (rows beyond the
 *     window are not moved); scratch_bytes >= fvqa_kv_beam_move_scratch(n_dst_seq, window_rows, dim, n_layers, dtype), else
 *     FVQA_EALIGN. Adapter rows are not touched.
 * dim * element size must be a multiple of 16 and the buffers 16-byte aligned. n_dst_seq, n_layers <= 65535. */
size_t fvqa_kv_beam_move_scratch(int n_seq, int window_rows, int dim, int n_layers, int dtype);
int fvqa_kv_beam_move(void* dst, const void* src, void* scratch, size_t scratch_bytes, const int32_t* src_seq,
                      const int32_t* lo, const int32_t* hi, int n_dst_seq, int n_src_seq, int group, int seq_len, int dim,
                      int n_layers, int adapter_len, int window_rows, int dtype, void* stream);
/* workspace bytes fvqa_attn_bwd needs (fp32 partials for the batch-summed adapter k/v
 * gradients and the per-head gate sums). Its FIRST 1024 BYTES are integer arrival counters of the
 * fused bf16 backward: the caller zeroes them once after allocating the workspace; every call
 * leaves them zero again. One workspace serves one stream at a time. */
size_t fvqa_attn_bwd_workspace(int n_seq, int seq_len, int n_heads, int head_dim, int adapter_len);
/* dqkv: (n_seq*S + A, 3*dim): dq,dk,dv for sequence rows; adapter rows get [0, dK_a, dV_a] summed over
 * sequences. With cos_t/sin_t == NULL, qkv holds rotated q,k and dq,dk come out NOT yet un-rotated
 * (fvqa_rope_qk inverse follows); with the tables, qkv is raw and dq,dk are gradients of the raw
 * projections. dgate1/dgate2 (H) fp32 are ACCUMULATED (+=). */
int fvqa_attn_bwd(const void* d_o, const void* qkv, const void* o, const float* lse_a,
                  const float* lse_t, const float* gate1, const float* gate2, const int32_t* vstart,
                  const float* cos_t, const float* sin_t,
                  void* dqkv, float* dgate1, float* dgate2, void* workspace, size_t workspace_bytes,
                  int n_seq, int seq_len, int n_heads, int head_dim, int adapter_len, int max_feats,
                  int dtype, void* stream);
/* As fvqa_attn_bwd with tables, for a `qkv` whose q, k fvqa_gemm_nt_rope has ALREADY rotated: nothing is rotated on load, dq and
 * dk are conjugate-rotated at the store, so dqkv holds the gradients of the RAW projections (bf16 MFMA build only). */
int fvqa_attn_bwd_rotated(const void* d_o, const void* qkv, const void* o, const float* lse_a,
                  const float* lse_t, const float* gate1, const float* gate2, const int32_t* vstart,
                  const float* cos_t, const float* sin_t,
                  void* dqkv, float* dgate1, float* dgate2, void* workspace, size_t workspace_bytes,
                  int n_seq, int seq_len, int n_heads, int head_dim, int adapter_len, int max_feats,
                  int dtype, void* stream);

/* ---- visual projection + temporal embedding (llama/model.py:322,324) ------------------
 * vf_raw[b,f,:] = video[b,f,:]·W^T (fp32, kept for the QAV head); vf_tok = storage-dtype
 * cast of vf_raw + temporal[f,:]. video (BF, in_dim) fp32, W (dim, in_dim) fp32, in_dim <= 2048.
 * The launch of fvqa_av_proj_fwd on one contiguous source (both pitches = in_dim), no bias. */
int fvqa_visual_proj_fwd(const float* video, const float* W, const float* temporal, float* vf_raw,
                         void* vf_tok, int n_frames_total, int max_feats, int in_dim, int dim,
                         int dtype, void* stream);
/* d_tok (BF,dim) fp32: gradient wrt the spliced frame tokens (fvqa_splice_bwd); d_qav (BF,dim)
 * fp32 or NULL: extra gradient wrt vf_raw from the QAV head.
 * dW (dim,in_dim) += (d_tok + d_qav)^T·video ; dtemporal (F,dim) += sum_b d_tok[b].
 * The launches of fvqa_av_proj_bwd on one contiguous source. */
int fvqa_visual_proj_bwd(const float* d_tok, const float* d_qav, const float* video, float* dW,
                         float* dtemporal, int n_frames_total, int max_feats, int in_dim, int dim,
                         void* stream);

/* ---- audio-visual front end (llama/model.py:209-227,306-324: --audio with concat / sum / attention / audio_only) ------
 * One source of a projection: x (rows, k) fp32 with row pitch ldx, against k columns of a weight w (dim rows) with row pitch
 * ldw. Every pointer 16-byte aligned, k % 4 == 0, pitches % 4 == 0. */
typedef struct fvqa_proj_src {
  const float* x;
  const float* w; /* forward: the weight's column range; backward: the same range of the weight GRADIENT (written) */
  int32_t ldx, ldw, k, reserved_;
} fvqa_proj_src;
/* out_raw (rows, dim) fp32 = sum_s x_s·w_s^T (+ bias (dim) or NULL), n_src = 1 or 2 — `concat`: two sources against two
 * column ranges of one weight; `sum`: two weights; `audio_only` and the projections of `attention`: one. temporal (F, dim)
 * and out_tok (rows, dim, storage dtype) = cast(out_raw + temporal[r % F]) both given or both NULL. Exact-fp32 matrix
 * cores for rows <= 128 and k % 64 == 0 (one launch), a wave-per-feature kernel otherwise; fixed order, bitwise repeatable. */
int fvqa_av_proj_fwd(const fvqa_proj_src* src, int n_src, const float* bias, const float* temporal, float* out_raw,
                     void* out_tok, int rows, int max_feats, int dim, int dtype, void* stream);
/* x (n_samples*n_query, dim) fp32 = softmax_t(q·k_t * scale)·v over the n_key <= 16 keys of the same sample, maximum
 * subtracted (llama/model.py:153-169); q (n_samples*n_query, dim | ldq), k, v (n_samples*n_key, dim | ldk, ldv). Its backward
 * (--train_audio) is fvqa_av_cross_attn_bwd. */
int fvqa_av_cross_attn_fwd(const float* q, const float* k, const float* v, float* x, int n_samples, int n_query,
                           int n_key, int dim, int ldq, int ldk, int ldv, float scale, void* stream);
/* dW_s (dim, k_s | ldw) += (d_tok + d_qav)^T·x_s for each of n_src = 0..2 TRAINABLE sources (src[s].w = where the source's
 * columns start in the weight gradient, k_s <= 2048), dtemporal (F, dim) += sum_b d_tok[b] as fvqa_visual_proj_bwd. */
int fvqa_av_proj_bwd(const float* d_tok, const float* d_qav, const fvqa_proj_src* src, int n_src, float* dtemporal,
                     int rows, int max_feats, int dim, void* stream);
/* --train_audio: the backward of the audio half of the front end. Same contract as the entries above: exact fp32, fixed
 * summation order, no float atomics, bitwise repeatable, operands checked before any launch.
 * Backward of fvqa_av_cross_attn_fwd with the forward's operands and pitches (k and v may lie side by side in one buffer) and
 * dx (n_samples*n_query, dim): dq (.., dim | lddq), dk, dv (n_samples*n_key, dim | lddk, lddv) are WRITTEN (dk | dv may share
 * one pitched buffer). The softmax is recomputed, maximum subtracted: dv_t = sum_f P_ft dx_f, dP_ft = dx_f·v_t,
 * dS = P o (dP - sum_t P dP), dq_f = scale sum_t dS_ft k_t, dk_t = scale sum_f dS_ft q_f. n_key <= 16, any n_query; one
 * workgroup per sample. With one key, dq and dk are exact zeros. */
int fvqa_av_cross_attn_bwd(const float* q, const float* k, const float* v, const float* dx, float* dq, float* dk, float* dv,
                           int n_samples, int n_query, int n_key, int dim, int ldq, int ldk, int ldv, int lddq, int lddk,
                           int lddv, float scale, void* stream);
/* Input gradient of a projection: dx (rows, k | lddx) = (g0 + g1)·w, g0 and g1 (rows, dim | ldg) fp32 (g1 or NULL), w (dim, k |
 * ldw) — a weight or a column range of one. Written. dim % 64 == 0 (the exact-fp32 matrix cores, 16 rows x 16 columns per workgroup). */
int fvqa_av_proj_dx(const float* g0, const float* g1, const float* w, float* dx, int rows, int dim, int k, int ldg, int ldw,
                    int lddx, void* stream);
/* Weight (+ bias) gradient of a linear layer: dW_s (dim, k_s | ldw) += g^T·x_s for each of n_src = 1..2 sources, g (rows, dim |
 * ldg) — fvqa_av_proj_bwd's kernel and launches for a general, pitched g; dbias (dim) += sum_rows g, or NULL. */
int fvqa_av_linear_bwd(const float* g, int ldg, const fvqa_proj_src* src, int n_src, float* dbias, int rows, int dim,
                       void* stream);

/* ---- token embedding gather + frame splice (llama/model.py:286-294,326-336) -----------
 * h[n,s,:] = emb[ids[n,s]] (zeroed where zero_labels[n,s] >= 0; NULL = never) then
 * mode 0 (vqa/vaq): rows [vstart, vstart+F) := vf_tok[n]           (slice assign, :327,:332)
 * mode 1 (qav):     h[n, index[n,f], :] += vf_tok[n,f]              (scatter_add_, :335-336) */
int fvqa_embed_splice(const int64_t* ids, const void* emb, const void* vf_tok,
                      const int64_t* zero_labels, const int64_t* index, void* h, int n_seq,
                      int seq_len, int dim, int max_feats, int vstart, int mode, int dtype,
                      void* stream);
/* d_tok[n,f,:] += dh[n, row(n,f), :] (fp32 accumulate); row = vstart+f (mode 0) or index[n,f] */
int fvqa_splice_bwd(const void* dh, const int64_t* index, float* d_tok, int n_seq, int seq_len,
                    int dim, int max_feats, int vstart, int mode, int dtype, void* stream);

/* ---- LM-head cross-entropy (llama/model.py:233-234,349-350,355-356) --------------------
 * logits (n_seq, S, V) fp32; labels (n_seq, S) int64 — row (n,s) for s < S-1 is scored
 * against labels[n, s+1]; ignore_index rows are skipped; mean over valid rows.
 * loss_sum[0] += sum of row losses, loss_sum[1] += number of valid rows (fp32, zero it first).
 * lse, rowloss (n_seq*S) receive each scored row's log-sum-exp and loss (fixed-order sum). */
int fvqa_ce_fwd(const float* logits, const int64_t* labels, float* lse, float* rowloss,
                float* loss_sum, int n_seq, int seq_len, int vocab, int64_t ignore_index,
                void* stream);
/* dlogits (n_seq,S,V) storage dtype = (softmax - onehot) * gscale[0] / n_valid on valid rows,
 * 0 elsewhere (including s = S-1). gscale: device fp32 scalar (upstream grad of the loss). */
int fvqa_ce_bwd(const float* logits, const int64_t* labels, const float* lse, const float* loss_sum,
                const float* gscale, void* dlogits, int n_seq, int seq_len, int vocab,
                int64_t ignore_index, int dtype, void* stream);

/* ---- QAV head (llama/model.py:359-361): logits[n,s,f] = xn[n,s,:]·vf_raw[n,f,:]/tau for
 * s < S-1, CE(ignore_index=-1) against labels[n,s+1]. xn has storage dtype.
 * probs (n_seq,S,F) fp32 scratch keeps the softmax for the backward. */
int fvqa_qav_head_fwd(const void* xn, const float* vf_raw, const int64_t* labels, float* probs,
                      float* rowloss, float* loss_sum, int n_seq, int seq_len, int dim,
                      int max_feats, float tau, int dtype, void* stream);
/* dxn (storage dtype, fully written) and d_raw (n_seq,F,dim) fp32 (+=) */
int fvqa_qav_head_bwd(const void* xn, const float* vf_raw, const int64_t* labels, const float* probs,
                      const float* loss_sum, const float* gscale, void* dxn, float* d_raw, int n_seq,
                      int seq_len, int dim, int max_feats, float tau, int dtype, void* stream);

/* ---- loss-scaler + grad-norm + AdamW (util/misc.py:259-273,282-294; train.py:120-121) --
 * One flat fp32 buffer holds every trainable gradient; seg_off (n_seg+1) int64 marks the
 * per-parameter segments. scale, found_inf, step, growth_tracker are DEVICE fp32 scalars, so
 * the optimizer step needs no device->host read.
 * fvqa_grad_unscale_norm: g *= 1/(scale[0]*grad_div) in place; seg_sq[i] = sum g^2 over segment i;
 * total_norm[0] = sqrt(sum_i seg_sq[i]) (the norm of per-parameter norms, util/misc.py:292);
 * found_inf[0] = 1 if any gradient is non-finite else 0 (GradScaler.unscale_).
 * grad_div >= 1: the number of data-parallel replicas whose gradients were SUMMED into `grad` by the all-reduce (DDP's
 * mean of train.py:115-117 without a pass of its own; 1 on a single GPU).
 * gemm_err (may be NULL): device address of a persistent-GEMM workspace's error word (fvqa_gemm_workspace); when it is
 * non-zero the step is skipped like an overflow and found_inf[0] = 2.
 * err_lane (may be NULL): one fp32 that data-parallel ranks all-reduce TOGETHER with the gradients (the element behind the
 * flat gradient buffer, set to 1 by a rank whose error word is raised): non-zero on every rank as soon as one rank's
 * exchange timed out, so all replicas skip the same step (found_inf[0] = 2) and stop together.
 * fvqa_scaler_update leaves the loss scale and its growth tracker untouched when found_inf[0] == 2. */
size_t fvqa_grad_norm_workspace(int n_seg);
int fvqa_grad_unscale_norm(float* grad, const int64_t* seg_off, int n_seg, const float* scale, float grad_div,
                           const void* gemm_err, const float* err_lane, float* seg_sq, float* found_inf,
                           float* total_norm, void* workspace, size_t workspace_bytes, void* stream);
/* AdamW (decoupled weight decay, bias correction with t = step[0]+1), skipped entirely when
 * found_inf[0] != 0 (GradScaler.step semantics). found_inf may be NULL. */
int fvqa_adamw_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                    float lr, float beta1, float beta2, float eps, float weight_decay,
                    const float* step, const float* found_inf, void* stream);
/* after the AdamW launches of one optimizer step: step[0] += 1 unless found_inf; dynamic loss
 * scale update of torch GradScaler (x backoff on overflow, x growth after growth_interval clean
 * steps). step or scale may be NULL. */
int fvqa_scaler_update(float* step, float* scale, float* growth_tracker, const float* found_inf,
                       float growth_factor, float backoff_factor, int growth_interval, void* stream);

/* ---- the rows a head reads ("tail rows") -----------------------------------------------------
 * The reference evaluates `output` at every position and lets the cross-entropy ignore the rows whose next label is 0
 * (llama/model.py:348-350); the QAV head likewise reads the frame-token rows only (:359-361). A row no head
 * reads contributes neither to a loss nor to any gradient — and in the LAST layer nothing else reads its output either. The
 * step therefore runs the last layer's post-attention half (WO + residual, FFN, final norm), the heads and all of their
 * backward on the tail rows only, gathered into a compact matrix; results are those of the dense form.
 * Row movers: a compact matrix of segs->off[n] rows against n streams of `stream_rows` dense rows each.
 *   gather : compact row off[k] + j  <- dense row k*stream_rows + map[k][j]      (an index outside the stream: a zero row)
 *   scatter: dense row k*stream_rows + r <- compact row off[k] + map[k][r], zeros where map[k][r] < 0 (every dense row of
 *            the n streams written exactly once: no pre-clear, no atomics)
 * map[k]: int32 device arrays (gather: off[k+1]-off[k] entries; scatter: stream_rows entries); rows 16-byte aligned,
 * dim a multiple of 16 bytes. */
typedef struct fvqa_row_segs {
  int32_t n, stream_rows;
  int32_t off[4];
  const int32_t* map[3];
} fvqa_row_segs;
int fvqa_gather_rows(const void* src, void* dst, const fvqa_row_segs* segs, int dim, int dtype, void* stream);
int fvqa_scatter_rows(const void* src, void* dst, const fvqa_row_segs* segs, int dim, int dtype, void* stream);

/* ---- native layer schedule (csrc/schedule.hip): the L transformer blocks of the step walked in
 * C++ — two calls per step instead of ~700 per-kernel calls from the host language. Every pointer
 * is a device pointer except the per-layer tables (host arrays of n_layers device pointers).
 * Layer-strided activation buffers are contiguous (layer-major) with R = n_seq*seq_len rows and
 * Ra = R + adapter_len rows. */
typedef struct fvqa_layer_plan {
  int32_t dtype, n_layers, n_seq, seq_len, n_heads, head_dim, adapter_len, max_feats, dim, hidden;
  float eps;
  int32_t reserved_;
  /* frozen weights, per layer: fused and transposed copies (storage dtype) */
  const void* const* wqkv;   /* (3D, D)  */
  const void* const* wo;     /* (D, D)   */
  const void* const* w13;    /* (2Hf, D): W1 | W3 rows interleaved in blocks of 16 (AB16) */
  const void* const* w2;     /* (D, Hf)  */
  const void* const* wqkv_t; /* (D, 3D)  */
  const void* const* wo_t;   /* (D, D)   */
  const void* const* w13_t;  /* (D, 2Hf): transpose of w13 (AB16 columns) */
  const void* const* w2_t;   /* (Hf, D)  */
  const void* const* an;     /* attention_norm weight (D) */
  const void* const* fn;     /* ffn_norm weight (D)       */
  const float* const* gate1; /* (H) fp32 */
  const float* const* gate2;
  float* const* dgate1;      /* (H) fp32, accumulated */
  float* const* dgate2;
  const float* adapter;      /* (L, A, D) fp32 adapter queries of the walked layers */
  void* adapter_c;           /* (L, A, D) scratch: their storage-dtype cast (written by fvqa_layers_fwd) */
  float* d_adapter;          /* (L, A, D) fp32, accumulated */
  const void* norm_w;        /* final norm weight (D) */
  /* forward arena */
  void* xs;                  /* (L+1, R, D): xs[0] in, xs[L] out      */
  float* rstd1;              /* (L, R) */
  float* rstd2;              /* (L, R) */
  void* qkv;                 /* (L, Ra, 3D) */
  void* o;                   /* (L, R, D)   */
  float* lse_a;              /* (L, n_seq*H*S) */
  float* lse_t;
  void* h;                   /* (L, R, D)   */
  void* ab;                  /* (L, R, 2Hf), AB16 */
  void* xn;                  /* (R, D) scratch */
  void* hn;                  /* (R, D)  scratch */
  void* z;                   /* (R, Hf) scratch */
  void* xnf;                 /* (R, D) final-norm output */
  float* rstdN;              /* (R) */
  const float* cos_t;        /* (>=S, Dh/2) */
  const float* sin_t;
  const int32_t* vstart;     /* (n_seq) */
  /* backward scratch */
  void* dcur;                /* (R, D) */
  void* dnxt;                /* (R, D) */
  void* dz;                  /* (R, max(Hf, D)) scratch */
  void* dab;                 /* (R, 2Hf), AB16 */
  void* dh;                  /* (R, D) */
  void* d_o;                 /* (R, D) */
  void* dqkv;                /* (Ra, 3D) */
  void* attn_ws;
  size_t attn_ws_bytes;
  void* gemm_ws;             /* >= fvqa_layers_gemm_workspace(plan) bytes, 256-byte aligned, first 4096 bytes
                                zeroed once after allocation (see fvqa_gemm_workspace) */
  size_t gemm_ws_bytes;
  /* tail rows (fvqa_row_segs above; rows == 0: dense, nothing here is read). With rows > 0 fvqa_layers_fwd runs the
   * last layer's post-attention half and the final norm on the gathered rows — xs[L], h[L-1], ab[L-1], rstd2[L-1], xnf and
   * rstdN are NOT written; tail.xnf (rows, D) is the final-norm output — and fvqa_layers_bwd takes `dxnf` as (rows, D). */
  struct fvqa_tail_rows {
    int32_t rows, reserved_;
    fvqa_row_segs gather, scatter;                  /* the same segments with the idx / inv maps */
    void *og, *xg, *h, *hn, *ab, *z, *xl, *xnf;   /* (rows, D) except ab (rows, 2Hf), z (rows, Hf); saved for the backward: h, ab, xl */
    float *rstd2, *rstdN;                           /* (rows) */
    void *dcur, *dab, *dt, *dh, *d_o;               /* backward scratch: (rows, D) except dab (rows, 2Hf) */
  } tail;
} fvqa_layer_plan;

/* bytes of GEMM workspace the projections of one layer (forward and backward) need at most */
size_t fvqa_layers_gemm_workspace(const fvqa_layer_plan* plan);
/* xs[0] -> ... -> xs[L], xnf = final RMSNorm; saves what the backward needs in the arena */
int fvqa_layers_fwd(const fvqa_layer_plan* plan, void* stream);
/* dxnf (R, D): gradient w.r.t. xnf. *d_x0 <- device pointer (plan->dcur or plan->dnxt) holding the
 * gradient w.r.t. xs[0]; gate / adapter gradients are accumulated into the plan's buffers. */
int fvqa_layers_bwd(const fvqa_layer_plan* plan, const void* dxnf, void** d_x0, void* stream);

/* --train_norm: where the RMSNorm weights' gradients go. d_an[i] / d_fn[i] (dim) fp32: attention_norm / ffn_norm of walked
 * layer i; d_norm (dim): the final norm; all += (segments of the flat gradient buffer). dw_ws: the workspace of
 * fvqa_rmsnorm_dw, >= fvqa_rmsnorm_dw_workspace(n_seq * seq_len, dim) bytes. */
typedef struct fvqa_norm_grads {
  float* const* d_an;        /* [n_layers] */
  float* const* d_fn;        /* [n_layers] */
  float* d_norm;
  void* dw_ws;
  size_t dw_ws_bytes;
} fvqa_norm_grads;
/* fvqa_layers_bwd with one fvqa_rmsnorm_dw (accumulate) queued beside each of its fvqa_rmsnorm_bwd calls, on the same g, x
 * and rstd: the final norm, then per walked layer ffn_norm and attention_norm. With tail rows the final norm and the last
 * layer's ffn_norm reduce over the compact rows — every other row's gradient is zero. norm_grads == NULL: exactly
 * fvqa_layers_bwd (the same launches in the same order). */
int fvqa_layers_bwd_norm(const fvqa_layer_plan* plan, const void* dxnf, void** d_x0, const fvqa_norm_grads* norm_grads,
                         void* stream);

/* ---- small utilities -------------------------------------------------------------------
 * dst rows [row0, row0+n_rows) of a (.., dim) storage-dtype matrix <- fp32 src (n_rows, dim)
 * (adapter_query rows appended under the normed activations, llama/model.py:339) */
int fvqa_cast_rows(const float* src, void* dst, int n_rows, int dim, int dtype, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FVQA_H */
