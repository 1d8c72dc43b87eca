/*
 * ofasys_amd.h -- C ABI of libofasys_amd.so: hand-written gfx950 (MI355X / CDNA4) kernels for the
 * OFASys unified encoder-decoder hot path.
 *
 * What this boundary replaces.  The reference has no C/FFI boundary of its own for this path except the
 * pybind11 fused-softmax extensions; everything else goes torch -> ATen -> cuBLAS/cuDNN.  Each entry point
 * below names the reference call site (relative to /root/reference/ofasys) whose arithmetic it carries.
 *
 * Conventions (carried over from the reference's extensions, module/fused_kernels/scaled_masked_softmax.h:476,
 * scaled_softmax_cuda.cu:84-99, scaled_masked_softmax.cpp:45-49):
 *   - the caller owns every buffer; the library never allocates device memory;
 *   - raw device pointers + explicit sizes / leading dimensions (in ELEMENTS), row-major;
 *   - work is enqueued on the caller's stream (`stream` is a hipStream_t passed as void*), no hidden sync,
 *     no internal threads;
 *   - every function returns an int status: 0 ok, nonzero = error (the Python wrapper raises RuntimeError,
 *     mirroring TORCH_CHECK); shape preconditions are status codes, not asserts;
 *   - dtype is an ofa_dtype; accumulation is always fp32.
 */
#ifndef OFASYS_AMD_H
#define OFASYS_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Element types.  Every entry point takes fp32, bf16 or fp16 storage (`dtype`), accumulates in fp32 and -- for the 16-bit types --
 * multiplies on the matrix cores (v_mfma_f32_32x32x16_bf16 / _f16).  fp16 is the reference trainer's default precision
 * (config/default_trainer.yaml:7-25) and the only dtype it routes to its fused-softmax extensions (multihead_attention.py:83-91);
 * the fused attention kernels (ofa_attn_fwd / _bwd / _bwd_prep) are 16-bit only.  "bf16" in a comment below means "the 16-bit
 * dtype of the call" unless it says otherwise. */
typedef enum { OFA_F32 = 0, OFA_BF16 = 1, OFA_F16 = 2 } ofa_dtype;

enum {
  OFA_OK = 0,
  OFA_ERR_INVALID = 1,     /* bad argument (null pointer, negative size, misaligned leading dimension) */
  OFA_ERR_UNSUPPORTED = 2, /* valid request this build has no kernel for (e.g. head_dim != 64 in the fused path) */
  OFA_ERR_LAUNCH = 3       /* hipLaunch / runtime error; see ofa_last_error() */
};

/* GEMM epilogue flags (ofa_gemm.flags) */
enum {
  OFA_GEMM_BIAS_COL = 1,   /* C[m][n] += bias[n]  (nn.Linear bias)                              */
  OFA_GEMM_BIAS_ROW = 2,   /* C[m][n] += bias[m]  (transposed-output projections)                */
  OFA_GEMM_ACCUM = 4,      /* C = result + C_old  (gradient accumulation)                        */
  OFA_GEMM_FORCE_SIMPLE = 8, /* use the exact-fp32-FMA VALU kernel even for bf16 (tests)         */
  OFA_GEMM_OUT_F32 = 16,   /* bf16 inputs, fp32 output                                           */
  OFA_GEMM_A_KPAD_ZERO = 32, /* caller guarantees A[m][K..roundup8(K)) == 0 (padded logits-gradient rows) */
  OFA_GEMM_NO_LDS_DMA = 64, /* force the register-staged loop (tests / A-B measurements)              */
  OFA_GEMM_DEFER_REDUCE = 128 /* split-K: leave the fp32 partials in ws, the caller folds them (ofa_fold_batched) */
};

int ofa_version(void);
const char* ofa_last_error(void);

/* ---- LayerNorm: torch.nn.LayerNorm(eps, affine) -- module/layer_norm.py:27-32; saves mean and rstd in fp32
 * exactly as the (never built) apex kernel does, fused_kernels/layer_norm_cuda.cpp:136-138. cols <= 8192. */
int ofa_layernorm_fwd(const void* x, const void* gamma, const void* beta, void* y, float* mean, float* rstd,
                      int64_t rows, int cols, float eps, int dtype, void* stream);
/* dgamma/dbeta are [cols] in `dtype` (accumulate != 0: added to their current contents, i.e. straight into a gradient
 * arena); `ws` is fp32 scratch of ofa_layernorm_bwd_ws_rows()*cols floats.  cols <= 2048 (fp32) / 4096 (bf16) per
 * row-part: rows up to 4x that are split over four waves. */
int ofa_layernorm_bwd_ws_rows(void);
/* dres (optional, same shape as x): added to dx -- the gradient that reaches x through a residual branch taken before
 * the LayerNorm (pre-LN layers: `residual = x; x = LN(x)`, transformer_layer.py:159-161), saving the separate add. */
int ofa_layernorm_bwd(const void* dy, const void* x, const void* gamma, const float* mean, const float* rstd,
                      const void* dres, void* dx, void* dgamma, void* dbeta, float* ws, int64_t rows, int cols,
                      int accumulate, int dtype, void* stream);
/* y = LayerNorm(gelu(h)) -- transformer_layer.py:194-197 (fc1 -> GELU (module/gelu.py:18-19, fp32 erf) -> ffn_layernorm). */
int ofa_gelu_layernorm_fwd(const void* h, const void* gamma, const void* beta, void* y, float* mean, float* rstd,
                           int64_t rows, int cols, float eps, int dtype, void* stream);
/* dbias (optional, [cols]): column sums of dh = gradient of the bias of the Linear that produced h (fc1), same
 * accumulate rule as dgamma/dbeta. */
int ofa_gelu_layernorm_bwd(const void* dy, const void* h, const void* gamma, const float* mean, const float* rstd,
                           void* dh, void* dgamma, void* dbeta, void* dbias, float* ws, int64_t rows, int cols,
                           int accumulate, int dtype, void* stream);

/* ---- residual join of a pre-LN sub-block (transformer_layer.py:167-208, 438-494), one pass each way:
 *   y = residual + dropout_p(LN_a(x)),  z = LN_b(y);   LN_a (gamma_a/beta_a) and LN_b (gamma_b/beta_b, z) are optional.
 * stats: fp32 [4][rows] = mean_a, rstd_a, mean_b, rstd_b (kept for the backward).  Dropout as ofa_dropout_add_fwd
 * (Philox position offset + *offset_base).  Rounding points match the unfused kernels (y is bit-identical without LN_a; with it, and for
 * every gradient, the row sums are grouped differently: fp32 rounding noise).
 * Backward: dy / dz = gradients of y / z (NULL = zero); dres = gradient of residual (== total gradient of y), dx = gradient
 * of x; ws: fp32 [5][ofa_join_bwd_slots()][cols] partial rows of dgamma_a, dbeta_a, dgamma_b, dbeta_b and (want_dx_colsum) the
 * column sums of dx -- the bias gradient of the Linear that produced x -- for ofa_fold_batched.
 * residual == NULL (and dres == NULL in backward): y = dropout_p(LN_a(x)) -- the adaptor post-hook's `dropout(layernorm_embedding(embed))`
 * (adaptor/base.py:178-182) in one pass instead of a LayerNorm and a dropout kernel.
 * keep_bits (optional, ofa_join_keep_bytes() bytes; 0 bytes: the shape has no such buffer, pass NULL): the forward leaves the dropout
 * decisions there, one bit per element in the kernels' own lane order, and a backward given the same buffer reads them instead of running the
 * Philox generator again (which is what bounds these kernels, not HBM); NULL on either side: the mask is regenerated, same bits. */
int64_t ofa_join_keep_bytes(int64_t rows, int cols, int dtype);
int ofa_join_fwd(const void* x, const void* residual, const void* gamma_a, const void* beta_a, const void* gamma_b,
                 const void* beta_b, void* y, void* z, float* stats, uint8_t* keep_bits, int64_t rows, int cols, float eps, float p,
                 uint64_t seed, uint64_t offset, const int64_t* offset_base, int dtype, void* stream);
int ofa_join_bwd_slots(int64_t rows, int cols, int dtype);
int ofa_join_bwd(const void* dy, const void* dz, const void* x, const void* y, const void* gamma_a, const void* gamma_b,
                 const float* stats, const uint8_t* keep_bits, void* dres, void* dx, float* ws, int64_t rows, int cols, float p,
                 uint64_t seed, uint64_t offset, const int64_t* offset_base, int want_dx_colsum, int dtype, void* stream);

/* ---- GEMM: C[M,N] = alpha * op(A)[M,K] * op(B)[K,N] (+bias) (+C).  Replaces F.linear / torch.bmm / matmul:
 * multihead_attention.py:199-217,308,338,346; transformer_layer.py:194,202; adaptor/general.py:223-243.
 *   transA == 0: A is [M,K] row-major (lda >= K);  transA == 1: A is stored [K,M] (lda >= M).
 *   transB == 0: B is [K,N] row-major (ldb >= N);  transB == 1: B is stored [N,K] (ldb >= K)  <- nn.Linear weight.
 * batch > 1: strided-batched (strides in elements).  Two-level batching for per-(batch, head) products on [B,T,heads*hd]
 * rows without copies: batch index z addresses operand X at (z / batch_inner)*strideX2 + (z % batch_inner)*strideX
 * (batch_inner <= 0 or >= batch: single level).  bf16 runs on MFMA (v_mfma_f32_32x32x16_bf16) when every
 * leading dimension is a multiple of 8 elements; fp32 (and OFA_GEMM_FORCE_SIMPLE) run an exact fp32-FMA kernel.
 * `ws`/`ws_bytes`: optional fp32 scratch that enables split-K for skinny outputs (may be NULL).
 *
 * Stores.  The MFMA kernels store whole quads of columns: with N4 = (N + 3) & ~3 they need ldc >= N4 (and ldc % 4 == 0; a call that does
 * not offer that runs the exact kernel), and what columns [N, N4) of rows 0 .. M-1 hold after the call is unspecified.  Nothing else
 * outside [M, N] is written: not the columns from N4 on, not a row from M on.  Split-K slabs (ws, or the caller's with
 * OFA_GEMM_DEFER_REDUCE) are [splits][M][N4] fp32.
 * Reads.  Of A and B only op(A)[M, K] and op(B)[K, N] influence C; a vector that crosses the logical edge of an operand is clamped or
 * its lanes are discarded, so rows past the operand's last row and the columns up to its leading dimension may hold anything.  The one
 * exception is OFA_GEMM_A_KPAD_ZERO: A[m][K .. lda) must then be zeros up to the next multiple of 64 that fits in lda (at least up to
 * roundup8(K)); B's rows from K on are not read (the kernels re-read row K-1 against those zeros).
 *
 * OFA_GEMM_ACCUM onto a 16-bit C has two arithmetics, and the plan of the call (ofa_gemm_plan) decides which one runs.  With
 * X = alpha * (op(A) op(B) + bias) in fp32 and rn16 = round to nearest even in C's type:
 *   - a tile kernel that finishes the product in its own epilogue (REG, LDS_DMA, RING, BIG, PP, MIXED with one K-slice) and the direct
 *     path of ofa_gemm_group_tn round the tile, add the old C and round again:           C = rn16(rn16(X) + C_old);
 *   - a split-K product, finished by the reduce launch or by ofa_fold_batched (OFA_GEMM_DEFER_REDUCE, the slabs of ofa_gemm_group_tn),
 *     and the exact kernel (SIMPLE) add the old C in fp32 and round once:                C = rn16(X + C_old).
 * The first is what a 16-bit `grad += g` of the reference does, the second is tighter; the same call may give different bits under
 * another plan.  An fp32 C (OFA_GEMM_OUT_F32, fp32 operands) is accumulated in fp32 on every route.  tests/gemm_exact.py pins both. */
int ofa_gemm(const void* A, const void* B, void* C, const void* bias, int M, int N, int K, int transA, int transB,
             int64_t lda, int64_t ldb, int64_t ldc, int batch, int64_t strideA, int64_t strideB, int64_t strideC,
             int batch_inner, int64_t strideA2, int64_t strideB2, int64_t strideC2,
             float alpha, int flags, int dtype, void* ws, int64_t ws_bytes, void* stream);

/* ofa_gemm (one product, no batch) that ALSO leaves the per-column (sum, sum of squares) of its rounded 16-bit output as partial rows
 * [groups][2][N] fp64, one per wave block of rows, written by the kernel's epilogue from the tile it holds anyway -- the statistics
 * pass of a BatchNorm behind a convolution (module/resnet.py:105-128) for free.  *groups (HOST int, set before the call returns) is
 * the number of partial rows written, or 0 when the selected plan cannot produce them (split-K, fp32 output, accumulation, N % 8,
 * more than max_groups rows): the product is computed either way and the caller then runs its own statistics pass. */
int ofa_gemm_colstat(const void* A, const void* B, void* C, const void* bias, int M, int N, int K, int transA, int transB,
                     int64_t lda, int64_t ldb, int64_t ldc, float alpha, int flags, int dtype, void* ws, int64_t ws_bytes,
                     double* partial, int max_groups, int* groups, void* stream);

/* ---- grouped weight-gradient products: up to 16 independent  slabs_p[s][m][n] = sum over K-slice s of a_p^T b_p  in ONE
 * launch (256 x 256 eight-wave tiles).  The nn.Linear weight gradients of one Transformer layer (dW = dY^T X, what autograd
 * computes for transformer_layer.py:194,202 and multihead_attention.py:199-217,346) are 9-36 such tiles each: launched alone
 * each has to be cut into 3-7 short K-slices to occupy the chip; together they fill it with ~2 long slices each.
 * The slabs are finished by ofa_fold_batched (out (+)= alpha * sum_s slabs[s]).  16-bit operands; any k >= 1 (a row count that
 * is not a multiple of the 64-row K tile is completed with zero rows inside the kernel), m, n, lda, ldb % 8 == 0, 16-byte aligned
 * pointers.  `items` is a HOST array. */
typedef struct ofa_gemm_group_item {
  const void* a;     /* [k, m] rows (lda >= m): output-gradient rows dY */
  const void* b;     /* [k, n] rows (ldb >= n): layer-input rows X */
  float* slabs;      /* [splits][m][n] fp32, written (not accumulated) */
  int64_t lda, ldb;
  int32_t m, n, k;
  int32_t splits;    /* filled by ofa_gemm_group_plan */
  void* out;         /* optional, with out_alpha / ldo: when the plan leaves this product ONE K-slice (splits == 1) the kernel adds */
  int64_t ldo;       /* out_alpha * a^T b straight onto out [m, n] (16-bit, row stride ldo, 16-byte aligned) in its epilogue -- no slab, */
  float out_alpha;   /* no fold launch (the weight gradients of a small micro-batch: every product is one slice).  NULL: always slabs */
  int32_t store;     /* with out, one slice: != 0 WRITES out_alpha * a^T b (the first writer of a gradient in a step: out is not read, the
                      * value is the one adding onto zeros gives); 0 adds onto out.  A product that goes through slabs hands the mode to
                      * its fold job (ofa_fold_job.accumulate) instead. */
} ofa_gemm_group_item;
/* host only: validates the items and fills `splits` (one K-slice length for the group: <= 256 workgroups in total) */
int ofa_gemm_group_plan(ofa_gemm_group_item* items, int n, int dtype);
int ofa_gemm_group_tn(const ofa_gemm_group_item* items, int n, int dtype, void* stream);

/* ---- the reference's fused softmax extensions, wave64 re-derivations.
 * x,y: [b, np, sq, sk]; softmax over sk of scale*x, fp32 accumulate.  sk <= 4096 (scaled_masked_softmax_cuda.cu:47-52). */
int ofa_scaled_softmax_fwd(const void* x, void* y, float scale, int b, int np, int sq, int sk, int dtype, void* stream);
/* dx = scale*(dy*y - y*sum(dy*y)); dx may alias dy (in place, scaled_softmax_cuda.cu:84-99). */
int ofa_scaled_softmax_bwd(const void* dy, const void* y, void* dx, float scale, int b, int np, int sq, int sk,
                           int dtype, void* stream);
/* mask: uint8 [mask_b (b or 1), 1, sq, sk]; masked scores are replaced by -10000.0 (scaled_masked_softmax.h:269-273). */
int ofa_scaled_masked_softmax_fwd(const void* x, const uint8_t* mask, void* y, float scale, int b, int np, int sq,
                                  int sk, int mask_b, int dtype, void* stream);
/* replaces scaled_masked_softmax.cpp:60-77 `backward(output_grads, softmax_results, scale)`: same arithmetic as
 * ofa_scaled_softmax_bwd (the mask does not enter the backward); dx may alias dy -- the reference's backward is completely
 * in place on output_grads (scaled_masked_softmax_cuda.cu:98-117). */
int ofa_scaled_masked_softmax_bwd(const void* dy, const void* y, void* dx, float scale, int b, int np, int sq, int sk,
                                  int dtype, void* stream);
/* x,y: [attn_batches, sq, sq]; implicit causal mask, masked outputs are zero (scaled_upper_triang_masked_softmax.h:113-230). */
int ofa_scaled_upper_triang_masked_softmax_fwd(const void* x, void* y, float scale, int attn_batches, int sq,
                                               int dtype, void* stream);
/* replaces scaled_upper_triang_masked_softmax.cpp:49-64 `backward`: dy,y,dx [attn_batches, sq, sq]; the strictly upper triangle
 * of dy is never read and dx is zero there (scaled_upper_triang_masked_softmax.h:232-329); dx may alias dy (in place,
 * scaled_upper_triang_masked_softmax_cuda.cu:68-95). */
int ofa_scaled_upper_triang_masked_softmax_bwd(const void* dy, const void* y, void* dx, float scale, int attn_batches,
                                               int sq, int dtype, void* stream);
int ofa_get_batch_per_block(int sq, int sk, int b, int np); /* scaled_masked_softmax.h:426-438, kept for API parity */

/* ---- attention-score softmax of the slow path, multihead_attention.py:311-334:
 * p = softmax_fp32( x*scale + bias + causal(-inf above diagonal) ; key_padding -> -inf ) over S.
 * x,bias,p: [BA, T, S] (bias may be NULL); kpm: uint8 [B, S] or NULL (BA = B*heads). */
int ofa_attn_softmax_fwd(const void* x, const void* bias, const uint8_t* kpm, void* p, float scale, int BA, int heads,
                         int T, int S, int causal, int dtype, void* stream);

/* ---- fused attention (bf16, head_dim 64): multihead_attention.py:218-346 without materialising [BA,T,S].  One descriptor for the
 * forward and the backward; a field a call does not use is zero / NULL, and the MODE follows from which pointers are set.
 * Attention dropout is not supported here (the reference default is attention_dropout = 0.0).  No transposed operand copies are
 * needed: the kernels transpose tiles on the LDS read (ds_read_b64_tr_b16).
 *
 * Operands.  q: [B, T, heads*64] rows (ld = ldq elements); k, v: [B, S, heads*64] rows (both ld = ldk); out: [B, T, heads*64]
 * (ld = ldo); lse: fp32 [B*heads, Tpad], the base-2 log-sum-exp of the scaled, biased, masked scores (the forward writes it; it may
 * be NULL there with neither seg nor a shared bias); Tpad: a multiple of 32 covering T.  scale multiplies q.k (the reference
 * pre-scales q, :218) and must be positive (the kernel takes row maxima on the raw scores; the forward refuses a non-positive scale).
 * kpm: optional uint8 [B,S]; c_attn: optional [heads] per-head output scale (:342-345), fp32 or bf16 as c_attn_dtype says (the
 * parameter itself, no cast kernel); causal: non-zero masks above the diagonal; dtype: OFA_BF16 or OFA_F16.
 * Backward: dout: [B,T,heads*64] rows (ld = ldo); delta: fp32 [B*heads, Tpad] = rowsum(dO*O).  out != NULL (the forward output O,
 * rows like dout): the dQ kernel computes delta from dO and O on its way in and WRITES it (rows t < T; in ragged mode also zeros in
 * the filler rows) -- for the dK/dV kernel and ofa_c_attn_grad; no separate pass.  out == NULL (not with a shared bias): delta is an
 * input, filled by ofa_attn_bwd_prep beforehand.  Writes dq [B,T,D] (ld = ldq), dk, dv [B,S,D] (ld = ldk).
 *
 * Dense bias (bias != NULL, bias_swz_row == NULL): [B*heads, T, S] additive, same dtype; dbias (optional, [B*heads,T,S]) receives dS.
 *
 * Batch-SHARED position bias (bias_swz_row != NULL).  The reference adds a dense bias [B*A, T, S] to the scores of every attention
 * of its default configuration (use_self_attn_bias, model/ofa.py:110-113; multihead_attention.py:308-311): abs-pos
 * (pos_q_linear(pos) * pos_scaling) pos_k_linear(pos)^T per head (adaptor/general.py:223-243; cross attention:
 * model/transformer.py:280-299) + table_l[bucket[i][j]] on every slot's diagonal block (general.py:265-280; text.py:101-104,
 * image_resnet.py:116-128, video_image_sequence.py:187-204).  Position embeddings do not depend on the batch row (text: arange;
 * image / video: the patch grid), so that tensor is B copies of ONE [A, Tb, Sb] matrix per layer -- which is what this mode takes,
 * indexed by (head, query position, key position) for every sample; in ragged mode by the position INSIDE the sample (so a batch
 * whose valid positions are a prefix of each padded row packs without touching the bias).  Tb >= T, Sb >= S.
 * The kernels do not read the row-major [heads, Tb, Sb] tensor but its two TILE-SWIZZLED images written by ofa_bias_build (which
 * also does the per-layer assembly of general.py:265-280): per head and 32 x 32 block, the 16 values MFMA lane l = (hi << 5 | i)
 * holds -- element r: row image  bias[32 qt + i][32 kt + (r & 3) + 8 (r >> 2) + 4 hi]  at ((h * nqt + qt) * nkt + kt) * 1024 + 16 l + r,
 * column image  bias[32 qt + (r & 3) + 8 (r >> 2) + 4 hi][32 kt + i]  at ((h * nkt + kt) * nqt + qt) * 1024 + 16 l + r,
 * nqt = ceil(Tb / 32), nkt = ceil(Sb / 32), positions outside [Tb, Sb] zero.  A wave then fetches a block's bias as 2 KiB of
 * consecutive bytes and feeds it to the score MFMAs as their initial accumulator.  The forward reads bias_swz_row (and needs lse);
 * the backward reads both images (and needs out).  dbias (optional): [heads, Tb, Sb] in dbias_dtype (OFA_F32, or a 16-bit code:
 * rounded once, from the fp32 sum) = sum over the batch of dS -- the gradient of the shared bias.  The reference obtains it by
 * materialising dS as [B*A, T, S] and reducing the expand; here a third kernel walks (a chunk of) the batch per [128 x 64] tile of
 * one head, recomputes S and dP of that tile (lse / delta are known) and accumulates dS in registers: no [B*A,T,S] tensor, no
 * atomics, bitwise reproducible.  bias: the row-major [heads, Tb, Sb] tensor in `dtype` (read once per tile by that third kernel;
 * may be NULL when dbias is).  ws / ws_bytes: see ofa_attn_sbias_chunks.
 *
 * Ragged ("packed rows") mode, seg != NULL: the reference pads every sample to the longest and masks the padding
 * (multihead_attention.py:319-326); here the batch may arrive packed instead.  seg: device int32 [B][4] = {q_off, q_len, k_off,
 * k_len} (16-byte aligned; q_off a multiple of 4).  q / out / dout / dq are [rows_q, ld] with sample b's queries in rows q_off ..
 * q_off+q_len-1, k / v / dk / dv are [rows_k, ld] likewise; lse / delta are fp32 [heads, Tpad] indexed by the packed query row
 * (Tpad >= rows_q; delta from ofa_attn_bwd_prep(B = 1, T = rows_q)); T, S are upper bounds of q_len, k_len (they size the launch
 * grid); rows_q / rows_k: total packed rows.  kpm must be NULL, and so must a dense bias / dbias (the shared bias is allowed).  The
 * rows of out / dq / dk / dv outside every segment (alignment / bucket filler) are written as zeros.
 *
 * Column sums (backward, any non-NULL cs_*): the backward also leaves the COLUMN SUMS of its outputs as fp32 partial rows for
 * ofa_fold_batched -- the bias gradients of the q / k / v projections (multihead_attention.py:199-217: q_proj / k_proj / v_proj carry
 * biases) and the gradient of c_attn (:342-345) -- instead of a column-sum pass over dq / dk / dv and ofa_c_attn_grad afterwards.
 * One partial row per (sample, 128-row tile, wave): cs_q: [ofa_attn_cs_slots(B, T)][cs_ldq], columns [64 h, 64 h + 64) of a row
 * written by one wave of the dQ workgroup of head h; cs_k, cs_v: [ofa_attn_cs_slots(B, S)][cs_ldk] likewise by the dK/dV kernel;
 * cs_c: [ofa_attn_cs_slots(B, T)][heads], sum over the wave's 32 rows of delta / c_attn[h].  Every partial row is written on every
 * call (empty tiles of a ragged batch: zeros), the sums are over the fp32 values BEFORE their rounding to `dtype`, in a fixed order.
 * Ragged mode: B = the segment count, T / S = max_q / max_k. */
typedef struct ofa_attn_call {
  const void *q, *k, *v, *dout;
  void* out;                         /* forward: written; backward: read (or NULL) */
  float *lse, *delta;
  void *dq, *dk, *dv;
  const void *bias, *bias_swz_row, *bias_swz_col;
  void* dbias;
  float* ws;
  const uint8_t* kpm;
  const void* c_attn;
  const int32_t* seg;
  float *cs_q, *cs_k, *cs_v, *cs_c;
  int64_t ldq, ldk, ldo, ws_bytes, cs_ldq, cs_ldk;
  int32_t B, heads, T, S, Tpad, Tb, Sb;
  int32_t causal, rows_q, rows_k;
  int32_t dtype, c_attn_dtype, dbias_dtype;
  float scale;
} ofa_attn_call;
int ofa_attn_fwd(const ofa_attn_call* c, void* stream);
int ofa_attn_bwd(const ofa_attn_call* c, void* stream);
int ofa_attn_bwd_prep(const void* dout, const void* out, float* delta, int B, int heads, int T, int Tpad, int64_t ldo,
                      int dtype, void* stream);
int ofa_attn_cs_slots(int B, int rows);
/* Batch chunks the dS-sum kernel of the shared-bias backward cuts B samples into (short sequences: the [128 x 64] tiles of the heads
 * alone would leave the chip idle).  1 and dbias_dtype == OFA_F32 or == dtype: it writes dbias itself, ws may be NULL.  Otherwise ws must
 * hold n * heads * Tb * Sb floats (the chunks' partial sums, folded in chunk order -- and cast -- by ofa_fold_batched inside the call). */
int ofa_attn_sbias_chunks(int B, int heads, int Tb, int Sb);
/* Gradient of the per-head scale c_attn (multihead_attention.py:58, 342-345: attn[t,b,h,:] *= c_attn[h]; O = c * PV, so
 * d c[h] = sum_{b,t} rowsum(dO*O)[b,h,t] / c[h]) from the delta rows of
 * ofa_attn_bwd_prep: dc[h] (+)= sum_b sum_{t<T} delta[(b*heads+h)*ld + t] / c_attn[h]; dc has c_attn's dtype. */
int ofa_c_attn_grad(const float* delta, const void* c_attn, void* dc, int B, int heads, int T, int64_t ld, int accumulate,
                    int c_attn_dtype, void* stream);
/* Decode-time attention (incremental branch, multihead_attention.py:241-279 + 308-346): ONE query row per (batch, head)
 * against a key/value cache.  q, out: [B, heads*64]; k, v: rows of a [B, capacity, ld] cache -- element (b, s, c) at
 * b*k_batch_stride + s*ldk + c -- of which the first S rows are valid; bias: optional [B*heads, S] additive row (the last
 * row of the relative-position bias); kpm: optional uint8 [B, kpm_ld] (non-zero = padded key); c_attn: optional per-head
 * scale (fp32 or bf16 per c_attn_dtype); probs: optional [B*heads, S] softmax output (need_weights).  Softmax in fp32;
 * fp32 and bf16 tensors; head_dim must be 64. */
int ofa_attn_decode(const void* q, const void* k, const void* v, const void* bias, const uint8_t* kpm, const void* c_attn,
                    int c_attn_dtype, void* out, void* probs, int B, int heads, int head_dim, int S, int64_t ldk,
                    int64_t k_batch_stride, int64_t kpm_ld, float scale, int dtype, void* stream);
/* out[b][i] = mean over heads of p[b][a][i], i < n  (head-averaged attention weights, multihead_attention.py:347-351). */
int ofa_mean_heads(const void* p, void* out, int B, int heads, int64_t n, int dtype, void* stream);
/* x: [B, T, C] rows (ld elements) -> xt: [B, C, Tpad] (zero-filled for t >= T). */
int ofa_transpose_heads(const void* x, void* xt, int B, int T, int C, int Tpad, int64_t ld, int dtype, void* stream);

/* ---- embeddings: F.embedding gather (adaptor/text.py:119-127) and its dense-gradient scatter-add, deterministic
 * (a wave per (vocabulary row, id-list slice) scans the ids with ballots; no atomics). ids: int64.
 * present_ws: optional V bytes of scratch (rows that do not occur are skipped); slice_ws: optional fp32 scratch of
 * ofa_embedding_bwd_slices(V, D) * V * D floats -- small tables with thousands of hits per row are then reduced in slices. */
/* Row gather with zero fill: out[r, :] = index[r] >= 0 ? src[index[r], :] : 0 (index int64 [n]; src [src_rows, D]).  Packs the
 * non-pad rows of a padded batch (ofasys_amd/packing.py; the reference computes the padding, preprocessor/utils.py:75-113) and,
 * with the inverse index, scatters gradients back. */
int ofa_gather_rows(const void* src, const int64_t* index, void* out, int64_t n, int D, int64_t src_rows, int dtype,
                    void* stream);
/* The same gather over the VIRTUAL concatenation along the sequence of nparts <= 8 slot outputs (adaptor/general.py:245-282
 * `torch.cat(tuple(x.embed ...), dim=1)`): index[r] = b * T + t addresses the concatenated [batch, T, D], T = sum lens; part k is its own
 * contiguous [batch, lens[k], D] (srcs / lens: HOST arrays).  The concatenated tensor is never built.  ofa_scatter_rows_part is the
 * backward for one part: out [batch, nk, D] row (b, j) = src[inverse[b * T + start + j]] or 0 (src: gradient of the packed rows). */
int ofa_gather_rows_parts(const void* const* srcs, const int* lens, int nparts, const int64_t* index, void* out, int64_t n, int D,
                          int64_t batch, int dtype, void* stream);
int ofa_scatter_rows_part(const void* src, const int64_t* inverse, void* out, int64_t batch, int nk, int Ttot, int start, int D,
                          int64_t src_rows, int dtype, void* stream);
/* out[r, :] = weight[ids[r], :]  (F.embedding, adaptor/text.py:124-125); is_pad (optional, n bytes): is_pad[r] = ids[r] == pad_id -- the
 * padding mask the text adaptor derives from the same ids (adaptor/text.py:108-111), written by the same pass. */
int ofa_embedding_fwd(const void* weight, const int64_t* ids, void* out, int64_t n, int D, int64_t V, uint8_t* is_pad, int64_t pad_id,
                      int dtype, void* stream);
/* dweight[seg_row[s], :] (+)= sum over p in [seg_off[s], seg_off[s+1]) of dout[order[p], :]   (D <= 64 columns).
 * The embedding gradient of a lookup whose ids are the same every step -- the rel-pos bias `table[bucket[i][j]]` (adaptor/text.py:
 * 101-104, image_resnet.py:116-128): order = positions sorted by id (stable), one segment per distinct id, built once per lookup
 * by the caller.  One wave per segment, fixed order: deterministic; accumulate != 0 adds to dweight (the gradient arena). */
int ofa_segment_rowsum(const void* dout, const int32_t* order, const int32_t* seg_off, const int32_t* seg_row, void* dweight, int nseg,
                       int D, int accumulate, int dtype, void* stream);
int ofa_embedding_bwd_slices(int64_t V, int D);
int ofa_embedding_bwd(const void* dout, const int64_t* ids, void* dweight, int64_t n, int D, int64_t V,
                      int64_t padding_idx, uint8_t* present_ws, float* slice_ws, int dtype, void* stream);
/* The same gradient id-major, in one launch without scratch: for id lists of at most OFA_EMBEDDING_IDS_MAX entries (staged in LDS) and
 * rows of whole 16-byte vectors -- ofa_embedding_bwd_ids_ok() says whether (n, D, V, dtype) qualifies.  The first position that holds an
 * id adds every row of that id in increasing position order and updates dweight[id] once.  slices: 1, or the
 * ofa_embedding_bwd_slices(V, D) the caller would have given ofa_embedding_bwd a slice_ws for -- the sums are then grouped as its slices
 * are, so the result equals ofa_embedding_bwd's bit for bit either way.  Rows of ids that do not occur are not touched; the padding id and
 * ids outside [0, V) are skipped. */
#define OFA_EMBEDDING_IDS_MAX 15360
int ofa_embedding_bwd_ids_ok(int64_t n, int D, int64_t V, int dtype);
int ofa_embedding_bwd_ids(const void* dout, const int64_t* ids, void* dweight, int64_t n, int D, int64_t V, int64_t padding_idx,
                          int slices, int dtype, void* stream);
/* The gradient of a lookup by the contiguous ids r0 .. r0 + T - 1 (position tables read with arange(T), the same rows for every sample),
 * from the gradient of the [batch, T, D] tensor the rows were broadcast into: dweight[r0 + t] += round(sum_b dout[b][t]) -- the batch
 * sum in fp32 in batch order, rounded to the storage type as ofa_batch_sum rounds it, then added as ofa_embedding_bwd adds a row:
 * ofa_batch_sum + ofa_embedding_bwd in one pass over dout, bit for bit.  batch == 1: dout is the [T, D] gradient of the rows themselves.
 * The caller promises the ids; nothing is read to check them. */
int ofa_embedding_range_bwd(const void* dout, void* dweight, int batch, int64_t T, int D, int64_t V, int64_t r0, int dtype, void* stream);
/* Debug library only (OFA_STEP_EDGES_OLD = bit mask over the items below): should this caller take the path it took before the
 * one-launch forms above existed?  Always 0 in the product library. */
enum { OFA_EDGE_POS_RANGE = 0, OFA_EDGE_TOKEN_BWD = 1, OFA_EDGE_COLSUM_FOLD = 2, OFA_EDGE_IM2COL = 3 };
int ofa_step_edges_old(int item);
/* Debug library only (OFA_STEP_TAIL_OLD = bit mask over the items below): the gradient plumbing around the optimizer as it ran before
 * -- bit 0: a zero fill of the whole gradient arena, every sink adding (no first-touch writes); bit 1: ofa_sumsq + ofa_step_schedule[_scaled]
 * + the counter add as launches of their own (no ofa_sumsq_schedule); bit 2: ofa_reduce_sum_f32 + ofa_step_stats_add behind the
 * criterion (no ofa_cross_entropy_fwd_grad_stats).  The product library has one path: always 0. */
enum { OFA_TAIL_FIRST_TOUCH = 0, OFA_TAIL_NORM_SCHEDULE = 1, OFA_TAIL_CRITERION_STATS = 2 };
int ofa_step_tail_old(int item);

/* ---- elementwise pieces of the layer (transformer_layer.py:167-208): */
int ofa_gelu_fwd(const void* x, void* y, int64_t n, int dtype, void* stream);                  /* module/gelu.py:18-19 */
int ofa_gelu_bwd(const void* dy, const void* x, void* dx, int64_t n, int dtype, void* stream);
/* QuickGELU of the ViT blocks (module/vit.py: x * sigmoid(1.702 x)); h, a, dy, dh: dense [rows, cols], fp32 math, one rounding.
 * bwd: dh = dy * s * (1 + 1.702 h (1 - s)), s = sigmoid(1.702 h); ws != NULL: also the column sums of dh (the bias gradient of the
 * Linear in front) as fp32 partial rows [ofa_quick_gelu_bwd_slots()][cols], every one written on every call, for ofa_fold_batched.
 * cols must be a whole number of 16-byte vectors and the buffers 16-byte aligned (else OFA_ERR_UNSUPPORTED); rows == 0: nothing. */
int ofa_quick_gelu_fwd(const void* h, void* a, int64_t rows, int cols, int dtype, void* stream);
int ofa_quick_gelu_bwd(const void* dy, const void* h, void* dh, float* ws, int64_t rows, int cols, int dtype, void* stream);
int ofa_quick_gelu_bwd_slots(int64_t rows, int cols, int dtype);        /* host only */
/* y = residual + dropout_p(x); mask is regenerated from (seed, offset) with Philox4x32-10, nothing is stored.
 * offset_base (optional, device int64[1]) is added to `offset` on the device: the stream position of a captured
 * (hipGraph) train step lives there and is advanced by the step itself, so replays draw fresh masks. */
int ofa_dropout_add_fwd(const void* x, const void* residual, void* y, int64_t n, float p, uint64_t seed,
                        uint64_t offset, const int64_t* offset_base, int dtype, void* stream);
int ofa_dropout_bwd(const void* dy, void* dx, int64_t n, float p, uint64_t seed, uint64_t offset,
                    const int64_t* offset_base, int dtype, void* stream);
/* y[r][c] = (a[r][c] + (b? b[rb][c]:0) + (vec? vec[c]:0)) * (rowmask && rowmask[r] ? 0 : 1)  -- adaptor/base.py:168-173,
 * model/transformer.py:110-112.  rb = r, or r % b_period when b_period > 0: b then holds ONE sample's rows (position embeddings are the
 * same for every sample of a batch: adaptor/text.py:124 `embed_positions(arange)`) and is never expanded to [B, T, D]. */
int ofa_add_rowvec_mask(const void* a, const void* b, const void* vec, const uint8_t* rowmask, void* y, int64_t rows,
                        int cols, int64_t b_period, int dtype, void* stream);
/* out[i] (+)= sum_{b < batch} x[b * n + i]  (fp32 accumulation, one rounding): the gradient of such a batch-shared tensor. */
int ofa_batch_sum(const void* x, void* out, int batch, int64_t n, int accumulate, int dtype, void* stream);

/* out[c] (out_dtype) (+)= alpha * sum_r x[r][c]  -- bias gradients of nn.Linear (autograd of multihead_attention.py:199-217). */
int ofa_colsum_ws_floats(int cols);
int ofa_colsum(const void* x, void* out, float* ws, int64_t rows, int cols, int64_t ld, float alpha, int accumulate,
               int dtype, int out_dtype, void* stream);

/* out[i] = sum_{k < n} inputs[k][i] (n <= 16 tensors of `numel` elements; `inputs` is a HOST array of device pointers; fp32
 * accumulation, one rounding): the gradient of a tensor several consumers read -- the abs-position bias that every layer of a stack
 * builds its attention bias from (adaptor/general.py:265-270, model/transformer.py:280-299) -- which autograd would sum with n - 1
 * pairwise adds. */
int ofa_add_n(const void* const* inputs, int n, void* out, int64_t numel, int dtype, void* stream);
/* y = a * b, b either [rows,cols] or a [cols] row vector (c_attn head scale, multihead_attention.py:342-345). */
int ofa_mul(const void* a, const void* b, void* y, int64_t rows, int cols, int b_rowvec, int dtype, void* stream);
/* y[r, :] = x[r, :] * scale[r / group] (fp32 scale per group of `group` consecutive rows): DropPath (module/droppath.py:
 * 40-60) on batch-major rows -- one keep/(1-p) factor per sample. */
int ofa_scale_row_groups(const void* x, const float* scale, void* y, int64_t rows, int cols, int64_t group, int dtype,
                         void* stream);
/* out[0] = sum(x[0..n)) in one deterministic pass (loss = sum of per-row losses). */
int ofa_reduce_sum_f32(const float* x, float* out, int64_t n, void* stream);
/* out[h] = sum_b sum_{t<T} x[(b*heads+h)*ld + t]  (gradient of c_attn from the attention row sums). */
int ofa_head_sum_f32(const float* x, float* out, int B, int heads, int T, int ld, void* stream);

/* ---- attention-bias assembly (adaptor/general.py:265-280): bias [B,A,T,T] (in place) gets values [n,n,A] added on
 * the diagonal block [start, start+n)^2 of every (b,a); the gradient reduces that block over the batch. */
/* Per-layer assembly of the batch-shared position bias, general.py:265-280 on ONE [heads, Tb, Sb] matrix:
 *   out = abs_bias (NULL: zeros);  out[:, s:s+n, s:s+n] += values_k[i][j][h]  for each slot k (values_k: [n, n, heads], `dtype`)
 * written as the row-major tensor (out, optional) and as the two swizzled images the shared-bias attention kernels read (swz_row,
 * swz_col: ofa_bias_swz_elems(heads, Tb, Sb) elements each, 16-byte aligned; layout: see ofa_attn_call).  16-bit dtypes only;
 * slot blocks need Tb == Sb. */
typedef struct ofa_bias_slots {
  const void* values[8];
  const void* values2[8];  /* NULL: a dense slot.  Else an OUTER slot (video_image_sequence.py:187-204: frame-level + patch-level
                            * rel-pos tables): value(i, j) = values[i / inner][j / inner] + values2[i % inner][j % inner], values
                            * [n / inner, n / inner, heads], values2 [inner, inner, heads] -- summed in `dtype` first, like the
                            * reference's broadcast add, without ever forming the [n, n, heads] tensor */
  int32_t start[8];
  int32_t n[8];
  int32_t inner[8];
  int32_t count;
} ofa_bias_slots;
int64_t ofa_bias_swz_elems(int heads, int Tb, int Sb);
int ofa_bias_build(const void* abs_bias, const ofa_bias_slots* slots, void* out, void* swz_row, void* swz_col, int heads, int Tb,
                   int Sb, int dtype, void* stream);
/* Gradient of an OUTER slot from the (batch-summed) bias gradient dbias [heads, T, T]: d_frames [F, F, heads] = sums over the patch
 * pairs, d_patches [P, P, heads] = sums over the frame pairs of the slot's diagonal block (fp32 accumulation, fixed order). */
int ofa_bias_outer_grad(const void* dbias, void* d_frames, void* d_patches, int heads, int T, int start, int F, int P, int dtype,
                        void* stream);
int ofa_bias_block_add(void* bias, const void* values, int B, int A, int T, int start, int n, int dtype, void* stream);
int ofa_bias_block_grad(const void* dbias, void* dvalues, int B, int A, int T, int start, int n, int dtype, void* stream);
/* A slot's OWN per-sample bias (an adaptor whose forward() fills AdaptorOutput.self_attn_bias, which the post-hook leaves alone:
 * adaptor/base.py:183-189; summed into the layer bias at adaptor/general.py:276): bias [B,A,T,T][:, :, s:s+n, s:s+n] += values
 * [B,A,n,n], and the gradient of `values` = that block of dbias, contiguous. */
int ofa_bias_block_add_batch(void* bias, const void* values, int B, int A, int T, int start, int n, int dtype, void* stream);
int ofa_bias_block_slice(const void* dbias, void* dvalues, int B, int A, int T, int start, int n, int dtype, void* stream);

/* ---- patch embedding (adaptor/image_patch_embed.py:59-73): im2col of non-overlapping p x p patches.
 * img [B,C,H,W] -> col [B*(lead + (H/p)*(W/p)), Kpad] with K = C*p*p in (c,ph,pw) order (= Conv2d weight.view(D,-1)), zero pad; every
 * sample's rows start with `lead` all-zero rows (1: the class-token position, so that the projection and its weight gradient run over
 * the [B, 1 + N, D] rows the adaptor returns and `torch.cat((cls_token, x))` (:71-73) never happens). */
int ofa_im2col_patch(const void* img, void* col, int B, int C, int H, int W, int p, int Kpad, int lead, int dtype, void* stream);

/* ---- criterion (engine/criterion/cross_entropy.py:27-67): fp32 log-softmax + NLL(sum, ignore_index) per row.
 * logits [rows, V] (ld elements); writes lse[rows] and row_loss[rows] (0 for ignored rows).
 * Precondition of all three cross-entropy entry points: the logits of columns 0..V-1 are finite (a row holding -inf logits may come out
 * NaN: constrained vocabularies are masked inside ofa_ls_cross_entropy_*, by range and byte mask, never by -inf); columns V..ld-1 are
 * never read into a result. */
int ofa_cross_entropy_fwd(const void* logits, const int64_t* target, float* lse, float* row_loss, int64_t rows,
                          int64_t V, int64_t ld, int64_t ignore_index, int dtype, void* stream);
/* Both in ONE pass over the logits (one read, one write instead of two reads and a write): lse, row_loss AND
 * dlogits = (softmax - onehot) * grad_scale[0] (grad_scale: device scalar known before the forward -- the backward seed or the loss
 * scale; NULL = 1; zero for ignored rows and for columns V..ld-1).  16-bit logits of at most 65536 padded columns
 * (ofa_cross_entropy_fwd_grad_ok != 0), the row is held in the registers of a 1024-thread block.  A non-ignored target outside [0, V)
 * is a caller error this entry survives as ofa_scst_loss_fwd_grad does: nothing is read out of bounds, row_loss = +inf, the gradient row
 * is 0.  (ofa_cross_entropy_fwd / _bwd read x[target] unchecked.) */
int ofa_cross_entropy_fwd_grad_ok(int64_t V, int64_t ld, int dtype);
int ofa_cross_entropy_fwd_grad(const void* logits, const int64_t* target, const float* grad_scale, float* lse, float* row_loss,
                               void* dlogits, int64_t rows, int64_t V, int64_t ld, int64_t ignore_index, int dtype, void* stream);
/* ofa_cross_entropy_fwd_grad plus the bookkeeping that followed it as two single-block launches: the last block to finish (a ticket:
 * `ticket` is one device word that is 0 before the first call; the kernel resets it) writes loss[0] = sum of row_loss in
 * ofa_reduce_sum_f32's order and adds [count of target != ignore_index, loss[0], the same count] to stats (fp64[3]) as
 * ofa_step_stats_add does: the same bits.  rows >= 1. */
int ofa_cross_entropy_fwd_grad_stats(const void* logits, const int64_t* target, const float* grad_scale, float* lse, float* row_loss,
                                     void* dlogits, int64_t rows, int64_t V, int64_t ld, int64_t ignore_index, int dtype, float* loss,
                                     double* stats, unsigned int* ticket, void* stream);
/* dlogits = (softmax - onehot) * grad_scale[0] (device scalar), zero for ignored rows and for columns V..ld-1. */
int ofa_cross_entropy_bwd(const void* logits, const int64_t* target, const float* lse, const float* grad_scale,
                          void* dlogits, int64_t rows, int64_t V, int64_t ld, int64_t ignore_index, int dtype,
                          void* stream);

/* label-smoothed cross entropy fused with the log-softmax (engine/criterion/label_smoothed_cross_entropy.py:62-191):
 * row_loss = (1-eps-eps_i)*nll + eps_i*smooth over the allowed vocabulary: all of it (cstart < 0), or [0,4) U
 * [cstart,cend) (constraint_range), intersected with the optional per-row byte mask cmask [rows, V].  row_cnt receives
 * the allowed count (needed by the backward); ignored rows give 0.  Backward: per-row weights row_w (optional; 0 drops a
 * row -- drop_worst) and the scalar grad_scale multiply the gradient. */
int ofa_ls_cross_entropy_fwd(const void* logits, const int64_t* target, float* lse, float* row_loss, float* row_nll,
                             float* row_cnt, int64_t rows, int64_t V, int64_t ld, int64_t ignore_index, float eps,
                             int64_t cstart, int64_t cend, const uint8_t* cmask, int dtype, void* stream);
int ofa_ls_cross_entropy_bwd(const void* logits, const int64_t* target, const float* lse, const float* row_cnt,
                             const float* row_w, const float* grad_scale, void* dlogits, int64_t rows, int64_t V, int64_t ld,
                             int64_t ignore_index, float eps, int64_t cstart, int64_t cend, const uint8_t* cmask, int dtype,
                             void* stream);
/* The same criterion for closed-set targets, the per-row byte mask replaced by ONE trie node per row (traverse.TraversePlan's CSR:
 * node_edge_off int32 [N + 1], edge_token int32 [E]).  Row r's allowed set A is {edge_token[e] : node_edge_off[n] <= e < node_edge_off[n + 1]},
 * n = node[r], inside [0, V) and, with cstart >= 0, inside [0,4) U [cstart,cend); C = |A|, eps_i = eps / (C - 1 + 1e-6), and lse, row_loss,
 * row_nll, row_cnt = C and the gradient are ofa_ls_cross_entropy_*'s over A.  An edge_token outside [0, V) is skipped, not read.
 * target == ignore_index: row_loss = row_nll = 0 and a zero gradient row.  A live target on a node outside [0, N) (-1: no closed set at
 * that position), on a node with no allowed child (lse = -inf), or that is no allowed child itself: row_loss = row_nll = +inf (the
 * reference masks the target's log-probability to -inf) and a zero gradient row, as ofa_scst_loss_fwd_grad treats an invalid target.
 * fwd: with dlogits != NULL the same launch also writes the gradient row [0, ld) at grad_scale[0] (device scalar, NULL = 1).
 * bwd: the gradient at grad_scale[0] * row_w[r] (row_w optional; 0 drops a row -- drop_worst) from the forward's lse and row_cnt.
 * One workgroup per row reads C logits, not V; every 16-byte vector of the gradient row is written.  dlogits 16-byte aligned. */
int ofa_trie_ls_cross_entropy_fwd(const void* logits, const int64_t* target, const int32_t* node, const int32_t* node_edge_off,
                                  const int32_t* edge_token, int64_t N, int64_t E, const float* grad_scale, float* lse,
                                  float* row_loss, float* row_nll, float* row_cnt, void* dlogits, int64_t rows, int64_t V,
                                  int64_t ld, int64_t ignore_index, float eps, int64_t cstart, int64_t cend, int dtype,
                                  void* stream);
int ofa_trie_ls_cross_entropy_bwd(const void* logits, const int64_t* target, const int32_t* node, const int32_t* node_edge_off,
                                  const int32_t* edge_token, int64_t N, int64_t E, const float* lse, const float* row_cnt,
                                  const float* row_w, const float* grad_scale, void* dlogits, int64_t rows, int64_t V,
                                  int64_t ld, int64_t ignore_index, float eps, int64_t cstart, int64_t cend, int dtype,
                                  void* stream);
/* The trie-edge head (csrc/trie_head.hip): the same criterion computed from FEATURES, the [rows, V] logits and their gradient never
 * built.  Row r on node n = node[r] has the slots j = 0 .. min(degree(n), Cmax) - 1, slot j being edge node_edge_off[n] + j; feats
 * [rows, D] (row stride ld_x), W [V, D] (ld_w), bias [V] or NULL, all of `dtype`, D a whole number of 16-byte vectors, rows 16-byte aligned.
 * fwd, one launch: z[r, j] = feats[r] . W[edge_token[e]] (+ bias) with fp32 accumulation into z fp32 [rows, Cmax]; over the allowed
 * slots ofa_trie_ls_cross_entropy_fwd's lse, row_loss, row_nll, row_cnt (same formulas, same refusals, +inf for a dead row) and the
 * UNSCALED compact gradient g fp32 [rows, Cmax]: g[r, j] = w_nll (p_j - [tok_j == target]) + eps_i (C p_j - 1), exactly 0 in a disallowed
 * slot and in every slot of an ignored, filler (node -1) or dead row.  Slots past a row's degree are not written.  row_hit != NULL
 * (validation): also "the target is the arg-max of the allowed children" with ofa_criterion_eval's tie rule (value, then lowest token);
 * g may then be NULL.
 * bwd_dx: dfeats[r, :] = grad_scale[0] row_w[r] sum_j g[r, j] W[tok_j, :] in `dtype` (row stride ld_dx), every row written in full.
 * bwd_dw: dW[u, :] += grad_scale[0] sum_{(r, j): tok_j = u} row_w[r] g[r, j] feats[r, :] (and dbias[u] += the same sum of coefficients,
 * dbias optional), no float atomics: one wave per distinct token u = head_tokens[.] walks tok_edge[tok_edge_off[.] ..) in order (the
 * plan's inverse CSR by token: head_tokens int32 [U] ascending, tok_edge_off [U + 1], tok_edge [E]), per edge the rows
 * bucket_rows[bucket_off[n] .. bucket_off[n + 1]) of the edge's node n = edge_node[e] in order (rows ordered by node, int32 [rows] and
 * [N + 1], built per step), sums in fp32 and does one read-modify-write of dW[u] in `dtype`: the same inputs give the same bits.  A
 * token without a contributing row is not touched.  grad_scale (device scalar) and row_w are optional (NULL = 1).
 * Every index read from device memory is clamped or skipped before use; a token outside [0, V) is never dereferenced. */
int ofa_trie_head_fwd(const void* feats, int64_t ld_x, const void* W, int64_t ld_w, const void* bias, int64_t D, int64_t V,
                      const int64_t* target, const int32_t* node, const int32_t* node_edge_off, const int32_t* edge_token, int64_t N,
                      int64_t E, int64_t Cmax, float* z, float* lse, float* row_loss, float* row_nll, float* row_cnt, float* g,
                      int32_t* row_hit, int64_t rows, int64_t ignore_index, float eps, int64_t cstart, int64_t cend, int dtype,
                      void* stream);
int ofa_trie_head_bwd_dx(const float* g, const void* W, int64_t ld_w, int64_t D, int64_t V, const int64_t* target, const int32_t* node,
                         const int32_t* node_edge_off, const int32_t* edge_token, int64_t N, int64_t E, int64_t Cmax,
                         const float* row_w, const float* grad_scale, void* dfeats, int64_t ld_dx, int64_t rows, int64_t ignore_index,
                         int64_t cstart, int64_t cend, int dtype, void* stream);
int ofa_trie_head_bwd_dw(const float* g, const void* feats, int64_t ld_x, int64_t D, int64_t V, const int32_t* node_edge_off,
                         const int32_t* edge_node, int64_t N, int64_t E, int64_t Cmax, const int32_t* head_tokens,
                         const int32_t* tok_edge_off, const int32_t* tok_edge, int64_t U, const int32_t* bucket_rows,
                         const int32_t* bucket_off, const float* row_w, const float* grad_scale, void* dW, int64_t ld_dw, void* dbias,
                         int64_t rows, int64_t cstart, int64_t cend, int dtype, void* stream);
/* self-critical sequence training (engine/criterion/scst_loss.py:24-36, 214-233): reward-weighted NLL of the generated tokens, forward
 * AND gradient in one call.  Row r belongs to sentence s = row_seq ? row_seq[r] : r / rows_per_seq and carries the weight
 * w = reward[s] (fp32 [nseq]; an s outside [0, nseq) reads nothing and weighs 0).  Over the allowed vocabulary A -- all of it
 * (cstart < 0), or [0,4) U [cstart,cend) -- it writes
 *     lse = log sum_{v in A} exp(x_v),  row_loss = w (lse - x_t),  dlogits_v = w grad_scale[0] (exp(x_v - lse) - [v == t])   (v in A)
 * and exactly 0 for v outside A, for columns V..ld-1, and for every column of a row whose target is ignore_index (row_loss 0) or whose
 * weight is 0.  A target that is not an allowed column of [0, V) is a caller error the kernel survives: nothing is read out of bounds,
 * row_loss = +inf, the gradient row is 0.  grad_scale: device scalar, NULL = 1.  16-bit logits with ld <= 65536 are held in the
 * registers of a 1024-thread block (one read, one write); fp32 logits and longer rows are read twice.  logits finite, as above. */
int ofa_scst_loss_fwd_grad(const void* logits, const int64_t* target, const float* reward, const int32_t* row_seq,
                           int64_t rows_per_seq, const float* grad_scale, float* lse, float* row_loss, void* dlogits, int64_t rows,
                           int64_t nseq, int64_t V, int64_t ld, int64_t ignore_index, int64_t cstart, int64_t cend, int dtype,
                           void* stream);
/* Validation (engine/criterion/label_smoothed_cross_entropy.py:114-198 in eval mode, compute_loss + compute_accuracy): ONE read of the
 * [rows, V] logits gives, per row, row_loss and row_nll (fp32; ofa_ls_cross_entropy_fwd's formulas: eps = 0 without a constraint is plain
 * cross entropy, row_loss == row_nll) and row_hit (int32: 1 iff the target is the arg-max of the stored logits over the allowed set A,
 * ties to the lowest column -- compared as stored values, so exact).  No gradient, no lse, no log-probabilities are written.
 * A is the whole vocabulary (cstart < 0), [0,4) U [cstart,cend), either intersected with the byte mask cmask [rows, V], or -- with
 * node != NULL -- the children of trie node node[r] as in ofa_trie_ls_cross_entropy_fwd (optionally inside the range; a byte mask
 * and nodes together are refused).  C = |A|; eps_i = eps / (C - 1) unconstrained, eps / (C - 1 + 1e-6) with any constraint.
 * target == ignore_index: row_loss = row_nll = 0, row_hit = 0.  A live target outside [0, V) or outside A: the target column is not
 * read, row_loss = row_nll = +inf, row_hit = 0.  Columns V..ld-1 and disallowed columns never enter a result.  Logits finite.
 * 16-bit logits with ld <= 65536, ld a multiple of 8, a 16-byte aligned base and no byte mask are held in the registers of a 1024-thread
 * block; everything else (fp32, a byte mask, longer rows, any other ld) streams through a 256-thread block, and the node form reads
 * only a node's children.  rows == 0: nothing is launched. */
int ofa_criterion_eval(const void* logits, const int64_t* target, const uint8_t* cmask, const int32_t* node,
                       const int32_t* node_edge_off, const int32_t* edge_token, int64_t N, int64_t E, float* row_loss, float* row_nll,
                       int32_t* row_hit, int64_t rows, int64_t V, int64_t ld, int64_t ignore_index, float eps, int64_t cstart,
                       int64_t cend, int dtype, void* stream);
/* acc fp64[4] = [ntokens, loss_sum, nll_sum, n_correct] += [count of target != ignore_index, sum row_loss, sum row_nll, count of
 * row_hit != 0] of one batch: ONE single-block launch that sums in ofa_reduce_sum_f32's order -- no atomics, the same inputs give the
 * same bits.  rows == 0: nothing is launched. */
int ofa_eval_stats_add(double* acc, const float* row_loss, const float* row_nll, const int32_t* row_hit, const int64_t* target,
                       int64_t rows, int64_t ignore_index, void* stream);
/* get_normalized_probs (model/ofa.py:287-299, module/utils.py:451-462): out fp32 [rows, V] = (log-)softmax_fp32(logits);
 * backward writes dlogits [rows, ld] in `dtype` (columns V..ld-1 zero). */
int ofa_probs_fwd(const void* logits, float* out, int64_t rows, int64_t V, int64_t ld, int log_probs, int dtype,
                  void* stream);
int ofa_probs_bwd(const float* dy, const float* y, void* dlogits, int64_t rows, int64_t V, int64_t ld, int log_probs,
                  int dtype, void* stream);

/* ---- train-step glue (engine/trainer.py:857-884, optim/adam.py:144-218, optim/fp16_optimizer.py): flat arenas. */
int ofa_sumsq_ws_floats(void);
int ofa_sumsq(const void* x, float* out /* fp32[1], accumulated into */, float* ws /* ofa_sumsq_ws_floats() floats */,
              int64_t n, int dtype, void* stream);
/* Scalar schedule of one update, on the device (one thread): gnorm = sqrt(gsq)/sample_size; sched[0] = (1/sample_size) *
 * min(1, clip_norm/(gnorm + 1e-6)) (trainer.py:857-884; no clipping when clip_norm <= 0); step += 1; sched[1] =
 * lr*sqrt(1-b2^step)/(1-b1^step); sched[2] = lr (adam.py:205-207).  sched (fp32[5]) feeds ofa_adam_step(step = 0).
 * Guard (trainer.py:866-876 raises FloatingPointError and skips optimizer.step): a non-finite gnorm or sample_size <= 0 gives
 * sched = [0, 0, lr, skip = 1], leaves `step` unchanged and adds 1 to sched[4] (count of skipped updates, for the host to poll);
 * otherwise sched[3] = 0. */
int ofa_step_schedule(const float* gsq, const double* sample_size, double* step, const double* lr, float* sched,
                      float* gnorm, float clip_norm, double beta1, double beta2, void* stream);
/* ofa_sumsq, then ofa_step_schedule (loss_scaler NULL) or ofa_step_schedule_scaled, then counter[0] += counter_add (counter NULL: none;
 * the Philox stream position of the step) in ONE launch: the last block to finish (`ticket`: one device word, 0 before the first call,
 * reset by the kernel) folds the block partials in ofa_sumsq's order and runs the schedule -- the same bits as the separate launches.
 * gsq[0] is WRITTEN (the sum of squares of x alone; it needs no clearing).  n >= 1; ws: ofa_sumsq_ws_floats() floats. */
int ofa_sumsq_schedule(const void* x, float* gsq, float* ws, unsigned int* ticket, int64_t n, int dtype, const double* sample_size,
                       double* step, const double* lr, float* sched, float* gnorm, double* loss_scaler, int64_t* counter,
                       int64_t counter_add, float clip_norm, double beta1, double beta2, double scale_factor, double scale_window,
                       double tolerance, double threshold, double min_loss_scale, void* stream);
/* stats [3] fp64 += [count of target != pad, loss[0], the same count]: one micro-batch's share of the update's logging sums
 * [sample_size, loss_sum, ntokens] (engine/trainer.py:842-860, criterion/cross_entropy.py:55-67 with sentence_avg = False); loss: a
 * device fp32 scalar; target: int64 [n].  One launch, nothing on the host. */
int ofa_step_stats_add(double* stats, const float* loss, const int64_t* target, int64_t n, int64_t pad, void* stream);
/* The same with a DYNAMIC LOSS SCALE (engine/optim/fp16_optimizer.py:170-204 clip_grad_norm / step, dynamic_loss_scaler.py:9-70):
 * the arena holds loss_scale * (sum of gradients); loss_scaler: device fp64[8] = [loss_scale, iter, last_overflow_iter,
 * last_rescale_iter, overflows_since_rescale, fatal, -, -].  sched[0] = 1 / (loss_scale * sample_size), times clip_norm / gnorm when
 * gnorm > clip_norm > 0 (the fp16 optimizer's form: no 1e-6, no clamp); a non-finite gnorm runs check_overflow (scale /=
 * scale_factor when overflows / iters since the last rescale >= tolerance, floor `threshold` (<= 0: none), `fatal` = 1 instead of
 * the reference's FloatingPointError at min_loss_scale) and skips the update; otherwise update(): scale *= scale_factor every
 * scale_window updates since the last overflow. */
int ofa_step_schedule_scaled(const float* gsq, const double* sample_size, double* step, const double* lr, float* sched,
                             float* gnorm, double* loss_scaler, float clip_norm, double beta1, double beta2, double scale_factor,
                             double scale_window, double tolerance, double threshold, double min_loss_scale, void* stream);
/* Adam on fp32 master weights with grads of `dtype`; coef[0] = grad multiplier (world/sample_size and clip folded
 * in by the caller on device), writes the `dtype` model copy.  Weight decay as adam.py:209-210 (p -= wd*lr*p).
 * step >= 1: bias correction from (lr, step) on the host.  step == 0: coef is device fp32[>=4] = [grad multiplier,
 * lr*sqrt(1-b2^t)/(1-b1^t), lr, skip] -- the schedule state stays on the device (captured train steps); skip != 0 (set by
 * ofa_step_schedule on a non-finite gradient norm) leaves master weights, both moments and the model copy untouched. */
int ofa_adam_step(float* master, float* exp_avg, float* exp_avg_sq, const void* grad, void* model_param,
                  const float* coef, int64_t n, float lr, float beta1, float beta2, float eps, float weight_decay,
                  int step, int dtype, void* stream);
/* The same with the grid capped at max_blocks blocks of 256 threads: 0 = the kernel's own cap of 65536 (a test reaches the second
 * quad of a thread and the second grid-stride trip at a small n with it).  ofa_adam_step forwards here with 0.
 * ofa_adam_step_blocks: host only, the blocks that launch has for n parameters (-1: bad argument). */
int ofa_adam_step_grid(float* master, float* exp_avg, float* exp_avg_sq, const void* grad, void* model_param,
                       const float* coef, int64_t n, float lr, float beta1, float beta2, float eps, float weight_decay,
                       int step, int dtype, int max_blocks, void* stream);
int ofa_adam_step_blocks(int64_t n, int max_blocks);
/* EMA shadow of the weights (engine/ema/ema.py:140-194), decided and applied on the device so that a captured step replays the
 * rule: with t = step[0] (fp64, the number of completed updates) and skip = sched[3] as ofa_step_schedule[_scaled] left them,
 *   apply <=> skip == 0 and t % update_freq == 0;  d = t < start_update ? 0 : decay;  a = fp32(1 - d), rounded once more to a
 *   16-bit state's own type.  That second rounding is what torch's CPU add_(alpha =) does and what the recorded reference holds
 *   (tests/golden/ema.npz); torch's GPU kernel keeps alpha in fp32, so against a reference run on a GPU a bf16 / fp16 state can
 *   differ in its last bit here (bf16(0.1) = 0.10009765625).  An fp32 state (ema_fp32) is not affected.
 *   state <- round_S(float(round_S(float(state) * d)) + a * float(p))       (mul_ then add_(alpha =): two roundings to S, no FMA)
 * state: `state_dtype` elements, fp32 (ema_fp32) or the model's `dtype`; p: the model-dtype parameters as the forward reads them;
 * shadow (optional, NULL: none): round_dtype(state), the weights of the averaged model.  When the rule does not apply nothing is
 * written.  max_blocks: 0 = the kernel's own grid cap (a test reaches the second grid-stride trip at a small n with it).
 * ofa_ema_step: one flat arena of n elements; state 16-byte (fp32) / 8-byte (16-bit) aligned, p and shadow alike for `dtype`. */
int ofa_ema_step(void* state, const void* p, void* shadow, int64_t n, const double* step, const float* sched, double decay,
                 int64_t start_update, int64_t update_freq, int dtype, int state_dtype, int max_blocks, void* stream);
/* ... and the floating-point tensors outside the arena (BatchNorm running statistics) in ONE launch: `segments` is a device table
 * of n records {const void* src; int64_t off; int64_t len} -- len `dtype` elements at src are averaged into state[off, off + len)
 * (and shadow[off, off + len)) of a second flat array of state_numel elements; max_len = the longest len.  Records that leave the
 * array are skipped. */
int ofa_ema_segments_step(void* state, const void* segments, void* shadow, int64_t n, int64_t state_numel, int64_t max_len,
                          const double* step, const float* sched, double decay, int64_t start_update, int64_t update_freq,
                          int dtype, int state_dtype, int max_blocks, void* stream);

/* ---- convolution stack of the image_resnet / video / audio adaptors (module/resnet.py:22-261, module/subsample.py:11-63).
 * Activations are NHWC rows [B*H*W, C]; a convolution is ofa_im2col (taps ordered (kh, kw, c), row length Kpad >=
 * kh*kw*C, zero padded) + ofa_gemm against the weight viewed as [Cout, kh*kw*C]; its input gradient is ofa_gemm +
 * ofa_col2im (gather formulation, deterministic).  x_nchw: the source is the [B,C,H,W] image itself. */
int ofa_conv_out_size(int in, int k, int stride, int pad);
int ofa_im2col(const void* x, void* col, int B, int H, int W, int C, int KH, int KW, int stride, int pad, int Kpad,
               int x_nchw, int dtype, void* stream);
int ofa_col2im(const void* dcol, void* dx, int B, int H, int W, int C, int KH, int KW, int stride, int pad, int Kpad,
               int dtype, void* stream);
/* Host only: the kernel ofa_im2col launches for these sizes -- 0 one element per access, 1 16-byte vectors (NHWC, C and Kpad whole
 * vectors), 2 the LDS tile kernel of an NCHW source (64 * Kpad elements within 48 KB); -1 for a bad argument. */
int ofa_im2col_route(int B, int Ho, int Wo, int C, int Kpad, int x_nchw, int dtype);
/* Host only: the launch shapes of the BatchNorm kernels over [rows, C] -- out[0] the row groups of the statistics kernels (= the fp64
 * partial rows they leave), out[1] log2 of the column vectors per statistics block, out[2] the blocks of the apply / dx kernels. */
int ofa_batchnorm_route(int64_t rows, int C, int dtype, int* out);
/* torch.nn.BatchNorm2d over the rows of [rows, C] (module/resnet.py:105-128): y = [relu]((x-mean)*rstd*gamma + beta
 * [+ residual]).  use_running == 0: batch statistics (biased variance), running buffers (fp32, optional) updated with
 * `momentum` and the unbiased variance; use_running != 0: eval mode.  mean/rstd: fp32 [C] outputs kept for backward.
 * ws: ofa_batchnorm_ws_floats(C) floats.  Backward: g = dy*[y>0] when relu; dres (optional) receives g.  beta (backward, optional;
 * relu layers without a residual input only): the gate is recomputed as [(x-mean)*rstd*gamma + beta > 0] and y is not read. */
int ofa_batchnorm_ws_floats(int C);
int ofa_batchnorm_fwd(const void* x, const void* gamma, const void* beta, const void* residual, void* y, float* mean,
                      float* rstd, float* running_mean, float* running_var, float* ws, int64_t rows, int C, float eps,
                      float momentum, int use_running, int relu, int dtype, void* stream);
int ofa_batchnorm_bwd(const void* dy, const void* y, const void* x, const void* gamma, const float* mean, const float* rstd,
                      void* dx, void* dres, void* dgamma, void* dbeta, float* ws, int64_t rows, int C, int batch_stats,
                      int relu, int accumulate, const void* beta, int dtype, void* stream);
/* SyncBatchNorm (adaptor/image_resnet.py:53-56, 87-90 `sync_bn` -> module/layer.py:26-27 nn.SyncBatchNorm): the same arithmetic in
 * two phases each way, around the CALLER's all-reduce (SUM over the data-parallel ranks) of `sums`:
 *   forward   fwd_stats: sums [2*C + 1] fp64 = this rank's (sum x, sum x^2, row count)  -> all-reduce -> fwd_apply: mean / rstd /
 *             running buffers from the reduced sums (the row count is read on the device: no host sync, ranks may differ), y for
 *             this rank's `rows` rows;
 *   backward  bwd_stats: sums [2][C] fp32 = this rank's (sum g, sum g*xhat); dgamma / dbeta from them (rank-local, like every other
 *             gradient before the gradient exchange) -> all-reduce -> bwd_dx: dx (and dres) with the reduced sums / *total_rows
 *             (device pointer: element 2*C of the forward's reduced sums).
 * fwd_apply with groups > 0 is also the BatchNorm forward BEHIND A CONVOLUTION whose GEMM left the column statistics of its output
 * as `groups` partial rows [groups][2][C] fp64 (ofa_gemm_colstat): no statistics pass over the activation at all. */
int ofa_batchnorm_fwd_stats(const void* x, double* sums, float* ws, int64_t rows, int C, int dtype, void* stream);
int ofa_batchnorm_fwd_apply(const void* x, const void* gamma, const void* beta, const void* residual, void* y, float* mean,
                            float* rstd, float* running_mean, float* running_var, const double* sums, int groups, int64_t rows,
                            int C, float eps, float momentum, int relu, int dtype, void* stream);
int ofa_batchnorm_bwd_stats(const void* dy, const void* y, const void* x, const void* gamma, const float* mean, const float* rstd,
                            float* sums, void* dgamma, void* dbeta, float* ws, int64_t rows, int C, int relu, int accumulate,
                            const void* beta, int dtype, void* stream);
int ofa_batchnorm_bwd_dx(const void* dy, const void* y, const void* x, const void* gamma, const float* mean, const float* rstd,
                         const float* sums, void* dx, void* dres, int64_t rows, const double* total_rows, int C, int relu,
                         const void* beta, int dtype, void* stream);
/* MaxPool2d(K, stride, pad) on NHWC; arg: one byte per output element (arg-max tap), consumed by the backward. */
int ofa_maxpool_fwd(const void* x, void* y, uint8_t* arg, int B, int H, int W, int C, int K, int stride, int pad, int dtype,
                    void* stream);
int ofa_maxpool_bwd(const void* dy, const uint8_t* arg, void* dx, int B, int H, int W, int C, int K, int stride, int pad,
                    int dtype, void* stream);
/* y = relu(x) (gate == NULL), or y = x*[gate > 0] (its backward with gate = the forward output). */
int ofa_relu(const void* x, const void* gate, void* y, int64_t n, int dtype, void* stream);

/* ---- batched fold of fp32 partial rows: out[c] (+)= alpha * sum_{s < nslots} part[s*stride + c], c < cols, for up to
 * any number of jobs in as few launches as possible (56 jobs per launch).  Producers that were asked to leave their
 * partials in place (ofa_layernorm_bwd / ofa_gelu_layernorm_bwd / ofa_colsum with accumulate == OFA_DEFER_FOLD,
 * ofa_gemm with OFA_GEMM_DEFER_REDUCE) are finished by this call; slot order is fixed, results are identical to the
 * immediate reduce.  `jobs` is a HOST array. */
typedef struct ofa_fold_job {
  const float* part;   /* device fp32 partial rows */
  void* out;           /* device output, fp32 or bf16 */
  int64_t cols;
  int64_t stride;      /* elements between consecutive partial rows (>= cols) */
  int32_t nslots;
  int32_t accumulate;  /* bit 0: added to the current contents of out; OFA_FOLD_LANES16: see below */
  float alpha;
  int32_t out_dtype;   /* OFA_F32 / OFA_BF16 */
} ofa_fold_job;
/* `accumulate | OFA_FOLD_LANES16`: a job of more than 16 slots is summed in sixteen slot lanes (lane l: slots l, l + 16, ...; lanes
 * added in lane order) -- the order of ofa_colsum's own final pass, so that a deferred column sum has the bits of an immediate one.
 * Without it such a job is summed in eight lanes (the order of the LayerNorm reduce kernels).  At most 16 slots: slot order either way. */
#define OFA_FOLD_LANES16 4
int ofa_fold_batched(const ofa_fold_job* jobs, int njobs, void* stream);
/* Batched device-to-device copy: dst_i[0 .. bytes_i) = src_i[0 .. bytes_i) for any number of (dense) buffers in as few launches as
 * possible (96 jobs per launch) -- the static inputs of a replayed step graph (engine/trainer.py's _prepare_sample moves a batch to
 * the device tensor by tensor; a replay has to copy each into the graph's input, ~3.5 us per launch).  `jobs` is a HOST array. */
typedef struct ofa_copy_job {
  const void* src;
  void* dst;
  int64_t bytes;
} ofa_copy_job;
int ofa_copy_batched(const ofa_copy_job* jobs, int njobs, void* stream);
/* Batched zero fill, the sibling of ofa_copy_batched: dst_i[0 .. bytes_i) = 0 (src is ignored) -- the gradient-arena views a train
 * step has to clear because no full writer stores to them first (partial writers: embedding rows; parameters nobody wrote). */
int ofa_zero_batched(const ofa_copy_job* jobs, int njobs, void* stream);
#define OFA_DEFER_FOLD 2
/* partial-row count (`nslots`) the corresponding call writes; ws layouts: LayerNorm [q][nslots][cols] with q = dgamma,
 * dbeta(, dbias); colsum [nslots][cols]; split-K GEMM [splits][M][(N+3)&~3] (ofa_gemm_splits == 1: no partials). */
int ofa_layernorm_bwd_slots(int64_t rows, int cols, int dtype, int gelu);
int ofa_colsum_slots(int64_t rows);
int ofa_gemm_splits(int M, int N, int K, int transA, int transB, int batch, int flags, int dtype, int64_t ws_bytes);
/* Host only: the kernel ofa_gemm launches for this product, written to plan[0 .. OFA_GEMM_PLAN_LEN).  Operands as ofa_gemm_splits
 * assumes them: dense (lda = transA ? M : K, ldb = transB ? K : N, ldc = N) and 16-byte aligned -- so a zero-padded contraction
 * (OFA_GEMM_A_KPAD_ZERO) is asked for with K rounded up as its rows are stored.  ws_bytes: the workspace the call passes (0: none). */
enum {
  OFA_GEMM_PLAN_KERNEL = 0,      /* OFA_GEMM_KERNEL_* */
  OFA_GEMM_PLAN_SIMPLE_WHY,      /* kernel SIMPLE: 1 fp32 operands, 2 OFA_GEMM_FORCE_SIMPLE, 3 a shape the MFMA kernels reject; else 0 */
  OFA_GEMM_PLAN_WAVES_M,         /* waves of a workgroup along M, N */
  OFA_GEMM_PLAN_WAVES_N,
  OFA_GEMM_PLAN_WAVE_TM,         /* 32 x 32 accumulator tiles of one wave along M, N */
  OFA_GEMM_PLAN_WAVE_TN,
  OFA_GEMM_PLAN_TILE_M,          /* output tile of a workgroup (MIXED: the tall one) */
  OFA_GEMM_PLAN_TILE_N,
  OFA_GEMM_PLAN_SPLITS,          /* K-slices (> 1: fp32 partial slabs in ws) */
  OFA_GEMM_PLAN_KSPLIT,          /* contraction length of a slice */
  OFA_GEMM_PLAN_K,               /* contraction length the kernel runs (rounded up to whole 64-row tiles where it zero-fills) */
  OFA_GEMM_PLAN_MIXED_TALL,      /* MIXED: row tiles of 256 ... */
  OFA_GEMM_PLAN_MIXED_SHORT,     /* ... and of 192 below them */
  OFA_GEMM_PLAN_COLSTAT_ROWS,    /* rows per column-statistics partial row (ofa_gemm_colstat); 0: the plan cannot write them */
  OFA_GEMM_PLAN_REDUCE,          /* 1: a split-K reduce launch follows */
  OFA_GEMM_PLAN_LEN
};
enum {
  OFA_GEMM_KERNEL_SIMPLE = 0,    /* the exact fp32-FMA VALU kernel */
  OFA_GEMM_KERNEL_REG = 1,       /* register-staged double-buffered loop (gemm_mfma_kernel, GLDS = false) */
  OFA_GEMM_KERNEL_LDS_DMA = 2,   /* LDS-DMA double-buffered loop (gemm_mfma_kernel, GLDS = true) */
  OFA_GEMM_KERNEL_RING = 3,      /* four-stage LDS-DMA ring (gemm_ring_kernel) */
  OFA_GEMM_KERNEL_BIG = 4,       /* eight-wave big tile, lockstep loop (gemm_big_kernel) */
  OFA_GEMM_KERNEL_PP = 5,        /* eight-wave big tile, ping-pong loop (gemm_pp_kernel) */
  OFA_GEMM_KERNEL_MIXED = 6      /* 256- and 192-row big tiles in one launch (gemm_big_mixed_kernel) */
};
int ofa_gemm_plan(int M, int N, int K, int transA, int transB, int batch, int flags, int dtype, int64_t ws_bytes, int* plan);

/* ---- generation steps: beam search (csrc/beam_search.hip), beam search under a forced prefix, trie-constrained beam search
 * (csrc/trie_beam.hip) and sampling (csrc/sample.hip).  Every step is a ROW PASS over the rows' distributions followed by a
 * SENTENCE PASS over a sentence's candidates; both take fixed device addresses and the step number only, so they are recorded inside
 * the per-step hipGraph.  Rows are bsz sentences x K beams (K <= 16, K * V < 2^24).  The two descriptors below are copied by value
 * into the kernel arguments before an entry point returns: nothing on the device reads the caller's host memory.
 *
 * ofa_gen_policy: what a row pass applies to a row's logits.  The fp32 log-softmax normaliser is taken of x / temperature with
 * constraint_range ([4, cstart) and [cend, V) -inf, cstart < 0: off; generator/sequence_generator.py:724, 742-745) applied first;
 * then the reference's post-normaliser masks in order (:296-343): EOS at step < min_len, NaN, PAD, unk_penalty, step >= max_len (all
 * but EOS), n-gram bans over tokens[row, 0..step] (int64 [rows, tok_ld], the token history) when ngram > 0.  done: optional int
 * [bsz] -- rows of finished sentences are skipped. */
typedef struct ofa_gen_policy {
  float temperature;
  int32_t cstart, cend;
  int32_t step, min_len, max_len;
  int32_t pad, unk, eos;
  float unk_penalty;
  int32_t ngram;
  const int64_t* tokens;
  int64_t tok_ld;
  const int32_t* done;
} ofa_gen_policy;

/* ofa_gen_state: what a sentence pass works on.  tokens int64 [rows, tok_ld] (tok_cap valid columns; column 0 = BOS) and scores
 * fp32 [rows, score_ld] are the histories, gathered in place; the next token goes to column step + 1 and the cumulative score to
 * column step.  ignore int [bsz, K] is cands_to_ignore; done int [bsz]; nfin int [1] counts finished sentences; reorder int64 [rows]
 * receives the source row of every row (the identity for a finished sentence).  Finalised hypotheses: fin_tok int64
 * [bsz, K, fin_ld] (tokens 1..step, then EOS), fin_pos fp32 [bsz, K, fin_ld] (positional scores), fin_score fp32 [bsz, K] (divided
 * by (step + 1)^len_penalty when normalize), fin_len / fin_cnt int [bsz, K] / [bsz]. */
typedef struct ofa_gen_state {
  int64_t* tokens;
  int64_t tok_ld;
  int32_t tok_cap;
  float* scores;
  int64_t score_ld;
  int32_t *ignore, *done, *nfin;
  int64_t* reorder;
  int64_t* fin_tok;
  float* fin_pos;
  int64_t fin_ld;
  float* fin_score;
  int32_t *fin_len, *fin_cnt;
} ofa_gen_state;

/* Beam search: the policy of SequenceGenerator.generate / BeamSearch.step (generator/sequence_generator.py:283-492,
 * finalize_hypos :530-627; utils/search.py:107-142) in two launches per decoding step.  ws: ofa_beam_ws_bytes(rows, V, K) bytes,
 * written by ofa_beam_topk and read by ofa_beam_select of the same step.
 * ofa_beam_topk: one read of logits [rows, ld] (V valid columns, fp32 / bf16 / fp16): the normaliser parts and each row's best 2K
 * candidates per 4096-column chunk under `pol`.
 * ofa_beam_select: one workgroup per sentence: the sentence's top min(2K, K * V - 1) candidates (beam 0 only at step 0), then the
 * bookkeeping of the step on `st`. */
int64_t ofa_beam_ws_bytes(int rows, int V, int K);
int ofa_beam_topk(const void* logits, int64_t ld, int rows, int V, int K, const ofa_gen_policy* pol, void* ws, int dtype,
                  void* stream);
int ofa_beam_select(const void* ws, const ofa_gen_state* st, int bsz, int K, int V, int step, int max_len, int eos, int unk,
                    float unk_penalty, int normalize, float len_penalty, void* stream);

/* ---- beam search under a forced target prefix (sample["prefix_tokens"], generator/sequence_generator.py:297-343, 497-523).
 * prefix int64 [bsz, prefix_ld]: the prefix tokens, <pad> where a sentence's prefix has ended; plen int [bsz]: its non-pad
 * entries per sentence.  A step with step < the prefix width and step < max_len is a PREFIX STEP: three launches, recorded in
 * the step graph like the two above.  Rows whose prefix token prefix[sentence, step] is not <pad> are forced, the others free.
 * ofa_beam_prefix_topk: ofa_beam_topk's row pass with the n-gram bans restricted to rows with plen < step + ngram - 1.  With
 * prefix != NULL (a prefix step) the min_len mask is applied to no row, every row stores the scaled logit of its prefix token
 * (constraint_range and temperature applied) in glogit fp32 [rows], and a forced row writes its normaliser parts only.  With
 * prefix == NULL it is a free step of a sample that carries a prefix (glogit unused).
 * ofa_beam_prefix_fill: one workgroup per forced row.  f = min over the rows of the unfinished sentences of
 * (glogit - normaliser) - 1, NaN if any is NaN; the row's candidates under the tie rule (value descending, token ascending) --
 * its prefix token with its own lprob, then the lowest unmasked tokens at f, unk at f - unk_penalty; NaN / -inf f: -inf -- are
 * written to ws as lprobs.  Needs 2K + step + 4 <= min(V, 1024).  Of `pol` it reads step, pad, unk, unk_penalty, ngram, tokens,
 * tok_ld and done.
 * ofa_beam_prefix_select: ofa_beam_select, taking the candidate values of forced rows as lprobs already. */
int ofa_beam_prefix_topk(const void* logits, int64_t ld, int rows, int V, int K, const ofa_gen_policy* pol, const int64_t* prefix,
                         int64_t prefix_ld, const int* plen, float* glogit, void* ws, int dtype, void* stream);
int ofa_beam_prefix_fill(void* ws, int rows, int V, int K, const ofa_gen_policy* pol, const int64_t* prefix, int64_t prefix_ld,
                         const int* plen, const float* glogit, void* stream);
int ofa_beam_prefix_select(const void* ws, const ofa_gen_state* st, int bsz, int K, int V, int step, int max_len, int eos, int unk,
                           float unk_penalty, int normalize, float len_penalty, const int64_t* prefix, int64_t prefix_ld, int pad,
                           void* stream);

/* ---- closed-set scoring (csrc/closed_set_score.hip): TraverseTask.inference (task/traverse_task.py:63-110) without the
 * full-vocabulary projection.  The answer trie arrives as flat int arrays (ofasys_amd/traverse.py TraversePlan): N nodes, E edges
 * grouped by node (node_edge_off [N + 1], edge_token [E], edge_node [E]), per node the (answer, position) whose decoder row
 * holds its hidden state (rep_ans / rep_pos [N]), per answer its path (path_off [C + 1], path_edge [P]) and the work items
 * ([n_items, 3]: node, first edge, one past the last; a few edges of one node each).
 * h: decoder features, row (b * chunk + (answer - c0)) * T + position, ld_h elements apart, D valid; W: output projection rows
 * [V, ld_w]; bias [V] or NULL; h, W and bias share `dtype`; rows 16-byte aligned.  ws: ofa_closed_set_ws_bytes(bsz, E, N) bytes
 * (edge logits fp32 [bsz, E], then node log-sum-exps fp32 [bsz, N]).
 * ofa_closed_set_edge_logits: z[b, e] = h[b, rep(node(e))] . W[edge_token[e]] (+ bias), fp32 accumulation, for the items given
 * whose node's representative answer lies in [c0, c0 + chunk) -- callable once per chunk of answers.
 * ofa_closed_set_reduce: the node log-sum-exps and scores[b, c] = sum over path(c) of (z - lse), fp32 [bsz, C] (two launches).
 * ofa_closed_set_score: both, for features that hold every answer (chunk = C, c0 = 0): three launches, no host synchronisation. */
int64_t ofa_closed_set_ws_bytes(int bsz, int E, int N);
int ofa_closed_set_edge_logits(const void* h, int64_t ld_h, int dtype, const void* W, int64_t ld_w, const void* bias, int D, int V,
                               int bsz, int chunk, int T, int c0, const int* items, int n_items, const int* edge_token,
                               const int* rep_ans, const int* rep_pos, int N, int E, void* ws, void* stream);
int ofa_closed_set_reduce(int bsz, int C, int N, int E, int P, const int* node_edge_off, const int* edge_node, const int* path_off,
                          const int* path_edge, void* ws, float* scores, void* stream);
int ofa_closed_set_score(const void* h, int64_t ld_h, int dtype, const void* W, int64_t ld_w, const void* bias, int D, int V,
                         int bsz, int C, int Tmax, int N, int E, int P, const int* items, int n_items, const int* node_edge_off,
                         const int* edge_token, const int* edge_node, const int* rep_ans, const int* rep_pos, const int* path_off,
                         const int* path_edge, void* ws, float* scores, void* stream);

/* ---- trie-constrained beam search (csrc/trie_beam.hip): a beam-search step whose rows are restricted to the children of the
 * answer trie's node they have reached (generator/sequence_generator.py:729-741), without the [rows, V] output projection.
 * The trie is a TraversePlan's flat arrays (N nodes, E edges: node_edge_off [N + 1], edge_token [E], edge_child [E]: the node an
 * edge leads to, -1 for an EOS edge; max_degree: the largest number of edges of one node).  node int [rows]: the trie node of every
 * row, -1 = dead (its whole distribution is -inf).
 * ofa_trie_beam_topk replaces ofa_beam_topk: h [rows, ld_h] are the decoder's last-position features, W [V, ld_w] / bias [V] or NULL
 * the output projection (one dtype, rows 16-byte aligned); per row one dot product per child edge of node[row] (fp32 accumulation,
 * + bias, / temperature), the fp32 normaliser parts and the best 2K FINITE candidates after the post-normaliser masks of `pol`,
 * written in ofa_beam_topk's layout of ws (ofa_beam_ws_bytes(rows, V, K) bytes) for ofa_beam_select of the same step.  The trie is
 * the only constraint: a `pol` with a constraint range (cstart >= 0) is refused.  Grid (ofa_trie_beam_splits(max_degree, V), rows);
 * a row with fewer than 2K finite candidates is completed with -inf candidates at the lowest token ids not listed, as torch.topk
 * breaks the reference's ties.  At step 0 only beam 0 of a sentence is computed (the sentence pass reads no other).
 * ofa_trie_beam_advance runs after ofa_beam_select: node[row] <- the child of node[reorder[row]] through tokens[row, step + 1]
 * (dead: dead parent, score -inf, EOS edge); a sentence whose K slots are all ignored or at -inf gets done = 1 and bumps nfin.  Of
 * `st` it reads the histories, ignore, reorder, done and nfin; the fin_* fields may be NULL.
 * ofa_trie_beam_splits: the grid's x extent for a plan (0: invalid arguments). */
int ofa_trie_beam_splits(int max_degree, int V);
int ofa_trie_beam_topk(const void* h, int64_t ld_h, int dtype, const void* W, int64_t ld_w, const void* bias, int D, int V,
                       int rows, int K, const int* node, const int* node_edge_off, const int* edge_token, int N, int E,
                       int max_degree, const ofa_gen_policy* pol, void* ws, void* stream);
int ofa_trie_beam_advance(int* node, const int* node_edge_off, const int* edge_token, const int* edge_child, int N, int E,
                          const ofa_gen_state* st, int bsz, int K, int step, void* stream);

/* ---- sampling (csrc/sample.hip): Sampling.step (utils/search.py:596-715) under SequenceGenerator's bookkeeping
 * (generator/sequence_generator.py:283-492), two launches per decoding step, recorded in the step graph like the beam launches.
 * Rows are bsz sentences x K slots (K <= 16, V <= 65536); a sentence's K slots are K independent samples.  No random numbers
 * are made: uniforms fp32 [rows] holds this step's one number in [0, 1) per row.  ws: ofa_sample_ws_bytes(rows, V, K) = 8 * rows
 * bytes (the drawn lprob fp32 [rows], then the drawn token int [rows]), written by ofa_sample_draw and read by ofa_sample_select.
 * ofa_sample_draw: one workgroup per row.  lprobs as ofa_beam_topk computes them under the same `pol` (the fp32 log-softmax of
 * x / temperature under constraint_range, then the post-normaliser masks); weights w = expf(lprob), not renormalised.  Kept set:
 * topp > 0: the tokens whose weight ranked strictly ahead (lprob descending, token ascending) is < topp (everything when the
 * row's total is below topp; topp <= 1); else topk > 0: the topk first of that ranking; else every token.  The draw is the kept
 * token with the smallest id c* such that the kept weight of ids <= c* exceeds u * (the kept weight of the row): an inverse CDF
 * in vocabulary order.  Weights are summed as integers in units of 2^-40, so the result does not depend on any summation order;
 * a row whose kept tokens all weigh less than that unit (or a NaN row: all -inf) draws its top-ranked token.  The lprob written
 * is the one under the full softmax.  At step 0 every row of a sentence reads the sentence's first row, with its own uniform.
 * Rows of finished sentences (done) are skipped and their ws entries left alone.
 * ofa_sample_select: one workgroup per sentence over the K draws: slot j continues itself (slot 0 at step 0) with
 * score = scores[row, step - 1] + lprob; an EOS draw with a finite score in a slot not ignored is finalised; ignored slots stay
 * ignored; the slots that go on are compacted to the front in column order (reorder is not the identity once a slot has ended);
 * a sentence is finished with K hypotheses or at step == max_len.  The bookkeeping on `st` is ofa_beam_select's. */
int64_t ofa_sample_ws_bytes(int rows, int V, int K);
int ofa_sample_draw(const void* logits, int64_t ld, int rows, int V, int K, const ofa_gen_policy* pol, int topk, float topp,
                    const float* uniforms, void* ws, int dtype, void* stream);
int ofa_sample_select(const void* ws, const ofa_gen_state* st, int bsz, int K, int step, int max_len, int eos, int normalize,
                      float len_penalty, void* stream);

/* ---- diverse decoding (csrc/diverse_beam.hip): DiverseBeamSearch.step (utils/search.py:549-593) and DiverseSiblingsSearch.step
 * (:738-787) as sentence passes that replace ofa_beam_select after ofa_beam_topk of the same step: same ws, same arguments, same
 * bookkeeping on `st`, one workgroup per sentence.  Both first reduce every row to its own top 2K by lprob, which needs
 * parts(V) * 2K <= 512.  Ties: value descending, then beam * V + token ascending.  The rewritten scores are the cumulative scores
 * from then on, so hypothesis scores and positional scores contain the penalties, as the reference's do.
 * ofa_diverse_group_select: `groups` G divides K (1 <= G <= K); group g owns beams g, g + G, ... and takes, after the groups before
 * it, its top min(2 K/G, rows * V - 1) of (lprob - strength * count[token]) + cumulative, count = the tokens those groups took
 * (duplicates and -inf picks included); at step 0 it reads row g alone.  The list handed to the bookkeeping is the reference's
 * interleave, rank j of group g at j * G + g.  strength must be finite and >= 0: a penalised top 2 K/G then lies inside the row's
 * unpenalised top 2K, which a reward would leave.
 * ofa_diverse_sibling_select: step 0 is ofa_beam_select's; afterwards the top 2K of ((lprob + cumulative) - (rank + 1) * rate) over
 * every beam's own top 2K, rank counted from 0 inside the beam.  Needs V > 2K; rate finite. */
int ofa_diverse_group_select(const void* ws, const ofa_gen_state* st, int bsz, int K, int V, int step, int max_len, int eos, int unk,
                             float unk_penalty, int normalize, float len_penalty, int groups, float strength, void* stream);
int ofa_diverse_sibling_select(const void* ws, const ofa_gen_state* st, int bsz, int K, int V, int step, int max_len, int eos, int unk,
                               float unk_penalty, int normalize, float len_penalty, float rate, void* stream);

/* ---- CTC loss on the encoder output (csrc/ctc.hip; engine/criterion/speech_to_text_loss.py:217-225, 326-362): F.ctc_loss(log_softmax_fp32
 * (logits), blank = 0, reduction = "sum", zero_infinity), forward and gradient, in four launches that read lengths and targets from
 * device memory (nothing synchronises; grids come from B, Tmax and Lmax) and use no float atomics: equal inputs give equal bits.
 * logits [rows, C] of `dtype`, row stride ld.  Sentence b is the rows seg[b * seg_ld] + t * row_stride, t < seg[b * seg_ld + 1] <= Tmax
 * (seg int32; padded T x B x C: offset b, stride B; packed: a segment table's q_off / q_len, stride 1); a description that leaves
 * [0, rows) or exceeds Tmax reads as an empty sentence.  Labels: target[b, p] - ds (int64 [B, Lmax]) at the positions that are neither
 * pad nor eos, compacted in order by the kernel; a label outside [1, C) makes the sentence infeasible.
 * Sums along the time axis (row_lse, alpha, beta, nll_raw, nll64) are fp64; exp / log run in fp32 on differences of size O(1).
 * A segment out of range trains on as an empty sentence; a row of all -inf logits gives NaN downstream.
 * ofa_ctc_rows: row_lse[r] = log sum_c exp logits[r, c] (fp64) and, if asked for, row_argmax[r] (int32, the lowest class among equals).
 * ofa_ctc_alpha_beta: the two recursions in fp32 log space on logits - row_lse; alpha, beta: fp64 [B, Tmax, 2 Lmax + 1] slabs, ws_meta
 * int32 [B, 3, Lmax] and ws_L int32 [B] for ofa_ctc_grad; nll_raw[b] = -log p(labels | rows) (+inf: infeasible), nll64[b] the same with
 * +inf replaced by 0 under zero_infinity and nll[b] its fp32 rounding.  2 Lmax + 1 <= 2304 and 2 <= C <= 8192 (ofa_ctc_max_target / ofa_ctc_max_classes), else
 * OFA_ERR_UNSUPPORTED.
 * ofa_ctc_grad: dlogits [rows, C] of `dtype` (row stride ld_d) = seed[0] (1 if NULL) * d nll_sum / d logits: every row outside a
 * sentence's length exactly 0, the rows of an infeasible sentence 0 under zero_infinity and NaN without it (torch's values).
 * ofa_ctc_greedy_decode: out[b, :out_len[b]] (int32 [B, Tmax], -1 behind) = the row arg-max of sentence b with consecutive duplicates
 * collapsed, then blanks dropped. */
int64_t ofa_ctc_max_classes(void);
int64_t ofa_ctc_max_target(void);
int ofa_ctc_rows(const void* logits, int64_t ld, int64_t rows, int64_t C, double* row_lse, int32_t* row_argmax, int dtype, void* stream);
int ofa_ctc_alpha_beta(const void* logits, int64_t ld, int64_t rows, int64_t C, const double* row_lse, const int32_t* seg,
                       int64_t seg_ld, int64_t row_stride, int64_t B, int64_t Tmax, const int64_t* target, int64_t Lmax, int64_t ds,
                       int64_t pad, int64_t eos, double* alpha, double* beta, int32_t* ws_meta, int32_t* ws_L, double* nll_raw, float* nll,
                       double* nll64, int zero_infinity, int dtype, void* stream);
int ofa_ctc_grad(const void* logits, int64_t ld, int64_t rows, int64_t C, const double* row_lse, const int32_t* seg, int64_t seg_ld,
                 int64_t row_stride, int64_t B, int64_t Tmax, int64_t Lmax, const double* alpha, const double* beta,
                 const int32_t* ws_meta, const int32_t* ws_L, const double* nll_raw, const float* seed, void* dlogits, int64_t ld_d,
                 int zero_infinity, int dtype, void* stream);
int ofa_ctc_greedy_decode(const int32_t* row_argmax, int64_t rows, const int32_t* seg, int64_t seg_ld, int64_t row_stride, int64_t B,
                          int64_t Tmax, int32_t* out, int32_t* out_len, void* stream);

/* ---- text-to-speech (adaptor/audio.py:327-336, 468-477, 721-763; engine/criterion/tacotron2_loss.py:169-198), csrc/conv1d.hip and
 * csrc/tacotron_loss.hip.
 * Conv1d over time on batch-major channels-last rows: x [B*T, C] -> col [B*T, Kpad], taps ordered (k, c), odd k, padding (k-1)/2,
 * Kpad a multiple of 8 and >= k*C (like ofa_im2col).  A tap outside its own sample's T rows is zero (never the neighbouring sample's
 * row); the columns k*C .. Kpad-1 are zero.  ofa_fold1d is the adjoint as a gather: every dx element is the fp32 sum of its <= k taps
 * in ascending tap order, rounded once.  16-byte accesses when C is a whole number of vectors and the buffers are aligned, else one
 * element per access.  An even k: OFA_ERR_UNSUPPORTED.  B == 0: nothing. */
int ofa_unfold1d(const void* x, void* col, int64_t B, int T, int C, int k, int Kpad, int dtype, void* stream);
int ofa_fold1d(const void* dcol, void* dx, int64_t B, int T, int C, int k, int Kpad, int dtype, void* stream);
/* y = dropout_p(tanh(x)), tanh in fp32; the mask is ofa_dropout_add_fwd's (Philox position offset + *offset_base, element e: halfword
 * e % 8 of counter e / 8).  Backward reads dy and y alone: dx = dy * keep / (1-p) * (1 - t^2), t = y (1-p).  p == 0: exact tanh. */
int ofa_tanh_dropout_fwd(const void* x, void* y, int64_t n, float p, uint64_t seed, uint64_t offset, const int64_t* offset_base,
                         int dtype, void* stream);
int ofa_tanh_dropout_bwd(const void* dy, const void* y, void* dx, int64_t n, float p, uint64_t seed, uint64_t offset,
                         const int64_t* offset_base, int dtype, void* stream);
/* The Tacotron2 criterion over feat_out, post, target [B, T, F] and eos_out [B, T] (contiguous, one dtype); frame (b, t) is valid iff
 * t < lengths[b] (int64, device), N = the number of valid frames:
 *   l1 = sum |feat - tgt| + sum |post - tgt|, mse = the same with squares, eos = sum bce_with_logits(eos_t, [t == len - 1], pos_weight);
 *   OFA_REDUCE_MEAN divides l1 and mse by N F and eos by N, OFA_REDUCE_SUM does not;  out (fp32 [4]) = (l1 + mse + eos, l1, mse, eos).
 * grad != 0: dfeat, dpost [B, T, F] and deos [B, T] of `dtype` = seed[0] (a device scalar; NULL: 1) times the gradient of out[0];
 * padded frames exactly 0, d|d| at d == 0 is 0.  grad == 0 writes the scalars alone (validation).
 * partial: fp64 [3 * ofa_tacotron2_loss_blocks(B*T, F)], folded in a fixed order by a second one-workgroup launch: equal inputs give
 * equal bits.  Refused before any launch: F <= 0 and an unknown reduction (OFA_ERR_INVALID), target_dtype != dtype (OFA_ERR_UNSUPPORTED). */
enum { OFA_REDUCE_MEAN = 0, OFA_REDUCE_SUM = 1 };
int64_t ofa_tacotron2_loss_blocks(int64_t rows, int F);                  /* host only */
int ofa_tacotron2_loss(const void* feat_out, const void* post, const void* target, const void* eos_out, const int64_t* lengths,
                       int B, int T, int F, float bce_pos_weight, int reduction, const float* seed, double* partial,
                       float* out, void* dfeat, void* dpost, void* deos, int grad, int dtype, int target_dtype, void* stream);

/* ---- autoregressive speech generation (generator/speech_generator.py:143-166 with adaptor/audio.py:327-336, 468-477, 721-732),
 * csrc/speech_step.hip: everything a decoding step does after the decoder, in ONE launch recorded into the step's hipGraph.  The
 * descriptor is copied by value into the kernel arguments before the entry point returns.  Per row b of x [B, D] (row stride ldx; the
 * decoder's output at the new position; every tensor of the model dtype unless said otherwise, weights row-major [out, in] as nn.Linear
 * holds them, read in place):
 *   feat = feat_w x + feat_b, rounded to the model dtype  -> feats[b, step, :]  (feats [B, T_cap, out_dim])
 *   p = sigmoid(round(eos_w x + eos_b)) in fp32           -> eos_prob[b, step]  (fp32 [B, T_cap])
 *   a row not yet finished with p > *threshold (strict; a device fp32, so one captured step serves every threshold) finishes: out_lens[b] = step + 1, finished[b] = 1 (both int32 [B]), *nfin += 1
 *   (an integer atomic add per workgroup that has newly finished rows: order-independent, so equal inputs give equal state);
 *   pad_next[b] (uint8 [B]) = finished[b] AFTER the update: the key-padding flag of position step + 1;
 *   embed[b, :] ([B, E]) = proj(prenet(feat)): `layers` x (Linear + ReLU + dropout p_drop), every layer's output rounded to the model
 *   dtype before and after the dropout, then the projection.  Dropout layer l draws ofa_dropout_add_fwd's mask of a [B, P] tensor at
 *   Philox position offset + l * offset_stride + *offset_base (element e = b * P + column: halfword e % 8 of counter e / 8); p_drop == 0
 *   draws nothing and is exact.  Dot products accumulate in fp32.
 * A workgroup owns ofa_speech_step_rows() rows from the head to the embedding: no workgroup waits for another.
 * ofa_speech_step_route (host only): 1 when the shape is served -- D, out_dim, P, E multiples of 8, 1 <= layers <= 4, the rows of a
 * workgroup fit the LDS -- else 0 (-1: unknown dtype); ofa_speech_step refuses the others with OFA_ERR_UNSUPPORTED and weights or
 * buffers that are not 16-byte aligned with OFA_ERR_INVALID. */
typedef struct ofa_speech_step_args {
  const void* x;
  int64_t ldx;
  const void *feat_w, *feat_b, *eos_w, *eos_b;
  const void* pre_w[4];
  const void* pre_b[4];
  const void *proj_w, *proj_b;
  void* feats;
  float* eos_prob;
  int32_t *finished, *out_lens, *nfin;
  uint8_t* pad_next;
  void* embed;
  const int64_t* offset_base;
  const float* threshold;
  uint64_t seed, offset, offset_stride;
  int32_t B, D, out_dim, P, E, layers, step, T_cap;
  float p_drop;
} ofa_speech_step_args;
int ofa_speech_step_rows(void);                                          /* host only */
int ofa_speech_step_route(int D, int out_dim, int P, int E, int layers, int dtype);   /* host only */
int ofa_speech_step(const ofa_speech_step_args* a, int dtype, void* stream);

/* ---- motion diffusion training (adaptor/motion_6d.py:84-107, module/diffusion.py:156-173, engine/criterion/diffusion_loss.py:50-57),
 * csrc/diffusion.hip: the three row passes around the stack.  x0, noise and the loss target are fp32 [B, T, Dd] (contiguous; Dd is
 * rarely a multiple of 4: their rows are read with 16-byte loads when Dd % 4 == 0 and the base is aligned, one element per access
 * otherwise); the model-dtype rows are W = max_data_dim wide and always take 16-byte accesses when W is a whole number of vectors.
 * Levels t (int64 [B], device) index the fp32 schedule tables [n_levels]; a level outside [0, n_levels) is clamped.
 *
 * ofa_diffusion_q_sample: out [B, T, W] of `dtype` <-
 *     x_t = fma(sqrt_acp[t_b], x0, sqrt_1m_acp[t_b] * noise)                      (fp32)
 *     v   = known_w ? fma(known_w[b, t], x0, (1 - known_w[b, t]) * x_t) : x_t     (known_w fp32 [B, T] or NULL; 0 gives x_t, 1 gives x0, exactly)
 *   rounded once to `dtype`; columns >= Dd and the frames with masks[b, t] != 0 (bool [B, T] or NULL) are exact zeros.
 *
 * ofa_film_fwd: out = (rows[r, :D] + 1) * h + rows[r, D:] over h [B, T, D], rows [R, 2D] (one dtype, contiguous, D % 8 == 0), r =
 *   row_of[b, t] (int32 [B, T]) or b when row_of is NULL; fp32 arithmetic (the sum scale + 1 rounded, then one fma), one store rounding.
 * ofa_film_bwd: dh = (rows[r, :D] + 1) * dout, and drows [R, 2D] of `dtype`: drows[r, :D] = sum of dout * h, drows[r, D:] = sum of dout
 *   over the positions of row r, fp32 sums in a fixed order without atomics: workgroup (chunk, b) adds its OFA_FILM_CHUNK frames of
 *   sentence b in ascending t into partial (fp32 [B, chunks, slots, 2D], chunks = ceil(T / OFA_FILM_CHUNK), slots = 1 without row_of,
 *   else 2), then one pass adds the chunks in ascending order.  With row_of, R must be B + 1 and every row_of[b, t] either b or B: the
 *   shared row B collects, in sentence order, every position that is not its sentence's own (the level-0 row of in-betweening).
 *   Without it R >= B.  Every row of drows is written (rows nobody reads: zeros).
 *
 * ofa_diffusion_loss: out (fp32 [1]) = scale / B * sum_b( sum_{t unmasked} sum_{d < Dd} |w_b * (pred - target)| / (Dd * count_b) ),
 *   count_b = the unmasked frames of sentence b (masks NULL: T), w_b = w[t_b] (w NULL, the epsilon objective: 1).  pred [B, T, W] of
 *   `dtype` is read in place at columns < Dd.  Per-thread fp32 sums of a few elements, then fp64 in a fixed order: workgroup (i, b)
 *   owns ofa_diffusion_loss_frames(Dd) frames of sentence b -> partial (fp64 [B, blocks]), counts (fp64 [B]); a second one-workgroup
 *   launch folds them.  grad != 0: dpred [B, T, W] of `dtype` = seed[0] (device scalar; NULL: 1) * scale * w_b * sign(pred - target) /
 *   (Dd * count_b * B), exact zeros at masked frames, at columns >= Dd and where pred == target.  A sentence without an unmasked
 *   frame divides by zero like the reference (the host checks where lengths are host-known).  Equal inputs give equal bits. */
enum { OFA_FILM_CHUNK = 16 };
int ofa_diffusion_q_sample(const float* x0, const float* noise, const int64_t* t, const float* known_w, const void* masks,
                           const float* sqrt_acp, const float* sqrt_1m_acp, int n_levels, int B, int T, int Dd, int W, void* out,
                           int dtype, void* stream);
int ofa_film_fwd(const void* h, const void* rows, const int32_t* row_of, int B, int T, int D, int R, void* out, int dtype, void* stream);
int ofa_film_bwd(const void* dout, const void* h, const void* rows, const int32_t* row_of, int B, int T, int D, int R, void* dh,
                 float* partial, void* drows, int dtype, void* stream);
int64_t ofa_diffusion_loss_frames(int Dd);                               /* host only */
int ofa_diffusion_loss(const void* pred, const float* target, const int64_t* t, const void* masks, const float* w, int n_levels,
                       float scale, const float* seed, int B, int T, int Dd, int W, double* partial, double* counts, float* out,
                       void* dpred, int grad, int dtype, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* OFASYS_AMD_H */
