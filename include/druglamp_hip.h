/*
 * druglamp_hip.h — C ABI of libdruglamp_hip.so (gfx950 / MI355X).
 *
 * The reference (Lzcstan/DrugLAMP) has NO native / FFI layer: its hot path is Python nn.Module
 * composition over stock PyTorch ops.  Every entry point below therefore replaces a *sequence of
 * eager torch ops* inside one reference function; the reference file:line each one stands in for
 * is cited next to it.  The Python host side (druglamp_amd/model/…) keeps the reference's module
 * names, forward signatures and state_dict keys and calls these entry points through ctypes
 * (see INTEGRATION.md for the binding a reference maintainer would add).
 *
 * Conventions
 *   - plain pointers and sizes only; no torch types.  All pointers are DEVICE pointers unless a
 *     parameter says "host".
 *   - the library owns nothing: the caller allocates inputs, outputs and workspaces
 *     (dl_*_workspace_bytes tells how much); no hipMalloc on any path below.
 *   - every launch goes to the hipStream_t passed in (void* here so that C callers need no HIP
 *     headers); nothing synchronises the device.
 *   - return value: 0 on success, negative dl_status otherwise; dl_last_error() gives a
 *     thread-local message.  Nothing aborts.
 *   - dtype: activations/weights are DL_F32 (exact-fp32 MFMA path, parity mode) or DL_BF16
 *     (bf16 MFMA, fp32 accumulate); statistics, biases, norm affine params, losses and all
 *     parameter gradients are fp32.
 */
#ifndef DRUGLAMP_HIP_H
#define DRUGLAMP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum { DL_OK = 0, DL_ERR_ARG = -1, DL_ERR_SHAPE = -2, DL_ERR_ALIGN = -3,
               DL_ERR_WORKSPACE = -4, DL_ERR_LAUNCH = -5, DL_ERR_UNSUPPORTED = -6 } dl_status;

typedef enum { DL_F32 = 0, DL_BF16 = 1 } dl_dtype;

typedef void* dl_stream;   /* hipStream_t */

const char* dl_last_error(void);
int dl_version(void);

/* ------------------------------------------------------------------------------------------
 * dl_gemm — C[m,n] = epilogue( sum_k X[m,k] * W[n,k] )
 *
 * Replaces torch.nn.Linear forward and its two autograd products wherever the hot path uses
 * them: Attention.forward query/key/value/out/fc (model/PMMA/attention.py:90-99,81-83,120),
 * Mlp.forward fc1/fc2 (model/PMMA/mlp.py:44-50), Embeddings.mol_embeddings
 * (model/PMMA/embed.py:40-42), PGCA in/out projections
 * (model/PGCA/guided_cross_attention_model.py:146-161,212,314), MHLA lin1/lin2
 * (model/PMMA/encoder.py:128-129).
 *
 * Operand storage: x_kslow == 0 -> X stored [M][K] (K contiguous, row pitch ldx elements);
 *                  x_kslow == 1 -> X stored [K][M] (M contiguous, pitch ldx).  Same for W/N.
 *   forward  y = x W^T      : X=x  (kslow 0), W=weight (kslow 0)
 *   dgrad    dx = dy W      : X=dy (kslow 0), W=weight viewed [contraction=N_out][K_in] (kslow 1)
 *   wgrad    dW = dy^T x    : X=dy (kslow 1, rows = N_out), W=x (kslow 1, rows = K_in)
 * Epilogue order: v = acc (+bias[n]); save pre_out; act; * gelu'(dact_pre); (+res if
 * res_before_dropout); dropout; (+res otherwise); store (or C += v when accumulate, f32 out).
 * split_k > 1: the contraction is cut into split_k slabs reduced by a second kernel; only the
 * plain epilogue (optionally accumulate) is allowed and out_dtype must be DL_F32.
 * ------------------------------------------------------------------------------------------ */
/* A pending second-stage reduction (see dl_reduce_batch): what dl_gemm's split-K path or dl_layernorm_bwd would have
 * launched right away, handed back to the caller instead so that several of them leave in ONE launch.  At the
 * strong-scaling batches (32-64 pairs per GPU) a step is bound by its launch count, and a third of those launches
 * were these reductions. */
typedef struct dl_reduce_item {
  int32_t kind;          /* DL_REDUCE_NONE (nothing pending), DL_REDUCE_SPLITK, DL_REDUCE_PARTIALS */
  int32_t out_dtype;     /* SPLITK: DL_F32 or DL_BF16 output */
  const float* src;      /* SPLITK: slabs [splits][M*N]; PARTIALS: partial [chunks][stride] */
  void* out;             /* SPLITK: C (row pitch ldc); PARTIALS: float [ncols] */
  int64_t mn;            /* SPLITK: M*N; PARTIALS: stride */
  int64_t ldc;
  int32_t N;             /* SPLITK: N; PARTIALS: ncols */
  int32_t splits;        /* SPLITK: slabs; PARTIALS: chunks */
  int32_t accumulate;
  int32_t M;             /* SPLITK: rows of the column sums that ride along (x_colsum), else 0 */
  const float* cs_slabs; /* SPLITK: [splits][M] or NULL */
  float* cs_out;
} dl_reduce_item;
enum { DL_REDUCE_NONE = 0, DL_REDUCE_SPLITK = 1, DL_REDUCE_PARTIALS = 2 };
enum { DL_REDUCE_BATCH_MAX = 24 };
/* Runs n <= DL_REDUCE_BATCH_MAX pending reductions in one launch; every item's result is bit-identical to what the
 * immediate path produces (same per-element summation order).  The buffers an item points to (the GEMM's workspace,
 * the LayerNorm partials) must stay untouched until this launch has run. */
int dl_reduce_batch(const dl_reduce_item* items, int32_t n, dl_stream s);

typedef struct {
  const void* X; int64_t ldx; int32_t x_kslow;
  const void* W; int64_t ldw; int32_t w_kslow;
  void* C; int64_t ldc;
  int64_t M, N, K;
  int32_t in_dtype, out_dtype;
  const float* bias;                 /* [N] or NULL */
  const void* residual; int64_t ldr; /* in_dtype, [M or res_row_mod][N] or NULL */
  int64_t res_row_mod;               /* >0: residual row = m % res_row_mod (positional table) */
  int32_t res_before_dropout;
  int32_t act;                       /* 0 none, 1 exact-erf GELU, 2 ReLU */
  void* pre_out; int64_t ldp;        /* in_dtype, pre-activation copy or NULL */
  const void* dact_pre; int64_t lddp;/* in_dtype, multiply by gelu'(dact_pre[m,n]) or NULL */
  float dropout_p; uint64_t dropout_seed;
  int32_t accumulate;
  int32_t split_k; void* workspace; size_t workspace_bytes;
  float* x_colsum;                   /* weight-gradient form only (x_kslow && w_kslow, plain epilogue): also writes
                                        x_colsum[m] = sum_k X[k][m], m < M (the bias gradient that accompanies
                                        dW = dY^T x, reference nn.Linear backward) from the X fragments the kernel
                                        streams anyway; fp32 [M] or NULL.  Counted in dl_gemm_workspace_bytes. */
  const uint64_t* dropout_seed_offset; /* DEVICE pointer or NULL: the mask is keyed by dropout_seed + *offset, read when
                                        the kernel runs — lets a hipGraph-captured step draw fresh masks per replay */
  int32_t algo;                      /* DL_GEMM_ALGO_AUTO, or DL_GEMM_ALGO_TILE128: never take the 256-wide persistent
                                        kernels (gemm_big.cuh) — outputs are bit-identical either way (tested) */
  int32_t* tile_tickets;             /* NULL, or a DEVICE array of 2 int32 that is ZERO on entry (and is zero again when the
                                        launch has finished): the one-workgroup-per-CU persistent kernel then takes its
                                        tiles beyond the first from an atomic ticket counter instead of a static stride, so
                                        a CU that starts late — e.g. because an RCCL channel workgroup of an overlapped
                                        gradient all-reduce was sitting on it — costs its share of tiles, not a second
                                        round.  Outputs are bit-identical with and without (tested). */
  dl_reduce_item* deferred;          /* NULL, or HOST pointer: a split-K call writes its slabs, describes the pending
                                        reduction here and does NOT launch it (kind = DL_REDUCE_NONE when the call took no
                                        split); the caller owns the workspace until dl_reduce_batch has run */
  int32_t prof_tag;                  /* sub-family of this product for the timing hooks (dl_prof_collect_tag): DL_TAG_*;
                                        no effect on the computation */
} dl_gemm_args;
enum { DL_TAG_OTHER = 0, DL_TAG_QKV_OUT = 1, DL_TAG_FFN = 2, DL_TAG_CONV = 3, DL_TAG_WGRAD = 4, DL_TAG_ADAPTOR = 5 };
enum { DL_GEMM_ALGO_AUTO = 0, DL_GEMM_ALGO_TILE128 = 1 };

size_t dl_gemm_workspace_bytes(const dl_gemm_args* a);
int dl_gemm(const dl_gemm_args* a, dl_stream s);
/* Two products of identical shape, layout and epilogue (the two streams of a paired PMMA block, reference
 * model/PMMA/block.py:33-62: the same layer applied to the drug stream and to the protein stream with separate
 * weights) in ONE launch when both are on the 128-tile path without split-K: at the strong-scaling batches each of them
 * fills half the CUs and the step is bound by its launch count.  Otherwise (large-tile / split-K shapes, x_colsum,
 * deferred reductions, different flags) the two run one after the other exactly as two dl_gemm calls.  Results are
 * bit-identical to two dl_gemm calls either way (tested). */
int dl_gemm_pair(const dl_gemm_args* a, const dl_gemm_args* b, dl_stream s);
/* n <= 16 weight-gradient products of DIFFERENT shapes in ONE launch (round 3): the dW = dY^T X products of one block's
 * backward (reference model/PMMA/block.py:33-62 as autograd differentiates it: fc1 / fc2 / out / fc / qkv of both streams).
 * At the strong-scaling batches each of them alone is a few 128 x 128 tiles over 8192-16384 rows: a launch, a prologue and a
 * 16- to 32-way split-K slab round trip for microseconds of matrix work.  Grouped, the tile lists are concatenated, the
 * parallelism comes from the number of products and the slab count drops to 1-4.  Every member is a dl_gemm_args in the
 * weight-gradient form (bf16 operands, x_kslow = w_kslow = 1, plain f32 output, split_k = 0, accumulate = 0; optional
 * x_colsum and `deferred`); dl_gemm_group_plan returns the slab count the library will use for each member (its workspace
 * must hold splits * M * (N + (x_colsum ? 1 : 0)) floats) or DL_ERR_UNSUPPORTED for a group it does not take (the caller
 * then issues dl_gemm calls).  A member's result is the fixed-order sum of its slabs like dl_gemm's, but NOT bit-identical
 * to the dl_gemm call (different slab count). */
int dl_gemm_group_plan(const dl_gemm_args* args, int32_t n, int32_t* splits_out);
int dl_gemm_group(const dl_gemm_args* args, int32_t n, dl_stream s);

/* column sums: out[n] (+)= sum_m X[m,n] — bias gradients of every Linear above. */
int dl_colsum(const void* X, int64_t ldx, int64_t M, int64_t N, int32_t dtype, float* out,
              int32_t accumulate, void* workspace, size_t workspace_bytes, dl_stream s);
size_t dl_colsum_workspace_bytes(int64_t M, int64_t N);

/* ------------------------------------------------------------------------------------------
 * BatchNorm over the rows of a channel-last [R][C] matrix (ProteinCNN's BatchNorm1d after each
 * Conv1d+ReLU, model/basic_model.py:176-178, with activations kept channel-last so that each Conv1d
 * is ONE dl_gemm over overlapping rows; see druglamp_amd/functional.py ProteinCNNFn).
 * Row validity: rows are grouped in windows of `win` rows; row r takes part iff
 * halo <= (r % win) < halo + valid  (win == 0: every row).  Invalid (halo) rows are written as zeros
 * by the apply kernels, so the next convolution sees zero padding.
 *   stats      : sums[0..C) = sum_r y, sums[C..2C) = sum_r y^2 over valid rows (fp32)
 *   apply_fwd  : z = (y - mean) * rstd * gamma + beta
 *   bwd_reduce : sums[0..C) = sum dz, sums[C..2C) = sum dz * yhat       (yhat = (y-mean)*rstd)
 *   bwd_apply  : dy = gamma*rstd*(dz - sums0/n - yhat*sums1/n), then * (y > 0) when relu_mask
 *                (y is the post-ReLU conv output that fed the BatchNorm)
 * ------------------------------------------------------------------------------------------ */
size_t dl_bn_workspace_bytes(int64_t R, int64_t C);
int dl_bn_stats(const void* y, int64_t R, int64_t C, int64_t win, int64_t halo, int64_t valid,
                int32_t dtype, float* sums, void* workspace, size_t workspace_bytes, dl_stream s);
/* sums (from dl_bn_stats: [sum | sum of squares]) -> batch mean, biased variance, rstd = rsqrt(var + eps), and
 * nn.BatchNorm1d's running-statistics update (momentum, unbiased running variance) in one launch; running_* may
 * be NULL. */
int dl_bn_finalize(const float* sums, int64_t n, float eps, float momentum, float* mean, float* var, float* rstd,
                   float* running_mean, float* running_var, int64_t C, dl_stream s);
int dl_bn_apply_fwd(const void* y, void* z, const float* mean, const float* rstd, const float* gamma,
                    const float* beta, int64_t R, int64_t C, int64_t win, int64_t halo, int64_t valid,
                    int32_t dtype, dl_stream s);
int dl_bn_bwd_reduce(const void* dz, const void* y, const float* mean, const float* rstd, int64_t R,
                     int64_t C, int64_t win, int64_t halo, int64_t valid, int32_t dtype, float* sums,
                     void* workspace, size_t workspace_bytes, dl_stream s);
int dl_bn_bwd_apply(const void* dz, const void* y, const float* mean, const float* rstd,
                    const float* gamma, const float* sums, float inv_n, int32_t relu_mask, void* dy,
                    int64_t R, int64_t C, int64_t win, int64_t halo, int64_t valid, int32_t dtype,
                    dl_stream s);
/* Row-weight forms of the four BatchNorm passes (round 4: ProteinCNN on distinct rows, reference model/basic_model.py:155-180
 * over the tiled sequences of utils.py:392-412; tables: druglamp_amd/protein_plan.py).  row_w [R] fp32 replaces the window
 * rule: row_w[r] < 0 a halo row (excluded from every sum, written as zeros), 0 a context row (computed and normalised, not
 * part of the statistics), m >= 1 a row that stands for m identical rows of the reference's layout:
 *   stats_rw      sums = [sum m y | sum m y^2]                      (n of dl_bn_finalize = sum of the weights)
 *   bwd_reduce_rw sums = [sum dz | sum dz * yhat] over rows with row_w >= 0 (a row's dz already is the sum over its copies)
 *   bwd_apply_rw  dy = gamma * rstd * (dz - m * (S0 / n + yhat * S1 / n)), then the ReLU mask; halo rows zero. */
int dl_bn_stats_rw(const void* y, int64_t R, int64_t C, const float* row_w, int32_t dtype, float* sums, void* workspace,
                   size_t workspace_bytes, dl_stream s);
/* dl_bn_stats (row_w = NULL: the window rule) or dl_bn_stats_rw (row_w given) followed by dl_bn_finalize, in two launches
 * instead of three: the second stage of the column reduction also forms mean / biased var / rstd and updates the running
 * statistics (nn.BatchNorm1d, basic_model.py:160-178).  Same arithmetic in the same order: bit-identical results.  sums [2C]
 * may be NULL. */
int dl_bn_stats_finalize(const void* y, int64_t R, int64_t C, int64_t win, int64_t halo, int64_t valid, const float* row_w,
                         int32_t dtype, int64_t n, float eps, float momentum, float* sums, float* mean, float* var, float* rstd,
                         float* running_mean, float* running_var, void* workspace, size_t workspace_bytes, dl_stream s);
int dl_bn_apply_fwd_rw(const void* y, void* z, const float* mean, const float* rstd, const float* gamma, const float* beta,
                       int64_t R, int64_t C, const float* row_w, int32_t dtype, dl_stream s);
int dl_bn_bwd_reduce_rw(const void* dz, const void* y, const float* mean, const float* rstd, int64_t R, int64_t C,
                        const float* row_w, int32_t dtype, float* sums, void* workspace, size_t workspace_bytes, dl_stream s);
int dl_bn_bwd_apply_rw(const void* dz, const void* y, const float* mean, const float* rstd, const float* gamma,
                       const float* sums, float inv_n, int32_t relu_mask, void* dy, int64_t R, int64_t C, const float* row_w,
                       int32_t dtype, dl_stream s);
/* Weighted tail rows (round 3: MolecularGCN's compact padding form, model/basic_model.py — the reference's virtual padding
 * nodes, handler/dataset.py:216-221, are identical in every layer and computed once).  Inside every window of `win` rows
 * the rows [lead, win) stand for w identical rows each; their incoming gradient is already the sum over those copies.
 * dl_bn_bwd_apply (run first, inv_n = 1 / the expanded row count) gave them the mean terms once; this adds the other
 * w - 1: dy[r] -= (w - 1) gamma rstd (S1 inv_n + xhat[r] S2 inv_n), in place, tail rows only. */
int dl_bn_tail_fix(void* dy, const void* y, const float* mean, const float* rstd, const float* gamma, const float* sums,
                   float inv_n, int32_t w, int64_t R, int64_t C, int64_t win, int64_t lead, int32_t dtype, dl_stream s);
/* BatchNorm1d followed by ReLU (round 5; the Linear -> BatchNorm1d -> ReLU stages of the SimSiam MLPs,
 * model/self_supervised_learning.py:126-166): z = max(0, (y - mean) rstd gamma + beta) over rows of [R][C]; the backward takes
 * the gradient dz with respect to z, recomputes the ReLU's open set from y, and gives sums [2C] = (d beta, d gamma) and dy
 * (three launches: masked partial sums, their reduction, the apply pass).  workspace: dl_bn_workspace_bytes(R, C). */
int dl_bn_apply_relu_fwd(const void* y, void* z, const float* mean, const float* rstd, const float* gamma, const float* beta,
                         int64_t R, int64_t C, int32_t dtype, dl_stream s);
int dl_bn_relu_bwd(const void* dz, const void* y, const float* mean, const float* rstd, const float* gamma, const float* beta,
                   float inv_n, void* dy, float* sums, int64_t R, int64_t C, int32_t dtype, void* workspace, size_t workspace_bytes,
                   dl_stream s);
/* Backward of a BatchNorm that ran on fixed statistics (eval mode: mean / rstd from the running statistics; frozen-BatchNorm
 * fine-tuning and input gradients of a deployed model).  dx does not depend on the column sums, so this is ONE pass over dz
 * and y plus the second stage over the per-workgroup partials:
 *   yhat = (y - mean) rstd;  g = dz, counted only where yhat gamma + beta > 0 when relu_out (a ReLU behind the BatchNorm);
 *   dy = g gamma rstd, zero where y <= 0 when relu_in (y is the output of the ReLU in front of the BatchNorm);
 *   sums[0..C) = sum g (d beta), sums[C..2C) = sum g yhat (d gamma) over the rows that take part.
 * Rows: the window rule (win, halo, valid; win = 0: every row), or row_w [R] when given: row_w[r] < 0 excludes the row.  The
 * weight is otherwise not applied: a compact row's dz already is the sum over the rows it stands for and yhat is shared by
 * them, so the unweighted sum over the compact rows is the sum over the expanded ones.  Excluded rows of dz and y are never
 * read; their dy rows are written as +0.  beta is read only with relu_out (else may be NULL).  sums may be NULL: the dy pass
 * alone, no workspace.  Otherwise workspace: dl_bn_workspace_bytes(R, C); the sums are deterministic (fixed order, no atomics).
 * dy must not alias dz or y.  bf16 with C in {64, 128, 256} and 16-byte bases takes the 16-byte form, everything else the
 * generic one. */
int dl_bn_eval_bwd(const void* dz, const void* y, const float* mean, const float* rstd, const float* gamma, const float* beta,
                   int32_t relu_in, int32_t relu_out, void* dy, float* sums, int64_t R, int64_t C, int64_t win, int64_t halo,
                   int64_t valid, const float* row_w, int32_t dtype, void* workspace, size_t workspace_bytes, dl_stream s);

/* ------------------------------------------------------------------------------------------
 * LayerNorm over the last dim (eps 1e-6 inside PMMA: model/PMMA/block.py:23-27,
 * model/PMMA/encoder.py:31; eps 1e-5 for v/x_gca_norm: model/basic_model.py:115,118).
 * fwd: y = (x - mean) * rstd * gamma + beta ; mean/rstd [M] f32 saved for bwd (may be NULL).
 * bwd: dx = LN'(dy) (+ dres if given); dgamma/dbeta [D] f32 (+)= column reductions.  dy_share >= 1:
 *      row r of x takes row r / dy_share of dy (1 = one dy row per x row; L = the gradient of a mean over
 *      L tokens, `f.mean(dim=1)` at model/DrugLAMP.py:73, read in place instead of expanded to M rows).
 * ------------------------------------------------------------------------------------------ */
int dl_layernorm_fwd(const void* x, int64_t ldx, const float* gamma, const float* beta, void* y,
                     int64_t ldy, float* mean, float* rstd, int64_t M, int64_t D, float eps,
                     int32_t dtype, dl_stream s);
size_t dl_layernorm_bwd_workspace_bytes(int64_t M, int64_t D);
int dl_layernorm_bwd(const void* dy, int64_t lddy, int64_t dy_share, const void* x, int64_t ldx, const float* mean,
                     const float* rstd, const float* gamma, const void* dres, int64_t lddres,
                     void* dx, int64_t lddx, float* dgamma, float* dbeta, int32_t accumulate,
                     int64_t M, int64_t D, int32_t dtype, void* workspace, size_t workspace_bytes,
                     dl_reduce_item* deferred, dl_stream s);
/* deferred (HOST pointer or NULL): with dbeta == dgamma + D the final [2][D] column reduction is described there instead
 * of launched (dl_reduce_batch runs it; the workspace must stay untouched until then); kind = DL_REDUCE_NONE otherwise. */

/* ------------------------------------------------------------------------------------------
 * Fused attention: O = softmax(scale * Q K^T) V, no mask, no dropout
 * (attention_dropout_rate = 0, configs/default_config.py:81; PGCA dropout = 0).
 *
 * One launch covers `n_problems` independent (K,V) sets ("problems" = batch x streams), each
 * with n_heads heads.  Every problem has 1 or 2 query SEGMENTS of Lq rows each that attend to
 * the SAME K/V — this is Attention.paired_attention (model/PMMA/attention.py:44-88): segment 0
 * is the stream's own q, segment 1 the other stream's q ("guided" attention), and the two
 * outputs land side by side ([attn | attn_p], the torch.cat at attention.py:81).
 * n_segments == 1 gives plain self attention (attention.py:109-122, head dim 128) and PGCA's
 * cross attention (guided_cross_attention_model.py:290-311; Lq=256, Lk=512, 1 head).
 *
 * Addressing (element strides, all tensors dtype `dtype`, head dim contiguous):
 *   own q   (p, h, r, :)   = Q + p*q_ps + h*q_hs + r*q_rs
 *   segment 0 of problem p queries with Q(p); segment 1 with Q(partner(p)),
 *       partner(p) = (p + partner_shift) % n_problems      (paired streams: [stream][batch]
 *       ordering, partner_shift = batch)
 *   k/v     (p, h, r, :)   = K + p*k_ps + h*k_hs + r*k_rs  (same for V with v_*)
 *   o  (seg, p, h, r, :)   = O + seg*o_ss + p*o_ps + h*o_hs + r*o_rs
 *   lse(seg, p, h, r)      = LSE + ((seg*n_problems + p)*n_heads + h)*Lq + r  (f32, natural log)
 * raw_logits (optional, f32): scale*QK^T before softmax, [p][h][Lq][Lk] for segment 0 —
 * what GuidedCrossAttention returns as its 2nd output (guided_cross_attention_model.py:307,316-320).
 * head_dim in {64, 128}; strides multiples of 16 bytes; Lq, Lk arbitrary (tails are masked).
 * ------------------------------------------------------------------------------------------ */
typedef struct {
  const void* Q; const void* K; const void* V; void* O; float* LSE; float* raw_logits;
  int64_t q_ps, q_hs, q_rs, k_ps, k_hs, k_rs, v_ps, v_hs, v_rs, o_ps, o_hs, o_rs, o_ss;
  int32_t n_problems, n_heads, n_segments, partner_shift, Lq, Lk, head_dim, dtype;
  float scale;
  int32_t algo;   /* DL_ATTN_ALGO_AUTO, or DL_ATTN_ALGO_STREAM: key tiles streamed through LDS whatever the lengths
                     (the form every long sequence takes; AUTO keeps K/V LDS-resident when Lk <= 256 at head_dim 64) */
  /* Key multiplicities (round 5; one segment only).  The last key_tail_rows keys each stand for key_tail_weight identical
   * keys of the attention the reference computes: PGCA's key / value rows are the 512 drug nodes / tokens of a molecule
   * (model/DrugLAMP.py:55-56), of which everything beyond the batch's block is one repeated padding row (virtual GCN nodes,
   * handler/dataset.py:216-221; zero token rows, utils.py:304-312).  softmax over the full key set = softmax over the distinct
   * keys with log(weight) added to a repeated key's logit; O, LSE and (backward) dQ are those of the full attention, dK / dV of
   * a tail key are the SUMS over the keys it stands for.  0 rows = plain attention. */
  int32_t key_tail_rows;
  float key_tail_weight;
} dl_attn_fwd_args;
enum { DL_ATTN_ALGO_AUTO = 0, DL_ATTN_ALGO_STREAM = 1, DL_ATTN_ALGO_TWO_PASS = 2, DL_ATTN_ALGO_ONE_PASS = 3 };
/* Backward at head_dim 64, bf16, Lk <= 256 (one segment, or two with partner(partner(p)) = p): AUTO takes the one-pass kernel
 * (dQ, dK, dV from one evaluation of P and dS) when it has a workgroup for every CU, the dQ + dK/dV kernel pair otherwise;
 * TWO_PASS / ONE_PASS force the choice (tests, A/B); ONE_PASS on an ineligible shape falls back to the pair. */
int dl_attn_fwd(const dl_attn_fwd_args* a, dl_stream s);

/* Backward.  dO is addressed like O (do_* strides); Delta has the shape of LSE and is scratch
 * filled by the call (rowsum(dO*O)).  dQ(p) receives BOTH contributions of q tensor p (its own
 * attention's segment 0 and its partner attention's segment 1) from one workgroup — nothing is
 * accumulated across launches and the result is deterministic.  dK/dV(p) sum over the segments
 * of attention p.  All three are overwritten. */
typedef struct {
  const void* Q; const void* K; const void* V; const void* O; const void* dO;
  const float* LSE; float* Delta;
  void* dQ; void* dK; void* dV;
  int64_t q_ps, q_hs, q_rs, k_ps, k_hs, k_rs, v_ps, v_hs, v_rs, o_ps, o_hs, o_rs, o_ss;
  int64_t do_ps, do_hs, do_rs, do_ss, dq_ps, dq_hs, dq_rs, dk_ps, dk_hs, dk_rs, dv_ps, dv_hs, dv_rs;
  int32_t n_problems, n_heads, n_segments, partner_shift, Lq, Lk, head_dim, dtype;
  float scale;
  int32_t algo;   /* as in dl_attn_fwd_args */
  int32_t key_tail_rows;     /* as in dl_attn_fwd_args (must match the forward call) */
  float key_tail_weight;
} dl_attn_bwd_args;
int dl_attn_bwd(const dl_attn_bwd_args* a, dl_stream s);

/* ------------------------------------------------------------------------------------------
 * Attention probability maps: out = softmax(scale * Q K^T) as fp32, V never touched.
 *
 * What the reference hands back for interpretation: GuidedCrossAttention's attn_output_weights
 * (guided_cross_attention_model.py:307-327 — the softmax at 308, the mean over heads at 324-327 when
 * need_weights and not need_raw) and the `weights` the PMMA Attention returns under vis=True
 * (model/PMMA/attention.py: attention_probs of paired_attention / forward).
 *
 * Problems, segments, heads and the Q / K addressing are dl_attn_fwd's (q_*, k_* strides,
 * partner_shift).  P[q][k] = exp(scale q.k + log w_k - LSE_q) with the LSE layout of dl_attn_fwd:
 * LSE may be the one a dl_attn_fwd call wrote for the same Q, K, scale and key tail (workspace may
 * then be NULL); with LSE == NULL the call first computes the statistics into `workspace`
 * (dl_attn_probs_workspace_bytes: n_segments * n_problems * n_heads * Lq floats).
 * Output rows have a pitch of out_ld ELEMENTS (>= the column count); nothing beyond a row's columns is written:
 *   head_mean == 0: row ((seg * n_problems + p) * n_heads + h) * Lq + q holds head h's map
 *   head_mean == 1: row (seg * n_problems + p) * Lq + q holds (1 / n_heads) sum_h P_h, summed in ascending h
 *                   (no atomics: bitwise repeatable)
 * Key multiplicities (key_tail_rows = t, key_tail_weight = w, one segment, as dl_attn_fwd; lead = Lk - t):
 *   expand_tail == 0: Lk columns, the softmax over the DISTINCT keys — a tail key's column carries the mass
 *                     of the w keys it stands for (any w >= 1)
 *   expand_tail == 1: lead + t * w columns, the map over the FULL key set in the order the host's expansion
 *                     of the tail uses: column lead + i * t + j (i < w, j < t) holds the probability of ONE
 *                     copy of tail key j, exp(scale q.k_{lead+j} - LSE_q).  w must be a whole number.
 * head_dim in {64, 128}; Q / K 16-byte aligned with strides multiples of 16 bytes; Lq, Lk arbitrary.
 * 16-byte stores when out is 16-byte aligned and out_ld a multiple of 4, 4-byte stores otherwise.
 * ------------------------------------------------------------------------------------------ */
typedef struct {
  const void* Q; const void* K; const float* LSE; float* out; int64_t out_ld;
  int64_t q_ps, q_hs, q_rs, k_ps, k_hs, k_rs;
  int32_t n_problems, n_heads, n_segments, partner_shift, Lq, Lk, head_dim, dtype;
  float scale;
  int32_t head_mean, key_tail_rows; float key_tail_weight; int32_t expand_tail;
  void* workspace; size_t workspace_bytes;
} dl_attn_probs_args;
size_t dl_attn_probs_workspace_bytes(const dl_attn_probs_args* a);
int dl_attn_probs(const dl_attn_probs_args* a, dl_stream s);

/* ------------------------------------------------------------------------------------------
 * Pair-indexed PGCA attention core (forward only): the screening path's cross attention over
 * cached per-entity operands.
 *
 * GuidedCrossAttention's key-is-value branch (guided_cross_attention_model.py:138-162,290-314) projects
 * the query from the protein alone and key / value from the drug alone, and its out-projection is
 * linear behind the softmax: softmax(Q K^T) V W_o^T = softmax(Q K^T) (V W_o^T).  So Q is kept per
 * protein, K and V' = V W_o^T per drug, and a (protein, drug) pair needs only the core below.
 *
 * For pair n < n_pairs with p = q_index[n], d = kv_index[n] (int32, device memory):
 *   S = scale * Q[p] K[d]^T  (+ log key_tail_weight on the last key_tail_rows keys, as dl_attn_fwd)
 *   O = softmax(S) V[d]  (+ bias[c] in column c, fp32, if bias is given)
 *   out (n, r, out_col0 + c) = O[r][c]         c < head_dim, r < Lq
 *   out (n, r, c)            = left (p, r, c)  c < left_cols (bitwise copy; only with left != NULL)
 * Addressing (element strides, all tensors dtype `dtype`, columns contiguous):
 *   q    (e, r, :) = Q + e*q_es + r*q_rs          e < n_q    (K, V: k_*, v_*, e < n_kv, r < Lk)
 *   left (e, r, :) = left + e*left_es + r*left_rs  e < n_q
 *   out  (n, r, :) = out + n*out_ps + r*out_rs
 * Nothing is written outside the addressed columns of the addressed rows.
 * A pair whose index is outside [0, n_q) or [0, n_kv) is skipped — nothing is read through the index,
 * nothing is written for the pair — and DL_FLAG_PAIR_INDEX is OR-ed into *flags (flags may be NULL).
 * One head, head_dim == 128 (else DL_ERR_UNSUPPORTED); Lq, Lk arbitrary (tails are masked); pointers 16-byte
 * aligned, strides multiples of 16 bytes; left_cols and out_col0 multiples of 8 elements, left_cols <= out_col0;
 * key_tail_rows <= Lk, key_tail_weight >= 1.  n_pairs == 0: DL_OK, nothing is launched.
 * ------------------------------------------------------------------------------------------ */
typedef struct {
  const void* Q; const void* K; const void* V; const void* left; void* out; const float* bias;
  const int32_t* q_index; const int32_t* kv_index; uint32_t* flags;
  int64_t q_es, q_rs, k_es, k_rs, v_es, v_rs, left_es, left_rs, out_ps, out_rs;
  int32_t n_pairs, n_q, n_kv, Lq, Lk, head_dim, dtype;
  int32_t left_cols, out_col0;
  float scale;
  int32_t key_tail_rows; float key_tail_weight;
} dl_pgca_pairs_args;
int dl_pgca_pairs_fwd(const dl_pgca_pairs_args* a, dl_stream s);

/* ------------------------------------------------------------------------------------------
 * Pair-indexed PGCA attention core over a packed per-drug row store (forward only): the resident
 * drug library of the screening path.  dl_pgca_pairs_fwd takes one Lk and one key_tail_weight for the
 * whole launch; here every drug has its own key count and multiplicity, read from a device table.
 * Both entry points launch the same kernel (csrc/pgca_pairs.hip), which differs only in where a
 * workgroup finds its keys: on a store of equal-length drugs with w_d = 1 they give the same bits.
 *
 * K and V point into one row store of kv_total_rows rows ([K | V'] with row strides k_rs, v_rs).
 * Drug d < n_kv owns the segment of Lk_d = kv_keys[d] rows that starts at row kv_row0[d]; each of the
 * segment's last key_tail_rows rows stands for w_d = kv_tail_weight[d] identical keys (w_d = 1: ordinary
 * keys).  key_tail_rows is launch-wide.
 *
 * For pair n < n_pairs with p = q_index[n], d = kv_index[n] (int32, device memory):
 *   S = scale * Q[p] K_d^T  (+ log w_d on the last key_tail_rows keys of the segment)
 *   O = softmax(S) V_d  (+ bias[c] in column c, fp32, if bias is given)
 *   out (n, r, out_col0 + c) = O[r][c]         c < head_dim, r < Lq
 *   out (n, r, c)            = left (p, r, c)  c < left_cols (bitwise copy; only with left != NULL)
 * Addressing (element strides, all tensors dtype `dtype`, columns contiguous):
 *   q    (e, r, :) = Q + e*q_es + r*q_rs          e < n_q
 *   K_d  (j, :)    = K + (kv_row0[d] + j)*k_rs     j < Lk_d     (V_d: V, v_rs)
 *   left (e, r, :) = left + e*left_es + r*left_rs  e < n_q
 *   out  (n, r, :) = out + n*out_ps + r*out_rs
 * kv_row0 (int64), kv_keys (int32), kv_tail_weight (float): device vectors of n_kv entries.
 * Nothing is written outside the addressed columns of the addressed rows; no row outside a pair's
 * segment is read for it.
 * The table lives on the device, so the kernel checks it: a pair is skipped — nothing is read through
 * its table entry, nothing is written for it — when
 *   its index is outside [0, n_q) or [0, n_kv)                        -> DL_FLAG_PAIR_INDEX is OR-ed into *flags
 *   kv_row0[d] < 0, kv_keys[d] < max(1, key_tail_rows),
 *   kv_row0[d] + kv_keys[d] > kv_total_rows, or kv_tail_weight[d] is
 *   not a finite value >= 1                                            -> DL_FLAG_KEY_TABLE
 * (flags may be NULL).  One head, head_dim == 128 (else DL_ERR_UNSUPPORTED); Lq arbitrary; Q / K / V / left / out /
 * bias 16-byte aligned, strides multiples of 16 bytes; kv_row0 8-byte, the other index vectors 4-byte aligned;
 * left_cols and out_col0 multiples of 8 elements, left_cols <= out_col0, out_rs >= out_col0 + 128;
 * key_tail_rows >= 0, kv_total_rows >= 0.  n_pairs == 0: DL_OK, nothing is launched.
 * ------------------------------------------------------------------------------------------ */
typedef struct {
  const void* Q; const void* K; const void* V; const void* left; void* out; const float* bias;
  const int32_t* q_index; const int32_t* kv_index;
  const int64_t* kv_row0; const int32_t* kv_keys; const float* kv_tail_weight; uint32_t* flags;
  int64_t q_es, q_rs, k_rs, v_rs, left_es, left_rs, out_ps, out_rs, kv_total_rows;
  int32_t n_pairs, n_q, n_kv, Lq, head_dim, dtype;
  int32_t left_cols, out_col0;
  float scale;
  int32_t key_tail_rows;
} dl_pgca_pairs_ragged_args;
int dl_pgca_pairs_ragged_fwd(const dl_pgca_pairs_ragged_args* a, dl_stream s);

/* ------------------------------------------------------------------------------------------
 * Pair-indexed PGCA probability maps: the softmax weights of the two attention cores above, as fp32,
 * straight from the cached per-entity operands (csrc/pgca_pairs_probs.hip).  What the reference hands
 * back for interpretation (get_cross_attn_prob: which drug atoms / tokens each protein site attends to)
 * for the (protein, drug) pairs of a screen.  No value row is read; there is no V, left or bias.
 *
 * dl_pgca_pairs_probs takes dense codes (one Lk, key_tail_rows = t and key_tail_weight = w for the whole
 * launch, as dl_pgca_pairs_fwd); dl_pgca_pairs_ragged_probs takes the packed row store and its device
 * table (kv_row0, kv_keys, kv_tail_weight, kv_total_rows, launch-wide key_tail_rows = t, as
 * dl_pgca_pairs_ragged_fwd: drug d has Lk_d keys whose last t stand for w_d identical keys each).
 * Both launch one kernel that differs only in where a workgroup finds its keys: on a store of
 * equal-length drugs with w_d = 1 and t = 0 they give the same bits.
 *
 * For pair n < n_pairs with p = q_index[n], d = kv_index[n] (int32, device memory), lead_d = Lk_d - t:
 *   P[r][k] = exp(scale Q[p]_r . K_d,k + log w_k - LSE_r)      (w_k = w_d on the last t keys, 1 elsewhere;
 *                                                               LSE_r over all keys with their weights)
 *   expand_tail == 0: out (n, r, k) = P[r][k], k < Lk_d — the softmax over the drug's DISTINCT keys; a tail
 *                     column carries the mass of the w_d keys it stands for (any w_d >= 1)
 *   expand_tail == 1: lead_d + t * w_d columns, the map over the FULL key set in the order the host's expansion
 *                     of the tail uses (ExpandTailFn, DrugLibrary.expand): column lead_d + i * t + j (i < w_d,
 *                     j < t) holds the probability of ONE copy of tail key j, exp(scale q.k_{lead_d+j} - LSE_r)
 *   columns from the drug's count up to out_cols - 1 are written as +0.0f: every row r < Lq of a valid pair is
 *   defined over all out_cols columns.
 * Addressing (element strides; Q / K dtype `dtype` with contiguous columns, out fp32):
 *   q    (e, r, :) = Q + e*q_es + r*q_rs          e < n_q
 *   K_d  (j, :)    = K + d*k_es + j*k_rs          j < Lk            (dense)
 *   K_d  (j, :)    = K + (kv_row0[d] + j)*k_rs    j < kv_keys[d]    (ragged)
 *   out  (n, r, c) = out + n*out_ps + r*out_rs + c     r < Lq, c < out_cols
 * Nothing is written at or beyond column out_cols, nothing outside the addressed rows; no row outside a pair's
 * segment is read for it.  No atomics on out: two calls agree bitwise.
 * A pair is skipped — nothing is read through its table entry, nothing is written for it — when
 *   its index is outside [0, n_q) or [0, n_kv)                           -> DL_FLAG_PAIR_INDEX is OR-ed into *flags
 *   its table entry is malformed (the conditions of dl_pgca_pairs_ragged_fwd) -> DL_FLAG_KEY_TABLE
 *   the drug's column count exceeds out_cols, or expand_tail is set (t > 0) and
 *   w_d is not a whole number <= 2^24                                       -> DL_FLAG_MAP_COLS
 * (flags may be NULL).  For the dense entry point the column count and the weight are known on the host and
 * checked there (DL_ERR_SHAPE / DL_ERR_ARG).
 * One head, head_dim == 128 (else DL_ERR_UNSUPPORTED); Lq arbitrary; Q / K 16-byte aligned with strides multiples of
 * 16 bytes; out 4-byte aligned, out_ps >= 0, out_rs >= out_cols > 0; 16-byte stores when out is 16-byte aligned and
 * out_ps, out_rs are multiples of 4, 4-byte stores otherwise; kv_row0 8-byte, the other index vectors 4-byte aligned;
 * expand_tail 0 or 1; key_tail_rows >= 0 (dense: <= Lk, key_tail_weight >= 1), kv_total_rows >= 0.
 * n_pairs == 0: DL_OK, nothing is launched, no pointer is looked at.
 * ------------------------------------------------------------------------------------------ */
typedef struct {
  const void* Q; const void* K; float* out;
  const int32_t* q_index; const int32_t* kv_index; uint32_t* flags;
  int64_t q_es, q_rs, k_es, k_rs, out_ps, out_rs;
  int32_t n_pairs, n_q, n_kv, Lq, Lk, head_dim, dtype;
  int32_t out_cols, expand_tail;
  float scale;
  int32_t key_tail_rows; float key_tail_weight;
} dl_pgca_pairs_probs_args;
int dl_pgca_pairs_probs(const dl_pgca_pairs_probs_args* a, dl_stream s);

typedef struct {
  const void* Q; const void* K; float* out;
  const int32_t* q_index; const int32_t* kv_index;
  const int64_t* kv_row0; const int32_t* kv_keys; const float* kv_tail_weight; uint32_t* flags;
  int64_t q_es, q_rs, k_rs, out_ps, out_rs, kv_total_rows;
  int32_t n_pairs, n_q, n_kv, Lq, head_dim, dtype;
  int32_t out_cols, expand_tail;
  float scale;
  int32_t key_tail_rows;
} dl_pgca_pairs_ragged_probs_args;
int dl_pgca_pairs_ragged_probs(const dl_pgca_pairs_ragged_probs_args* a, dl_stream s);

/* ------------------------------------------------------------------------------------------
 * Pair-indexed PGCA hit profiles: the two reductions of a probability map that interpretation asks for
 * (which drug keys receive a protein's attention; which sites attend sharply, and to what), computed
 * from the same operands as the maps above WITHOUT writing the map (csrc/pgca_pairs_profile.hip): about
 * 4 KB per pair instead of 512 KB.  dl_pgca_pairs_profile takes dense codes, dl_pgca_pairs_ragged_profile
 * the packed row store and its device table, exactly as dl_pgca_pairs_probs / dl_pgca_pairs_ragged_probs do;
 * both launch one kernel, and on a store of equal-length drugs they give the same bits.
 *
 * For pair n < n_pairs with p = q_index[n], d = kv_index[n], let P (Lq rows, F_d = lead_d + t * w_d columns)
 * be the map the entry points above define under expand_tail == 1 (copy i of tail key j at column
 * lead_d + i * t + j, every copy carrying exp(scale q.k_{lead_d+j} - LSE_r)):
 *   key_mass  (n, c) = (1 / Lq) sum_r P[r][c]     c < F_d; +0.0f for F_d <= c < out_cols   (sums to 1 over c)
 *   site_peak (n, r) = max_c P[r][c]              r < Lq
 *   site_key  (n, r) = the smallest column at which the computed P[r][.] attains that maximum.  Copies of a
 *                      tail key are equal and copy 0 comes first, so 0 <= site_key < Lk_d: an index into the
 *                      drug's STORED keys; a tail key competes with one copy's probability, not w_d times it.
 * Addressing (element strides; Q / K as above; key_mass and site_peak fp32, site_key int32):
 *   key_mass  (n, c) = key_mass  + n*mass_ps + c      c < out_cols
 *   site_peak (n, r) = site_peak + n*site_ps + r      r < Lq       (site_key: the same pitch)
 * Nothing else is written.  One launch, no workspace, no atomics on data: two calls agree bitwise.
 * A pair is skipped — nothing is read through its table entry, nothing is written to any of the three
 * outputs — when
 *   its index is outside [0, n_q) or [0, n_kv)                                -> DL_FLAG_PAIR_INDEX is OR-ed into *flags
 *   its table entry is malformed (the conditions of dl_pgca_pairs_ragged_fwd) -> DL_FLAG_KEY_TABLE
 *   F_d exceeds out_cols, w_d (t > 0) is not a whole number <= 2^24, or the
 *   drug has more than 576 stored keys                                        -> DL_FLAG_MAP_COLS
 * (flags may be NULL).  For the dense entry point these are known on the host and checked there (DL_ERR_SHAPE /
 * DL_ERR_ARG; Lk > 576: DL_ERR_UNSUPPORTED).
 * One head, head_dim == 128 (else DL_ERR_UNSUPPORTED); Lq arbitrary (one workgroup walks a pair's query blocks);
 * Q / K 16-byte aligned with strides multiples of 16 bytes; the outputs and index vectors 4-byte, kv_row0 8-byte
 * aligned; mass_ps >= out_cols > 0, site_ps >= Lq; key_tail_rows >= 0 (dense: <= Lk, key_tail_weight >= 1),
 * kv_total_rows >= 0; reserved == 0.  n_pairs == 0: DL_OK, nothing is launched, no pointer is looked at.
 * ------------------------------------------------------------------------------------------ */
typedef struct {
  const void* Q; const void* K; float* key_mass; float* site_peak; int32_t* site_key;
  const int32_t* q_index; const int32_t* kv_index; uint32_t* flags;
  int64_t q_es, q_rs, k_es, k_rs, mass_ps, site_ps;
  int32_t n_pairs, n_q, n_kv, Lq, Lk, head_dim, dtype;
  int32_t out_cols;
  float scale;
  int32_t key_tail_rows; float key_tail_weight;
  int32_t reserved;
} dl_pgca_pairs_profile_args;
int dl_pgca_pairs_profile(const dl_pgca_pairs_profile_args* a, dl_stream s);

typedef struct {
  const void* Q; const void* K; float* key_mass; float* site_peak; int32_t* site_key;
  const int32_t* q_index; const int32_t* kv_index;
  const int64_t* kv_row0; const int32_t* kv_keys; const float* kv_tail_weight; uint32_t* flags;
  int64_t q_es, q_rs, k_rs, mass_ps, site_ps, kv_total_rows;
  int32_t n_pairs, n_q, n_kv, Lq, head_dim, dtype;
  int32_t out_cols;
  float scale;
  int32_t key_tail_rows;
  int32_t reserved;
} dl_pgca_pairs_ragged_profile_args;
int dl_pgca_pairs_ragged_profile(const dl_pgca_pairs_ragged_profile_args* a, dl_stream s);

/* ------------------------------------------------------------------------------------------
 * Pair-indexed PGCA hit attributions: gradient x code of a target at the pair stage, per drug key and
 * per protein site, from the cached operands and the gradient of the pair's concat row, WITHOUT forming
 * dQ, dK or dV' (csrc/pgca_pairs_attr.hip).  dl_pgca_pairs_attr takes dense codes, dl_pgca_pairs_ragged_attr
 * the packed row store and its device table, exactly as the profile entry points do; both launch one
 * kernel, and on a store of equal-length drugs they give the same bits.
 *
 * K points at [K | V'] rows: V'_c is columns head_dim .. 2 head_dim - 1 of the row K_c (k_rs >= 2 head_dim).
 * For pair n < n_pairs with p = q_index[n], d = kv_index[n], w_c the multiplicity of stored key c (1 for
 * c < lead_d, w_d on the last t rows), dO (n, r, :) the gradient w.r.t. the attention output of row r:
 *   s[r,c]  = scale Q[p]_r . K_d,c          p[r,c] = exp(s[r,c]) / sum_c' w_c' exp(s[r,c'])
 *   g[r,c]  = dO[n]_r . V'_d,c              D[r]   = sum_c w_c p[r,c] g[r,c]       ds[r,c] = p[r,c] (g[r,c] - D[r])
 *   key_attr  (n, col) = sum_r (ds[r,c] s[r,c] + p[r,c] g[r,c])   one copy's value of stored key c, at every column
 *                        of the key's copies (copy i of tail key j at lead_d + i * t + j, as key_mass); +0.0f for
 *                        F_d <= col < out_cols.  It equals (dK_c . K_c + dV'_c . V'_c) / w_c.
 *   site_attr (n, r)   = sum_c w_c ds[r,c] s[r,c]  (+ d_sites (n, r, :) . sites (p, r, :) over left_cols columns when
 *                        sites / d_sites are given: both or neither)          r < Lq.  It equals dq_r . q_r (+ the left dot).
 * The tail bias log w enters the normaliser only, never the factor s[r,c].  All sums are fp32.
 * Addressing (element strides; every operand dtype `dtype` with contiguous columns; outputs fp32):
 *   q      (e, r, :) = Q + e*q_es + r*q_rs               K_d as in the profile entry points
 *   dO     (n, r, :) = dO + n*do_ps + r*do_rs            sites (e, r, :) = sites + e*left_es + r*left_rs
 *   d_sites(n, r, :) = d_sites + n*dl_ps + r*dl_rs
 *   key_attr (n, c)  = key_attr + n*mass_ps + c          site_attr (n, r) = site_attr + n*site_ps + r
 * Nothing else is written.  One launch, no workspace, no atomics on data: two calls agree bitwise.
 * A pair is skipped, with the flags and under the conditions of the profile entry points (more than 576 stored
 * keys included).  One head, head_dim == 128; Lq arbitrary; Q / K / dO / sites / d_sites 16-byte aligned with strides
 * multiples of 16 bytes, left_cols a multiple of 16 bytes; the outputs and index vectors 4-byte, kv_row0 8-byte
 * aligned; mass_ps >= out_cols > 0, site_ps >= Lq; reserved == 0.  n_pairs == 0: DL_OK, nothing is launched.
 * ------------------------------------------------------------------------------------------ */
typedef struct {
  const void* Q; const void* K; const void* dO; const void* sites; const void* d_sites; float* key_attr; float* site_attr;
  const int32_t* q_index; const int32_t* kv_index; uint32_t* flags;
  int64_t q_es, q_rs, k_es, k_rs, do_ps, do_rs, left_es, left_rs, dl_ps, dl_rs, mass_ps, site_ps;
  int32_t n_pairs, n_q, n_kv, Lq, Lk, head_dim, dtype;
  int32_t out_cols, left_cols;
  float scale;
  int32_t key_tail_rows; float key_tail_weight;
  int32_t reserved;
} dl_pgca_pairs_attr_args;
int dl_pgca_pairs_attr(const dl_pgca_pairs_attr_args* a, dl_stream s);

typedef struct {
  const void* Q; const void* K; const void* dO; const void* sites; const void* d_sites; float* key_attr; float* site_attr;
  const int32_t* q_index; const int32_t* kv_index;
  const int64_t* kv_row0; const int32_t* kv_keys; const float* kv_tail_weight; uint32_t* flags;
  int64_t q_es, q_rs, k_rs, do_ps, do_rs, left_es, left_rs, dl_ps, dl_rs, mass_ps, site_ps, kv_total_rows;
  int32_t n_pairs, n_q, n_kv, Lq, head_dim, dtype;
  int32_t out_cols, left_cols;
  float scale;
  int32_t key_tail_rows;
  int32_t reserved;
} dl_pgca_pairs_ragged_attr_args;
int dl_pgca_pairs_ragged_attr(const dl_pgca_pairs_ragged_attr_args* a, dl_stream s);


/* ------------------------------------------------------------------------------------------
 * MHLA token gate (MultiHeadLinearAttention.forward, model/PMMA/encoder.py:127-140):
 * logits [B][L][H] -> g = softmax over L (per b, per h); out = flat-reinterpreted product:
 * within sample b, flat index f = (j*L + l)*hd + c (j<H, hd = D/H) of the contiguous [L][D]
 * buffer is scaled by g[b][l][j].  (NOT a head split — the reference does a .view on the
 * contiguous (B,L,D) tensor.)  out = v * gate (+ v if add_residual, the caller's `mv + hv`).
 * bwd: dv, dlogits.
 * ------------------------------------------------------------------------------------------ */
int dl_token_gate_fwd(const void* v, const void* logits, void* out, float* gate_out, int64_t B,
                      int64_t L, int64_t D, int32_t H, int32_t add_residual, int32_t dtype,
                      dl_stream s);
int dl_token_gate_bwd(const void* dout, const void* v, const float* gate, void* dv, void* dlogits,
                      int64_t B, int64_t L, int64_t D, int32_t H, int32_t add_residual,
                      int32_t dtype, dl_stream s);
/* Gradient of MHLA's lin2 input through the GELU in front of it (encoder.py:127-140: logits = lin2(gelu(lin1 v))):
 * dpre[m][n] = gelu'(pre[m][n]) * sum_{h < H} dlogits[m][h] * w2[h][n], w2 = lin2.weight [H][d_diff] in the compute dtype.
 * An inner dimension of H = 8: one elementwise pass over `pre` instead of a zero-padded 64-deep GEMM (round 5). */
int dl_gate_dpre(const void* dlogits, const void* w2, const void* pre, void* dpre, int64_t M, int64_t d_diff, int32_t H,
                 int32_t dtype, dl_stream s);

/* ------------------------------------------------------------------------------------------
 * Stream concatenation of the PMMA encoder (model/PMMA/encoder.py:50: `cat((prot, mol), -1)` before
 * the self-attention layers) and its gradient.  src [S][R][row_bytes] -> dst [R][S * row_bytes];
 * inverse = 1 goes the other way (src [R][S * row_bytes] -> dst [S][R][row_bytes]).
 * ------------------------------------------------------------------------------------------ */
int dl_interleave_streams(const void* src, void* dst, int64_t R, int64_t row_bytes, int32_t S, int32_t inverse,
                          dl_stream s);
/* Symmetric-normalised, transposed adjacency of a batch of dense graphs: ahat[b][i][j] = din[i] * adj[b][j][i] * dout[j]
 * with clamped degrees^-1/2 (MolecularGCN: model/basic_model.py:137-153, 591-617 — dgl GraphConv norm='both').
 * adj (B, n, n) fp32, ahat (B, n, n) out_dtype; n <= 4096 (the adjacency tile sits in LDS up to n = 194). */
int dl_norm_adjacency(const float* adj, void* ahat, int64_t B, int32_t n, int32_t out_dtype, dl_stream s);
/* Neighbourhood aggregation of MolecularGCN on dense batched graphs (dgl GraphConv norm='both' `update_all(copy_u, sum)`,
 * model/basic_model.py:591-617): out[b][i][:] = sum_j A'[b][i][j] * feat[b][j][:] for the n real nodes (A' = ahat, or
 * ahat^T when transpose = 1: the gradient), out[b][i][:] = feat[b][i][:] for the virtual padding nodes n <= i < N (their
 * only edge is the self loop).  ahat (B, n, n) from dl_norm_adjacency, feat / out (B, N, C), all `dtype`; n <= 128, C = 128. */
int dl_graph_aggregate(const void* ahat, const void* feat, void* out, int64_t B, int32_t n, int32_t N, int32_t C,
                       int32_t transpose, int32_t dtype, dl_stream s);
/* cat[r] = [a[r] | b[r]] for two row-major buffers (model/DrugLAMP.py:57,66: `cat((prot_sites, guided), 2)` in front of
 * the MHLA blocks); inverse = 1 splits cat back into a and b (the gradient). */
int dl_concat2(void* a, void* b, void* cat, int64_t R, int64_t a_row_bytes, int64_t b_row_bytes, int32_t inverse,
               dl_stream s);

/* ------------------------------------------------------------------------------------------
 * Elementwise helpers on the path.
 * ------------------------------------------------------------------------------------------ */
/* y = dropout(x + pe[row % L]) — Embeddings.forward prot branch (model/PMMA/embed.py:51-52).  A p that rounds to a 16-bit
 * threshold of 0 (p == 0 or p < 2^-17) is no dropout: the plain sum, unscaled; dl_dropout_apply and dl_gemm do the same. */
int dl_add_rowmod_dropout(const void* x, const void* pe, void* y, int64_t M, int64_t D,
                          int64_t L, float p, uint64_t seed, const uint64_t* seed_offset, int32_t dtype, dl_stream s);
/* y = dropout_mask(seed)(x) / (1-p) — regenerates a forward mask for the backward pass.
 * seed_offset (here and above): DEVICE pointer or NULL, see dl_gemm_args.dropout_seed_offset. */
int dl_dropout_apply(const void* x, void* y, int64_t n_rows, int64_t D, int64_t ldx, int64_t ldy,
                     float p, uint64_t seed, const uint64_t* seed_offset, int32_t dtype, dl_stream s);
/* LLM feature ingest (input side of the path): ONE pass over the pre-extracted embedding tensor
 * x [B][S][F] produces the reference's fill bit (1 where the embedding row sums to exactly 0,
 * model/DrugLAMP.py:11-19) and the fill-bit-augmented, site-pooled features
 * pooled[b][j][:] = mean over the site_len chunks c of [x | fill][b][c*(S/site_len) + j][:]
 * (DrugLAMP.py:39-40; site_len = 1 just appends the fill bit), zero-padded to ceil8(F+1) columns so that
 * the adaptor GEMMs are aligned.  fill has x's dtype, pooled has out_dtype. */
int dl_fill_pool(const void* x, void* fill, void* pooled, int64_t B, int64_t S, int64_t F, int32_t site_len,
                 int32_t in_dtype, int32_t out_dtype, dl_stream s);
/* dx = dy * gelu'(pre) (exact-erf GELU): backward of the GELU that sits between a Linear and a LayerNorm in
 * the LLM adaptors (model/basic_model.py:189-193, DrugLAMP.py:46-52). */
int dl_gelu_bwd(const void* dy, const void* pre, void* dx, int64_t n, int32_t dtype, dl_stream s);
/* dst(bf16|f32) = src(f32|bf16) elementwise cast (weight casts, master fp32 -> compute dtype). */
int dl_cast(const void* src, int32_t src_dtype, void* dst, int32_t dst_dtype, int64_t n,
            dl_stream s);
/* Batch assembly of the pre-extracted LLM embeddings from a DEVICE-RESIDENT packed store (replaces the
 * reference's per-sample torch.load + host loops, handler/dataset.py:186-195 and utils.py:304-334):
 *   store   [total_rows][F]  every unique protein / drug embedding, rows of one entity contiguous
 *   offsets [B] first row of sample b's entity, lengths [B] its row count
 *   out     [B][S][F]:  repeat = 1 -> the entity's rows written floor(S / len) times back to back, zeros after
 *                                     (repeat_pad, utils.py:314-324: protein side, S = 9 * 256)
 *                       repeat = 0 -> rows 0 .. min(len, S) - 1, zeros after (tail_pad, utils.py:304-312: drug side, S = 512)
 * F * sizeof(dtype) must be a multiple of 16. */
int dl_gather_pad(const void* store, const int64_t* offsets, const int32_t* lengths, void* out, int64_t B,
                  int64_t S, int64_t F, int32_t repeat, int32_t dtype, dl_stream s);
/* ProteinCNN head (model/basic_model.py:168-171): out[b][halo + l][:D] = weight[ids[b][l]][:] (nn.Embedding row
 * gather), out[b][halo + l][D] = fill[b][l] (the concatenated fill bit); `halo` zero rows on each side of every
 * sample are the conv 'same' padding of this library's channel-last layout.  weight is passed PADDED to
 * [V][D + 1] (last column ignored; 16-byte aligned rows; the padded table must fit 64 KB of LDS, else DL_ERR_SHAPE);
 * fill [B][L] and out [B][L + 2*halo][D + 1]; all `dtype`. */
int dl_embed_pad(const int64_t* ids, const void* weight, const void* fill, void* out, int64_t B, int64_t L,
                 int32_t V, int32_t D, int32_t halo, int32_t dtype, dl_stream s);
/* Device-side guard flags (sticky bits OR-ed into a caller-owned uint32 word; the trainer polls it):
 * the compact forms below are only valid for inputs with the padding structure of the reference's collate. */
enum { DL_FLAG_PROT_PERIOD = 1, DL_FLAG_DRUG_TOKEN_PAD = 2, DL_FLAG_GCN_NODE_PAD = 4, DL_FLAG_PLAN_ROWS = 8,
       DL_FLAG_PAIR_INDEX = 16 /* dl_pgca_pairs_fwd: a pair's entity index is out of range (the pair was skipped) */,
       DL_FLAG_KEY_TABLE = 32 /* dl_pgca_pairs_ragged_fwd: a drug's key table entry is malformed (the pair was skipped) */,
       DL_FLAG_MAP_COLS = 64 /* dl_pgca_pairs_probs / _ragged_probs: a drug's map does not fit out_cols, or expand_tail met a
                                multiplicity that is no whole number <= 2^24 (the pair was skipped) */ };
/* ProteinCNN head on distinct rows (round 4; model/basic_model.py:168-171 over a sequence tiled by utils.py:392-412):
 * out[r][:D] = weight[ids[src[r]]], out[r][D] = fill[src[r]] for src[r] >= 0 (a flat index into ids / fill [B * L]), a zero
 * row for src[r] < 0.  weight padded to [V][D + 1] as for dl_embed_pad.  With `period` [B] given the same launch checks
 * every sample's (id, fill bit) sequence: equal at distance period[b] inside the last whole period's end E, constant on
 * [E, L) — what the row tables assume; a violation ORs DL_FLAG_PROT_PERIOD into *flags.  period[b] == 0: sample b's tables
 * keep every position (no periodic claim), nothing is checked for it. */
int dl_embed_rows(const int64_t* ids, const void* weight, const void* fill, const int32_t* src, void* out, int64_t R,
                  int32_t V, int32_t D, const int32_t* period, int64_t B, int64_t L, uint32_t* flags, int32_t dtype, dl_stream s);
/* out[i][:] = src[index[i]][:] (zeros where index[i] < 0), rows of row_bytes (a multiple of 16): the compact ProteinCNN
 * output expanded to all positions (the reference's full (B, 2304, 128) activation, basic_model.py:179). */
int dl_rows_gather(const void* src, const int32_t* index, void* out, int64_t N, int64_t row_bytes, dl_stream s);
/* out[r][:] = sum_{k < rep[r][2]} x[rep[r][0] + k * rep[r][1]][:] — the gradient of dl_rows_gather for index maps whose
 * preimages are arithmetic progressions (rep = (first, stride, count) per output row; count 0 gives a zero row); fixed
 * summation order, fp32 accumulation. */
int dl_rows_sum_strided(const void* x, const int32_t* rep, void* out, int64_t R, int64_t C, int32_t dtype, dl_stream s);
/* Guard of the drug branch's compact padding forms (reference handler/dataset.py:211-222 virtual nodes; utils.py:304-312
 * tail_pad zero rows): rows row0 .. N - 1 of every sample of x [B][N][row_bytes] must equal row row0 of sample 0 bit for bit,
 * else `code` is OR-ed into *flags. */
int dl_rows_equal_check(const void* x, int64_t B, int64_t N, int64_t row_bytes, int64_t row0, uint32_t code, uint32_t* flags,
                        dl_stream s);
/* The row tables of the ProteinCNN distinct-row layout, built on the device from the batch's residue counts (round 5).  The
 * reference tiles a protein of Lr residues with period P = Lr + 2 up to S positions (utils.py:392-412,
 * repeat_integer_label_protein) and the three 'same' convolutions (model/basic_model.py:155-180) see 7 positions to the left and
 * 8 to the right, so a sample has ~P + 31 distinct output rows; druglamp_amd/protein_plan.py states which (segments A / B / C,
 * halo rows, multiplicities) and builds the same tables on the host — the two are compared entry by entry in the tests.
 * lengths [B] int32 residue counts; R = row capacity of the tables (>= the rows the batch needs: rows behind them become
 * padding rows; fewer ORs DL_FLAG_PLAN_ROWS into *flags and writes nothing for the samples that do not fit);
 * src [R] flat input index or -1, w [R] -1 halo / 0 context / multiplicity, rep [R][3] (first, stride, count),
 * row_of [B * S] representative row of every position, period [B] (0 for samples kept in the plain layout). */
int dl_protein_plan_build(const int32_t* lengths, int64_t B, int64_t S, int64_t R, int32_t* src, float* w, int32_t* rep,
                          int32_t* row_of, int32_t* period, uint32_t* flags, dl_stream s);
/* ProteinCNN tail (model/basic_model.py:176-179 + DrugLAMP.py:39-40): the reference keeps the conv output
 * channel-first (B, C, L), REINTERPRETS that buffer with .view(B, L, C) and then site-pools it
 * (.view(B, site_len, n_site, C).mean(1)).  z is this library's channel-last conv output with `halo` zero rows
 * around every sample, [B][L + 2*halo][C]; pooled is [B][L / site_len][C].  fwd reproduces view + mean exactly in
 * one pass over z; bwd writes the full padded gradient dz (halo rows zeroed) from dpooled.  bf16 only.
 * site_len 1 (the masked-LM pass, model/self_supervised_learning.py:67-101: the reinterpretation alone) is a per-sample matrix
 * transpose and runs as one (64 x 64 tiles through LDS) when L and C are multiples of 64. */
int dl_cnn_sitepool_fwd(const void* z, void* pooled, int64_t B, int64_t L, int64_t C, int32_t halo,
                        int32_t site_len, int32_t dtype, dl_stream s);
int dl_cnn_sitepool_bwd(const void* dpooled, void* dz, int64_t B, int64_t L, int64_t C, int32_t halo,
                        int32_t site_len, int32_t dtype, dl_stream s);
/* The same through the row map of the distinct-row layout (round 4, druglamp_amd/protein_plan.py): z is the COMPACT conv
 * output [R][C]; position (b, l) is represented by row row_of[b * L + l].  fwd reads the pooling's operands through the map
 * (no expansion to [B][L][C]); bwd writes the compact gradient dz [R][C] directly: a row's gradient is the sum over the
 * positions it stands for (rep[r] = (first flat position, stride, count), count 0 = a zero row).  bf16 only. */
int dl_cnn_sitepool_rows_fwd(const void* z, const int32_t* row_of, void* pooled, int64_t B, int64_t L, int64_t C,
                             int32_t site_len, int32_t dtype, dl_stream s);
int dl_cnn_sitepool_rows_bwd(const void* dpooled, const int32_t* rep, const int32_t* row_of, void* dz, int64_t B, int64_t L,
                             int64_t C, int64_t R, int32_t site_len, int32_t dtype, dl_stream s);
/* Weight preparation: ONE launch refreshes every compute-dtype (and transposed) image of the fp32 master
 * parameters after an optimiser step — the per-parameter `.to(dtype)` / `.t().contiguous()` / `cat(q,k,v)` copies
 * a torch implementation of the reference's modules makes implicitly, batched.  items / block_map are DEVICE
 * arrays built once by the host: block_map[2b] = item index, block_map[2b+1] = 64x64 tile index in that item.
 * plain item (transpose = 0): dst[(row0 + r) * ld + c] = src[r][c];   transposed item (1): dst[c * ld + row0 + r] = src[r][c];
 * strided item (2, round 3): dst[row0 + r * ld + c * cs] = src[r][c] with any (also negative) column stride — the GEMM
 * layouts of a Conv1d weight [co][ci][k] (one item per output channel: forward Wg[co][j*ci + c] = w[co][c][j], data
 * gradient Wd[ci][j'*co + o] = w[o][ci][k-1-j']), which torch derived with flip / permute / contiguous / cast launches. */
typedef struct dl_wprep_item {
  const float* src;        /* fp32 master parameter, [rows][cols] contiguous */
  void* dst;               /* image base (out_dtype) */
  int64_t ld;              /* image leading dimension in elements (strided items: row stride) */
  int32_t rows, cols;
  int32_t row0;            /* offset of this parameter inside a concatenated image (strided items: element offset) */
  int32_t transpose;       /* 0 plain, 1 transposed, 2 strided */
  int64_t cs;              /* strided items: column stride in elements */
} dl_wprep_item;
int dl_weight_prep(const dl_wprep_item* items_dev, const int32_t* block_map_dev, int32_t n_blocks,
                   int32_t out_dtype, dl_stream s);
/* out[d] (+)= sum over rows r of x[r][d] where rows are grouped by (r % L): pe gradients. */
int dl_rowmod_sum(const void* x, float* out, int64_t M, int64_t D, int64_t L, int32_t accumulate,
                  int32_t dtype, dl_stream s);

/* ------------------------------------------------------------------------------------------
 * Loss kernels.
 * cos_rowloss: SimSiam loss_fn (model/self_supervised_learning.py:184-187):
 *   per row r: 2 - 2*cos(x_r, y_r); out_sum (+)= sum_r.  bwd gives dx (y is a detached target).
 * ntxent_stream: nt_xent_loss (self_supervised_learning.py:168-182): P = [q;k] (2n x d),
 *   logits = P P^T / T with the diagonal removed, positive of i is i+n (mod 2n), loss = sum CE / 2n,
 *   computed by streaming tiles with an online log-sum-exp; never materialises (2n)^2.
 * triplet_sigcos: ccpp_p_tri_loss (model/cross_modality.py:15-47) with distance
 *   1 - sigmoid(cos) (utils.py:571-574): all-pairs sigmoid(cos) matrix once, then the masked
 *   triplet reduction over the label matrix gt[n_p][n_d] (1 positive, 0 negative, -1 ignore).
 * ------------------------------------------------------------------------------------------ */
int dl_cos_rowloss_fwd(const float* x, const float* y, float* row_loss, float* loss_sum,
                       int64_t n_rows, int64_t D, dl_stream s);
int dl_cos_rowloss_bwd(const float* x, const float* y, float grad_scale, float* dx, int64_t n_rows,
                       int64_t D, dl_stream s);
/* Cross entropy over rows with few classes (round 5): F.cross_entropy(logits (N, C), labels, ignore_index) of the masked-LM
 * heads (model/self_supervised_learning.py:93-99; N = batch x 2304 tokens, C = 27).  logits [N][ld] (fp32 / bf16; ld >= C: the
 * GEMM in front pads the row), labels int64 [N].  fwd: lse [N] (log-sum-exp per row, kept for bwd), out2[0] = mean loss over the
 * rows whose label is not ignore_index, out2[1] = their number; fixed summation order.  As torch: NaN when no row is counted
 * (0 / 0); a label outside [0, C) other than ignore_index (torch: device-side assert) poisons the loss with NaN — never skipped silently.  bwd: dlogits [N][ldd],
 * columns < Cp written (softmax - onehot) * grad_out[0] / out2[1] for counted rows, zeros elsewhere; grad_out is a DEVICE scalar. */
size_t dl_ce_rows_workspace_bytes(int64_t N);
int dl_ce_rows_fwd(const void* logits, int64_t ld, const int64_t* labels, int64_t N, int32_t C, int64_t ignore_index, int32_t dtype,
                   float* lse, float* out2, void* workspace, size_t workspace_bytes, dl_stream s);
int dl_ce_rows_bwd(const void* logits, int64_t ld, const int64_t* labels, int64_t N, int32_t C, int64_t ignore_index, int32_t dtype,
                   const float* lse, const float* out2, const float* grad_out, void* dlogits, int64_t ldd, int32_t Cp, dl_stream s);
/* Imbalance-aware classification loss (cls_loss.hip): weighted / focal binary cross entropy on the classifier's logits.
 * score [N][ld] (fp32 / bf16, ld >= n_out), labels fp32 [N] in [0, 1], weights fp32 [N] or NULL (every weight 1).  Row i:
 *   z = score[i][0] (n_out == 1) or score[i][1] - score[i][0] (n_out == 2),  p = sigmoid(z),  y = labels[i],  w = weights[i],
 *   d = |y sigmoid(-z) - (1 - y) sigmoid(z)| (= |y - p|, without cancellation in the tails),  m = d^gamma (gamma == 0: 1),
 *   l = w m [a_pos y softplus(-z) + a_neg (1 - y) softplus(z)],   softplus(t) = max(t, 0) + log1p(exp(-|t|)).
 * fwd: probs[i] = p (probs may be NULL), out2[0] = sum_i l / den, out2[1] = den; den = N without weights, the sum of the valid
 * weights with (den == 0: NaN, 0 / 0).  bwd: dscore [N][ldd] in score's dtype, g = grad_out[0] / out2[1] * d l / d z in the one
 * column, (-g, +g) in two; the full derivative, d m / d z = -gamma d^(gamma - 1) sgn(y - p) p (1 - p) with sgn(0) = 0; recomputed
 * from z, nothing is saved per row; grad_out is a DEVICE scalar and out2 the forward's.  Columns >= n_out are not written.
 * a_pos, a_neg finite, >= 0, not both 0; gamma == 0 or 1 <= gamma <= 8 (else DL_ERR_ARG).  a_pos = pw, a_neg = 1, gamma = 0 is
 * BCE-with-logits with pos_weight pw; a_pos = alpha, a_neg = 1 - alpha is the focal loss; (1, 1, 0) on two outputs is the
 * two-class cross entropy.
 * Forms: N <= 4096 rows — one 256-thread workgroup does rows, sum and division in ONE launch and needs no workspace
 * (dl_cls_loss_workspace_bytes returns 0, workspace may be NULL); above, one row per thread with a pair of partial sums per
 * 256 rows in the workspace and a final one-workgroup launch.  The backward is one launch.  Fixed summation order, no
 * floating-point atomics: bitwise repeatable.
 * Bad inputs: a non-finite z makes that row's loss term and gradient NaN (so the loss is NaN; probs is sigmoid(z) by IEEE
 * rules: 1, 0, NaN for +inf, -inf, NaN); a label outside [0, 1] or not finite, or a weight that is negative or not finite,
 * poisons its row the same way and ORs `code` into *flags (a caller-owned word, as for dl_rows_equal_check; flags may be NULL).
 * A bad weight counts 0 in den, so the other rows keep their gradient. */
size_t dl_cls_loss_workspace_bytes(int64_t N);
int dl_cls_loss_fwd(const void* score, int64_t ld, int32_t n_out, int32_t dtype, const float* labels, const float* weights, int64_t N,
                    float a_pos, float a_neg, float gamma, float* probs, float* out2, void* workspace, size_t workspace_bytes,
                    uint32_t code, uint32_t* flags, dl_stream s);
int dl_cls_loss_bwd(const void* score, int64_t ld, int32_t n_out, int32_t dtype, const float* labels, const float* weights, int64_t N,
                    float a_pos, float a_neg, float gamma, const float* out2, const float* grad_out, void* dscore, int64_t ldd,
                    dl_stream s);
/* General form (round 3): the rows whose loss / gradient a call produces (side `a`, resident) are scored against a second
 * set of rows (side `b`, streamed); each side is [q rows ; k rows], n rows per half, row-major (n x d), dtype DL_F32 or
 * DL_BF16 (bf16 operands on v_mfma_f32_16x16x32_bf16, log-sum-exp / loss / gradients in fp32).  Rows are identified
 * by their index in the GLOBAL batch: row r of a side's q half is gid_offset + r, of its k half n_global + gid_offset + r;
 * a row's positive is the same sample in the other half, its own column is excluded (the reference removes the diagonal,
 * self_supervised_learning.py:172-176).  One process: a = b = {q, k, n, 0}, n_global = n (what dl_ntxent_fwd / _bwd do).
 * Data parallel (north star: the contrastive denominator sees the global batch; the reference is rank-local): a = this
 * rank's rows {q_loc, k_loc, n, rank * n}, b = the all-gathered rows {q_all, k_all, world * n, 0}, n_global = world * n.
 *   dl_ntxent_fwd_ex: row_lse[2 a.n], row_loss[2 a.n] (= lse_i - logit(i, positive)), *loss (optional) = mean row_loss.
 *   dl_ntxent_bwd_ex: da_q, da_k (fp32, a.n x d) = grad_scale / T * sum_j w_ij b_j with
 *     w_ij = [a.lse] softmax_i(j) + [b.lse] softmax_j(i) - (#lse given) [j positive of i]; a.lse / b.lse = that side's
 *     row_lse from the forward call, or NULL if the side's rows are not softmax rows of this call.  Both given = the
 *     whole gradient of the single-process loss in one pass; the data-parallel path calls it twice (local rows with
 *     their lse against the gathered rows, and the gathered rows against the local rows with their lse: the latter is
 *     the key-side gradient that a reduce-scatter returns to its owners). */
typedef struct dl_ntxent_side {
  const void* q;          /* n x d rows of the first half */
  const void* k;          /* n x d rows of the second half */
  int64_t n;
  int64_t gid_offset;
  const float* lse;       /* backward only; 2 n floats or NULL */
} dl_ntxent_side;
typedef struct dl_ntxent_args {
  dl_ntxent_side a, b;
  int64_t n_global;
  int64_t d;              /* 64 or 128 */
  int32_t dtype;          /* DL_F32 | DL_BF16, both sides */
  float temperature;
} dl_ntxent_args;
int dl_ntxent_fwd_ex(const dl_ntxent_args* a, float* row_lse, float* row_loss, float* loss, dl_stream s);
int dl_ntxent_bwd_ex(const dl_ntxent_args* a, float grad_scale, float* da_q, float* da_k, dl_stream s);
size_t dl_ntxent_workspace_bytes(int64_t n, int64_t d);
int dl_ntxent_fwd(const float* q, const float* k, int64_t n, int64_t d, float temperature,
                  float* loss, float* row_lse, void* workspace, size_t workspace_bytes,
                  dl_stream s);
int dl_ntxent_bwd(const float* q, const float* k, int64_t n, int64_t d, float temperature,
                  const float* row_lse, float grad_out, float* dq, float* dk, dl_stream s);
/* Dot-product top-M (latent_topk.hip): for each of the P query rows q (P x 256, row-major) the M library rows of lib
 * (D x 256) with the largest 256-term dot product, without a (P, D) matrix.  q and lib both DL_F32 (exact
 * v_mfma_f32_16x16x4_f32) or both DL_BF16 (v_mfma_f32_16x16x32_bf16), fp32 accumulation in one fixed order: s(p, d) has the
 * same bits whatever P, D, M, slab and the pair's place in a tile.  Nothing is normalised.
 *   values[P][M] fp32, indices[P][M] int32: value descending, equal values by ascending index, at the cut the lower index
 *   wins; a NaN score ranks above every number (torch.topk's order), NaNs by ascending index.  Deterministic.
 *   slab: library rows per workgroup pass, a positive multiple of 64, or 0 for the host's choice (the library is split over
 *   ceil(D / slab) workgroups per 64-row query tile; a second kernel merges their lists).  The result does not depend on it.
 *   workspace: dl_latent_topk_workspace_bytes(P, D, M, slab) bytes (0 for arguments dl_latent_topk rejects), 8-byte aligned:
 *   per (query tile, slab, row) CAP = pow2(2 M + 64), clamped to [128, 2048], candidate keys of 8 bytes.
 * Before anything is launched: a null pointer, P < 1, M outside [1, min(D, 1024)], a bad dtype or slab: DL_ERR_ARG; D outside
 * [1, 2^31) or more workgroups than one grid: DL_ERR_SHAPE; q / lib not 16-byte aligned, values / indices not 4-byte aligned:
 * DL_ERR_ALIGN; a null, misaligned or short workspace: DL_ERR_WORKSPACE.  Two launches on stream s, no host synchronisation.
 * (The workspace pair FOLLOWS the stream here: tests/test_stream_contract_gpu.py lists the stream-last entries against its own
 * case table; this entry's stream contract is pinned by tests/test_latent_topk_gpu.py with the same procedure.) */
size_t dl_latent_topk_workspace_bytes(int64_t P, int64_t D, int32_t M, int64_t slab);
int dl_latent_topk(const void* q, const void* lib, int64_t P, int64_t D, int32_t M, int32_t dtype, int64_t slab,
                   float* values, int32_t* indices, dl_stream s, void* workspace, size_t workspace_bytes);
/* `dist` must hold dl_triplet_sigcos_buffer_floats(n_p, n_d) floats: the (n_p x n_d) distance matrix
 * first, then scratch that dl_triplet_sigcos_bwd reuses (pass the same buffer). */
size_t dl_triplet_sigcos_buffer_floats(int64_t n_p, int64_t n_d);
int dl_triplet_sigcos_fwd(const float* p_lats, const float* d_lats, const int8_t* gt, int64_t n_p,
                          int64_t n_d, int64_t dim, float margin, float* dist, float* loss,
                          float* n_tri, dl_stream s);
int dl_triplet_sigcos_bwd(const float* p_lats, const float* d_lats, const int8_t* gt,
                          const float* dist, int64_t n_p, int64_t n_d, int64_t dim, float margin,
                          const float* n_tri, float grad_out, float* dp, float* dd, dl_stream s);

/* ------------------------------------------------------------------------------------------
 * Fused AdamW over a flat fp32 parameter arena (torch.optim.AdamW semantics, decoupled weight
 * decay, bias correction; trainer.py:225-229 steps up to three of these per batch).
 * step is the 1-based step count AFTER increment.  Optionally emits a compute-dtype copy.
 * DL_ERR_ARG before anything is launched: a null pointer, n <= 0, step < 1, n beyond one grid (2^31 - 1 workgroups of 1024
 * elements); the same holds for dl_adamw_step_guarded and dl_adamw_step_groups below.
 * ------------------------------------------------------------------------------------------ */
int dl_adamw_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                  float lr, float beta1, float beta2, float eps, float weight_decay, int64_t step,
                  float grad_scale, void* param_lowp, int32_t lowp_dtype, dl_stream s);

/* ------------------------------------------------------------------------------------------
 * Gradient guard: global-norm clipping and the non-finite step skip, decided on the device (the host never reads
 * the norm; the optimiser kernel reads the decision).  Per step: dl_grad_sqnorm once per contiguous gradient run (the
 * first with accumulate = 0), dl_grad_guard_finalize once, dl_adamw_step_guarded for every optimiser launch.
 *
 * dl_grad_sqnorm: acc[0] = (accumulate ? acc[0] : 0) + sum_i g[i]^2 over n fp32 values, n > 0 arbitrary, g 16-byte
 *   aligned, acc and workspace 8-byte aligned.  Every square and every sum is fp64 (the square of an fp32 value is exact
 *   in fp64 and never overflows it), so a gradient of finite values gives a finite sum whatever its magnitude, and a NaN
 *   or an infinity anywhere gives a non-finite sum.  No atomics: one partial per workgroup stored into the workspace, a
 *   one-workgroup second launch sums them in a fixed order; the result is a function of the values, n and accumulate
 *   alone, and two calls agree bit for bit.  The relative error against the exact sum is at most n * 2^-53.
 *   workspace_bytes >= 8 * min(2048, ceil(n / 4096)) (fewer are used for some n; the contents need no initialisation
 *   and mean nothing afterwards).
 * dl_grad_guard_finalize (one thread): with norm = pre_scale * sqrt(acc[0]) in fp64 and nonfinite = !isfinite(acc[0]),
 *   skip     = nonfinite && skip_nonfinite
 *   coef     = max_norm <= 0 ? 1 : min(1, max_norm / (norm + 1e-6)) in fp64 (torch.nn.utils.clip_grad_norm_; a NaN norm
 *              gives a NaN coefficient, as torch's clamp does with error_if_nonfinite=False)
 *   guard[0] = skip ? 0 : (float)coef      guard[1] = (float)norm (may round to +inf for a finite gradient; coef does not)
 *   guard[2] = skip ? 1 : 0                guard[3] = 0 (reserved)
 *   counters[0] += skip                    counters[1] += (coef < 1 && !skip)       (cumulative, owned by the caller)
 *   guard: 4 floats, 16-byte aligned; counters: 2 int64; acc 8-byte aligned.
 * dl_adamw_step_guarded: dl_adamw_step with the gradient scale (float)(grad_scale * guard[0]) — the same arithmetic, the
 *   same bits as dl_adamw_step called with that scale — and when guard[2] != 0 nothing is written: param, exp_avg,
 *   exp_avg_sq and param_lowp keep their bits.  The host-side step count is the caller's business either way.
 * All three: null pointers, n <= 0, step < 1, a misaligned pointer and a workspace that is too small return DL_ERR_ARG
 * before anything is launched.
 * ------------------------------------------------------------------------------------------ */
int dl_grad_sqnorm(const float* g, int64_t n, double* acc, int32_t accumulate, void* workspace, int64_t workspace_bytes,
                   dl_stream s);
int dl_grad_guard_finalize(const double* acc, float pre_scale, float max_norm, int32_t skip_nonfinite, float* guard,
                           int64_t* counters, dl_stream s);
int dl_adamw_step_guarded(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                          float lr, float beta1, float beta2, float eps, float weight_decay, int64_t step,
                          float grad_scale, void* param_lowp, int32_t lowp_dtype, const float* guard, dl_stream s);

/* ------------------------------------------------------------------------------------------
 * Fused AdamW with parameter groups: a learning-rate scale and a weight decay per group, the group looked up on the device
 * per 16-byte chunk, so that one launch serves a run of parameters of mixed groups.
 *
 * dl_adamw_step_groups: quad_group holds ceil(n / 4) bytes, quad_group[q] = the group id k of elements 4q .. 4q+3 (the flat
 *   arena pads every parameter to a multiple of 4 elements: a chunk belongs to one parameter); group_tab holds n_groups rows
 *   of 2 floats {lr_scale, weight_decay}.  The chunk is updated by dl_adamw_step's arithmetic (csrc/optim.hip: the three
 *   dl_adamw_step* entry points launch one kernel, adamw_kernel, from one host launcher) with lr_k = lr * group_tab[2k],
 *   ONE fp32 multiply, and weight_decay = group_tab[2k + 1].
 *   Bit contract: for every maximal segment of equal group id, param, exp_avg, exp_avg_sq and param_lowp hold the bits of
 *   dl_adamw_step (guard null) / dl_adamw_step_guarded (guard given) called on that segment alone with lr = (float)lr *
 *   (float)lr_scale and that weight decay.
 *   guard: null, or the 16-byte {coef, norm, skip, 0} record of dl_grad_guard_finalize: the gradient scale is
 *   (float)(grad_scale * guard[0]), and when guard[2] != 0 nothing is written (one 16-byte load at a wave-uniform address,
 *   return before any other access, as dl_adamw_step_guarded).
 *   A chunk whose id is >= n_groups is not touched: its table row is not read and nothing of it is written (memory safety
 *   against a bad table; druglamp_amd.param_groups never builds one).  lr_scale = 0 is NOT freezing: the moments move and
 *   p * (1 - 0 * wd) - 0 * (m / denom) turns a -0.0 parameter into +0.0.
 *   16-byte loads and stores with a scalar tail for n % 4; one 16-byte chunk per thread, the grid a function of n alone; no
 *   atomics, no LDS: two calls on the same data agree bit for bit.  28.25 B per element (28 of AdamW + the id byte per chunk).
 *   DL_ERR_ARG before anything is launched: null param / grad / exp_avg / exp_avg_sq / quad_group / group_tab, n <= 0,
 *   step < 1, n_groups outside [1, 64], guard not 16-byte aligned.
 * ------------------------------------------------------------------------------------------ */
int dl_adamw_step_groups(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                         float lr, float beta1, float beta2, float eps, int64_t step, float grad_scale,
                         void* param_lowp, int32_t lowp_dtype, const uint8_t* quad_group, const float* group_tab,
                         int32_t n_groups, const float* guard, dl_stream s);

/* ------------------------------------------------------------------------------------------
 * Weight EMA: a shadow copy of the flat parameter arena moved towards the live parameters, one pass per training step.
 *
 * dl_ema_update: for every i < n, in fp32,
 *     d = param[i] - ema[i];   ema[i] = (d == 0) ? ema[i] : fmaf(weight, d, ema[i])
 *   — the lerp form e + w (p - e): one rounding of the difference, one of the fma, so |result - exact| <=
 *   3 * 2^-24 * max(|ema[i]|, |param[i]|) for weight in [0, 1].  ema[i] == param[i] is a fixed point BIT FOR BIT for any
 *   weight (parameters that received no gradient and arena padding keep their bits); the explicit d == 0 case is what
 *   extends that to a pair of negative zeros, where the fma alone would give +0.  param is never written.
 *   guard: null, or the 16-byte {coef, norm, skip, 0} record of dl_grad_guard_finalize; when guard[2] != 0 nothing is
 *   written (one 16-byte load at a wave-uniform address, return before any other access, as dl_adamw_step_guarded).
 *   Non-finite values pass through as the arithmetic says: a NaN parameter makes that element NaN, +-inf against a finite
 *   average makes +-inf (NaN at weight 0: 0 * inf), inf against the same inf makes NaN (inf - inf).
 *   16-byte loads and stores with a scalar tail for n % 4; one 16-byte chunk per thread, the grid a function of n alone; no
 *   atomics, no LDS: two calls on the same data agree bit for bit.
 *   DL_ERR_ARG before anything is launched: null ema or param, n <= 0, ema / param / guard not 16-byte aligned, weight not
 *   a finite value in [0, 1], ema == param.
 * ------------------------------------------------------------------------------------------ */
int dl_ema_update(float* ema, const float* param, int64_t n, float weight, const float* guard, dl_stream s);

/* ------------------------------------------------------------------------------------------
 * Kernel timing hooks used by bench.py for the roofline object: when enabled for a kernel
 * family, launches are bracketed by hipEventRecord on their own stream.
 * family: 0 gemm, 1 attn_fwd, 2 attn_bwd, 3 layernorm, 4 (unused since round 4), 5 ntxent_fwd, 6 ntxent_bwd.
 * These event lists are the library's ONLY process-global state; they exist while a family is enabled and are
 * never touched otherwise (dl_prof_enable(family, 0) frees them).
 * dl_prof_enable(family, on): on = 0 off; on = N >= 1 times one launch in N of the family, picked by a hash
 * of the launch index so that no launch slot of a periodic step is favoured (an
 * event pair costs ~6 us of stream time on gfx950: N = 1 times everything, a larger N keeps the
 * measurement from slowing the step it measures).
 * dl_prof_collect synchronises the recorded events and returns, over the TIMED launches,
 * launches / total ms / total algorithmic flops / total algorithmic bytes since dl_prof_enable.
 * dl_prof_totals returns the count and algorithmic work of ALL launches of the family since
 * dl_prof_enable, timed or not.
 * Algorithmic bytes of a dl_gemm launch: every DISTINCT operand byte once (an operand whose row pitch is smaller than
 * its row length — the implicit-im2col convolutions — spans (rows - 1) * pitch + length elements), the output, and
 * the epilogue's extra operands (pre_out, dact_pre, residual, bias, the read-back of an accumulating output).
 * ------------------------------------------------------------------------------------------ */
int dl_prof_enable(int32_t family, int32_t on);
int dl_prof_collect(int32_t family, int64_t* launches, double* total_ms, double* total_flops,
                    double* total_bytes);
int dl_prof_totals(int32_t family, int64_t* launches, double* total_flops, double* total_bytes);
/* The same per sub-family tag (dl_gemm_args.prof_tag) of a family: the timed launches' count / ms / algorithmic flops /
 * algorithmic bytes, and the count / flops / bytes of ALL the tag's launches since dl_prof_enable. */
int dl_prof_collect_tag(int32_t family, int32_t tag, int64_t* timed_launches, double* timed_ms, double* timed_flops,
                        double* timed_bytes, int64_t* all_launches, double* all_flops, double* all_bytes);

#ifdef __cplusplus
}
#endif
#endif /* DRUGLAMP_HIP_H */
