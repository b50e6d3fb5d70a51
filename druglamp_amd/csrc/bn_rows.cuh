// bn_rows.cuh — what bn.hip and bn_eval.hip share: the chunking rule of the partial-sum kernels (and with it the workspace
// size), the row rule, the shared tails of the partial-sum kernels, the wide-form predicate and dispatch, the second-stage
// launch and the argument checks of the dl_bn_* entry points.
#pragma once
#include <type_traits>
#include "common.cuh"

namespace {
// ---- chunking: a partial-sum kernel runs grid (ceil(C/256), chunks), workgroup y owns rows [y * rows, (y + 1) * rows) and
// writes partial[y][2][C].  dl_bn_workspace_bytes and every launcher take both numbers from here.
struct BnChunks {
  int rows, chunks;
};
static inline BnChunks bn_chunks(int64_t R, int64_t C) {
  const int64_t colgroups = (C + 255) / 256;
  const int64_t want = (1024 + colgroups - 1) / colgroups;
  int64_t rows = (R + want - 1) / want;
  if (rows < 32) rows = 32;
  rows = (rows + 3) / 4 * 4;
  return BnChunks{(int)rows, (int)((R + rows - 1) / rows)};
}
static inline size_t bn_workspace_bytes(int64_t R, int64_t C) { return (size_t)bn_chunks(R, C).chunks * 2 * (size_t)C * sizeof(float); }
static inline dim3 bn_partial_grid(int64_t C, const BnChunks& ck, bool wide) {
  return wide ? dim3(1, (uint32_t)ck.chunks) : dim3((uint32_t)((C + 255) / 256), (uint32_t)ck.chunks);
}

// ---- the row rule.  rw == nullptr: the window rule (inside every `win` rows the rows [halo, halo + valid) take part, weight
// 1; win == 0: every row); else rw[r] is the row's weight: < 0 halo row (excluded, written as zeros), 0 context row (computed,
// not part of the statistics), m >= 1 a row that stands for m identical rows (the ProteinCNN compact layout,
// druglamp_amd/protein_plan.py).  -1 = excluded.
// The modulo is 32-bit on purpose: a 64-bit one costs ~100 instructions and this runs once per row per thread (the host checks
// R < 2^31 and win < 2^31: bn_check_rows31 / bn_check_window).
__device__ __forceinline__ bool bn_window_row(int64_t r, int64_t win, int64_t halo, int64_t valid) {
  if (win == 0) return true;
  const uint32_t q = (uint32_t)r % (uint32_t)win;
  return q >= (uint32_t)halo && q < (uint32_t)(halo + valid);
}
__device__ __forceinline__ float bn_row_weight(const float* __restrict__ rw, int64_t r, int64_t win, int64_t halo, int64_t valid) {
  if (rw) return rw[r];
  return bn_window_row(r, win, halo, valid) ? 1.f : -1.f;
}
// bn_row_weight(..) >= 0 for the kernels that want no more than that (spelled out: the generic kernel of bn_eval.hip compiles
// to other code through the float)
__device__ __forceinline__ bool bn_row_in(const float* __restrict__ rw, int64_t r, int64_t win, int64_t halo, int64_t valid) {
  if (rw) return rw[r] >= 0.f;
  return bn_window_row(r, win, halo, valid);
}

// ---- the end of a partial-sum kernel: the workgroup's (s0 | s1) -> partial[blockIdx.y][2][C], summed in a fixed order.
// Generic form (lane -> 4 columns from c, four waves): wave 0 adds the four waves' quads.
__device__ __forceinline__ void bn_store_partials(f32x4 (&red)[2][4][64], f32x4 s0, f32x4 s1, int lane, int wave, int c, int C,
                                                  float* __restrict__ partial) {
  red[0][wave][lane] = s0; red[1][wave][lane] = s1;
  __syncthreads();
  if (wave == 0 && c < C) {
    s0 = red[0][0][lane] + red[0][1][lane] + red[0][2][lane] + red[0][3][lane];
    s1 = red[1][0][lane] + red[1][1][lane] + red[1][2][lane] + red[1][3][lane];
    *reinterpret_cast<f32x4*>(partial + ((int64_t)blockIdx.y * 2 + 0) * C + c) = s0;
    *reinterpret_cast<f32x4*>(partial + ((int64_t)blockIdx.y * 2 + 1) * C + c) = s1;
  }
}
// Wide form (thread -> one 8-column chunk, 256 / (C/8) row groups): thread t < 2*C sums column (t % C) of array (t / C) over
// the row groups.
__device__ __forceinline__ void bn_store_partials_wide(float (&red)[2][256][8], const float (&s0)[8], const float (&s1)[8], int C,
                                                       float* __restrict__ partial) {
  const int tid = threadIdx.x, cpr = C >> 3, rpp = 256 / cpr;
#pragma unroll
  for (int e = 0; e < 8; ++e) { red[0][tid][e] = s0[e]; red[1][tid][e] = s1[e]; }
  __syncthreads();
  for (int t = tid; t < 2 * C; t += 256) {
    const int which = t / C, col = t % C, cch = col >> 3, e = col & 7;
    float acc = 0.f;
    for (int g = 0; g < rpp; ++g) acc += red[which][g * cpr + cch][e];
    partial[((int64_t)blockIdx.y * 2 + which) * C + col] = acc;
  }
}

// ---- host side -----------------------------------------------------------------------------------------------------
// The wide forms: bf16, C in {64, 128, 256}, every matrix base 16-byte aligned (a null pointer counts as aligned).
static inline bool bn_wide(int32_t dtype, int64_t C, const void* a, const void* b = nullptr, const void* c = nullptr) {
  return dtype == DL_BF16 && (C == 64 || C == 128 || C == 256) && (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15) == 0;
}
// f(std::integral_constant<int, C>) for the C of a wide form
template <typename F> static inline void bn_wide_columns(int64_t C, F&& f) {
  if (C == 64) f(std::integral_constant<int, 64>{});
  else if (C == 128) f(std::integral_constant<int, 128>{});
  else f(std::integral_constant<int, 256>{});
}
// second stage: sums[2C] = the column sums of partial[chunks][2C]
static inline void bn_reduce_partials(const void* ws, const BnChunks& ck, int64_t C, float* sums, hipStream_t s) {
  hipLaunchKernelGGL(dl_reduce_partials_kernel, dim3((uint32_t)((2 * C + DL_REDUCE_COLS - 1) / DL_REDUCE_COLS)), dim3(1024), 0, s,
                     (const float*)ws, ck.chunks, (int64_t)(2 * C), (int)(2 * C), sums, 0);
}

// The checks the entry points share; `who` names the entry.  BN_TRY returns a failed check's status.
#define BN_TRY(call)                 \
  do {                               \
    const int rc_ = (call);          \
    if (rc_ != DL_OK) return rc_;    \
  } while (0)
static inline int bn_check_dtype(const char* who, int32_t dtype) {
  DL_CHECK_ARG(dtype == DL_BF16 || dtype == DL_F32, DL_ERR_ARG, "%s: bad dtype", who);
  return DL_OK;
}
static inline int bn_check_rows31(const char* who, int64_t R) {             // 32-bit row arithmetic in the kernels
  DL_CHECK_ARG(R < (1ll << 31), DL_ERR_SHAPE, "%s: R must fit 31 bits", who);
  return DL_OK;
}
static inline int bn_check_quads32(const char* who, int64_t R, int64_t C) {   // one thread per 4 elements, 32-bit index
  DL_CHECK_ARG(R < (1ll << 31) && R * (C / 4) < (1ll << 32), DL_ERR_SHAPE, "%s: R * C / 4 must fit 32 bits", who);
  return DL_OK;
}
static inline int bn_check_window(const char* who, int64_t win, int64_t halo, int64_t valid) {
  DL_CHECK_ARG(win >= 0 && halo >= 0 && valid >= 0 && (win == 0 || halo + valid <= win) && win < (1ll << 31), DL_ERR_ARG,
               "%s: bad window", who);
  return DL_OK;
}
static inline int bn_check_workspace(const char* who, int64_t R, int64_t C, const void* ws, size_t ws_bytes) {
  DL_CHECK_ARG(ws && ws_bytes >= bn_workspace_bytes(R, C), DL_ERR_WORKSPACE, "%s: workspace too small", who);
  return DL_OK;
}
}  // namespace
