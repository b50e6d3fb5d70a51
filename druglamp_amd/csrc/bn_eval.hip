// bn_eval.hip — backward of a BatchNorm that ran on FIXED statistics (eval mode: the running mean / variance), channel-last
// [R][C] with the row rules of bn.hip.  With fixed statistics dx does not depend on the column sums, so the training-mode
// chain (partial sums, their reduction, the apply pass: bn.hip) is ONE pass over dz and y that writes dx and the per-workgroup
// partial sums of (d beta, d gamma) together, plus the tiny second stage over the partials:
//   yhat = (y - mean) rstd,   g = dz [relu_out: where yhat gamma + beta > 0],   dx = g gamma rstd [relu_in: where y > 0],
//   sums[0..C) = sum_r g,   sums[C..2C) = sum_r g yhat     over the rows that take part.
// Row weights mark excluded rows (< 0) and nothing else: a compact row's dz already is the sum over the rows it stands for and
// yhat is shared by them, so the unweighted sum over the compact rows is the sum over the expanded ones.
#include "bn_rows.cuh"

namespace {
// Generic form.  grid (ceil(C/256), chunks): lane -> 4 columns, wave w -> rows r0 + w, r0 + w + 4, ... of the workgroup's chunk.
// SUMS: partial[chunk][2][C] = the chunk's (sum g | sum g yhat), summed over the four waves in a fixed order.
template <typename T, bool SUMS>
__global__ __launch_bounds__(256) void bn_eval_bwd_kernel(const T* __restrict__ dz, const T* __restrict__ y, const float* __restrict__ mean,
                                                          const float* __restrict__ rstd, const float* __restrict__ gamma,
                                                          const float* __restrict__ beta, int relu_in, int relu_out, T* __restrict__ dy,
                                                          int64_t R, int C, int64_t win, int64_t halo, int64_t valid,
                                                          const float* __restrict__ rw, float* __restrict__ partial, int rows_per_block) {
  __shared__ f32x4 red[2][4][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = blockIdx.x * 256 + lane * 4;
  const int64_t r0 = (int64_t)blockIdx.y * rows_per_block;
  const int64_t r1 = min(R, r0 + rows_per_block);
  f32x4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = {0.f, 0.f, 0.f, 0.f};
  if (c < C) {
    const f32x4 mu = *reinterpret_cast<const f32x4*>(mean + c), rs = *reinterpret_cast<const f32x4*>(rstd + c);
    const f32x4 gm = *reinterpret_cast<const f32x4*>(gamma + c);
    const f32x4 gr = gm * rs;
    f32x4 bt = {0.f, 0.f, 0.f, 0.f};
    if (relu_out) bt = *reinterpret_cast<const f32x4*>(beta + c);
    for (int64_t r = r0 + wave; r < r1; r += 4) {
      f32x4 o = {0.f, 0.f, 0.f, 0.f};                      // excluded rows: never read, written as zeros
      if (bn_row_in(rw, r, win, halo, valid)) {
        f32x4 d = load4<T>(dz + r * C + c);
        const f32x4 yv = load4<T>(y + r * C + c);
        const f32x4 yh = (yv - mu) * rs;
        if (relu_out) {
#pragma unroll
          for (int e = 0; e < 4; ++e) d[e] = (yh[e] * gm[e] + bt[e] > 0.f) ? d[e] : 0.f;
        }
        if (SUMS) { s0 += d; s1 += d * yh; }
        o = d * gr;
        if (relu_in) {
#pragma unroll
          for (int e = 0; e < 4; ++e) o[e] = yv[e] > 0.f ? o[e] : 0.f;
        }
      }
      store4<T>(dy + r * C + c, o);
    }
  }
  if (!SUMS) return;
  bn_store_partials(red, s0, s1, lane, wave, c, C, partial);
}

// Wide form (bf16, C in {64, 128, 256}, 16-byte bases).  grid (1, chunks).  A thread keeps ONE 8-column chunk (16 bytes) for the
// whole launch, so the per-column parameters are loaded once; 256 / (C/8) rows per pass, four passes in flight: the loads of
// dz and y of four rows are issued before the first is used.  Partial layout as above.
constexpr int BN_EVAL_U = 4;

// RELU_OUT is a template parameter here (a flag in the generic form): without it gamma and beta are not kept, and the kernel
// stays within the 128 registers of four workgroups per CU without scratch (with it: three).
template <bool SUMS, bool RELU_OUT>
__global__ __launch_bounds__(256, RELU_OUT ? 3 : 4) void bn_eval_bwd_wide_kernel(const bf16_t* __restrict__ dz, const bf16_t* __restrict__ y,
                                                               const float* __restrict__ mean, const float* __restrict__ rstd,
                                                               const float* __restrict__ gamma, const float* __restrict__ beta,
                                                               int relu_in, bf16_t* __restrict__ dy, int64_t R, int C,
                                                               int64_t win, int64_t halo, int64_t valid, const float* __restrict__ rw,
                                                               float* __restrict__ partial, int rows_per_block) {
  __shared__ float red[2][256][8];
  const int tid = threadIdx.x;
  const int cpr = C >> 3, rpp = 256 / cpr;                  // 16-byte chunks per row, rows per pass
  const int ch = tid % cpr, rsub = tid / cpr, c = ch * 8;
  const int64_t r0 = (int64_t)blockIdx.y * rows_per_block;
  const int64_t r1 = min(R, r0 + rows_per_block);
  float s0[8], s1[8], mu[8], rs[8], gm[8], bt[8], gr[8];            // (gm, bt: RELU_OUT only)
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    s0[e] = 0.f; s1[e] = 0.f;
    mu[e] = mean[c + e]; rs[e] = rstd[c + e]; gm[e] = gamma[c + e]; bt[e] = RELU_OUT ? beta[c + e] : 0.f;
    gr[e] = gm[e] * rs[e];
  }
  for (int64_t r = r0 + rsub; r < r1; r += BN_EVAL_U * rpp) {
    u32x4 wd[BN_EVAL_U], wy[BN_EVAL_U];
    bool ok[BN_EVAL_U];
#pragma unroll
    for (int u = 0; u < BN_EVAL_U; ++u) {
      const int64_t rr = r + (int64_t)u * rpp;
      ok[u] = rr < r1 && bn_row_in(rw, rr, win, halo, valid);
      wd[u] = u32x4{0u, 0u, 0u, 0u}; wy[u] = wd[u];
      if (ok[u]) {
        wd[u] = *reinterpret_cast<const u32x4*>(dz + rr * C + c);
        wy[u] = *reinterpret_cast<const u32x4*>(y + rr * C + c);
      }
    }
#pragma unroll
    for (int u = 0; u < BN_EVAL_U; ++u) {
      const int64_t rr = r + (int64_t)u * rpp;
      if (rr >= r1) break;
      u32x4 o = {0u, 0u, 0u, 0u};                           // excluded rows: never read, written as zeros
      if (ok[u]) {
        float d[8], yv[8];
        unpack8(wd[u], d);
        unpack8(wy[u], yv);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float yh = (yv[e] - mu[e]) * rs[e];                  // same operation order as the generic form
          float g = d[e];
          if (RELU_OUT) g = (yh * gm[e] + bt[e] > 0.f) ? g : 0.f;
          if (SUMS) { s0[e] += g; s1[e] += g * yh; }
          float v = RELU_OUT ? g * gm[e] * rs[e] : g * gr[e];     // (RELU_OUT: gr is not kept either)
          if (relu_in) v = yv[e] > 0.f ? v : 0.f;
          d[e] = v;
        }
        o = pack8(d);
      }
      store16_fam<2>(dy + rr * C + c, o);
    }
  }
  if (!SUMS) return;
  bn_store_partials_wide(red, s0, s1, C, partial);
}
}  // namespace

extern "C" int dl_bn_eval_bwd(const void* dz, const void* y, const float* mean, const float* rstd, const float* gamma, const float* beta,
                              int32_t relu_in, int32_t relu_out, void* dy, float* sums, int64_t R, int64_t C, int64_t win, int64_t halo,
                              int64_t valid, const float* row_w, int32_t dtype, void* workspace, size_t workspace_bytes, dl_stream stream) {
  hipStream_t s = (hipStream_t)stream;
  const char* who = "dl_bn_eval_bwd";
  DL_CHECK_ARG(dz && y && mean && rstd && gamma && dy && R > 0 && C > 0 && C % 4 == 0, DL_ERR_ARG, "%s: bad args", who);
  DL_CHECK_ARG(!relu_out || beta, DL_ERR_ARG, "%s: relu_out needs beta", who);
  DL_CHECK_ARG(dy != dz && dy != y, DL_ERR_ARG, "%s: dy must not alias dz or y", who);
  BN_TRY(bn_check_dtype(who, dtype));
  BN_TRY(bn_check_rows31(who, R));
  BN_TRY(bn_check_window(who, win, halo, valid));
  const bool with_sums = sums != nullptr;
  if (with_sums) BN_TRY(bn_check_workspace(who, R, C, workspace, workspace_bytes));
  if (row_w) { win = 0; halo = 0; valid = 0; }
  const BnChunks ck = bn_chunks(R, C);
  float* ws = with_sums ? (float*)workspace : nullptr;
  const bool wide = bn_wide(dtype, C, dz, y, dy);
  const dim3 grid = bn_partial_grid(C, ck, wide);
  auto generic = [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL((with_sums ? bn_eval_bwd_kernel<T, true> : bn_eval_bwd_kernel<T, false>), grid, dim3(256), 0, s, (const T*)dz,
                       (const T*)y, mean, rstd, gamma, beta, (int)relu_in, (int)relu_out, (T*)dy, R, (int)C, win, halo, valid, row_w, ws, ck.rows);
  };
  if (wide) {
    auto k = with_sums ? (relu_out ? bn_eval_bwd_wide_kernel<true, true> : bn_eval_bwd_wide_kernel<true, false>)
                       : (relu_out ? bn_eval_bwd_wide_kernel<false, true> : bn_eval_bwd_wide_kernel<false, false>);
    hipLaunchKernelGGL(k, grid, dim3(256), 0, s, (const bf16_t*)dz, (const bf16_t*)y, mean, rstd, gamma, beta, (int)relu_in, (bf16_t*)dy, R,
                       (int)C, win, halo, valid, row_w, ws, ck.rows);
  } else if (dtype == DL_BF16) generic(bf16_t{});
  else generic(float{});
  if (with_sums) bn_reduce_partials(ws, ck, C, sums, s);
  DL_CHECK_LAUNCH(who);
  return DL_OK;
}
