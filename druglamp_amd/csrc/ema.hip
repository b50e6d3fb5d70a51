// ema.hip — the weight EMA of the training step: one pass that moves a shadow copy of the flat parameter arena towards the
// live parameters.  One entry point (contract: include/druglamp_hip.h):
//   dl_ema_update   ema[i] += weight * (param[i] - ema[i]) in lerp form; writes nothing when guard[2] != 0
// Per-element fp32 on 16-byte vectors, 12 B per element, HBM-bound.  No atomics, no LDS: two calls on the same data agree
// bit for bit.
#include "common.cuh"

namespace {

constexpr int EMA_THREADS = 256;

// The lerp form: one rounding of p - e, one of the fma.  e == p gives p - e = +0 and the fma returns e, except for the sign
// of a zero (fma(w, +0, -0) is +0 under round-to-nearest): a zero difference keeps e's bits outright, so that e == p is a
// fixed point bit for bit, (-0, -0) included.  A NaN difference (a NaN operand, inf - inf) is not zero and goes through the fma.
__device__ __forceinline__ float ema_lerp(float e, float p, float w) {
  const float d = p - e;
  return d == 0.0f ? e : fmaf(w, d, e);
}

// AdamW's launch shape: one 16-byte chunk per thread, the thread that owns the ragged end goes scalar.
__global__ __launch_bounds__(EMA_THREADS) void ema_update_kernel(float* __restrict__ ema, const float* __restrict__ param,
                                                                 int64_t n, float w, const float* __restrict__ guard) {
  if (guard) {
    const f32x4 gd = *reinterpret_cast<const f32x4*>(guard);            // one load at a wave-uniform address
    if (gd[2] != 0.0f) return;                                          // skipped step: nothing is written
  }
  const int64_t i4 = ((int64_t)blockIdx.x * EMA_THREADS + threadIdx.x) * 4;
  if (i4 >= n) return;
  if (n - i4 >= 4) {
    f32x4 e = *reinterpret_cast<const f32x4*>(ema + i4);
    const f32x4 p = *reinterpret_cast<const f32x4*>(param + i4);
#pragma unroll
    for (int j = 0; j < 4; ++j) e[j] = ema_lerp(e[j], p[j], w);
    *reinterpret_cast<f32x4*>(ema + i4) = e;
  } else {
#pragma clang loop vectorize(disable) interleave(disable)               // at most three elements: keep them scalar
    for (int64_t i = i4; i < n; ++i) ema[i] = ema_lerp(ema[i], param[i], w);   // the n % 4 trailing elements
  }
}

inline bool aligned_to(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

}  // namespace

extern "C" int dl_ema_update(float* ema, const float* param, int64_t n, float weight, const float* guard, dl_stream stream) {
  hipStream_t s = (hipStream_t)stream;
  DL_CHECK_ARG(ema && param, DL_ERR_ARG, "dl_ema_update: null pointer");
  DL_CHECK_ARG(n > 0, DL_ERR_ARG, "dl_ema_update: n must be positive");
  DL_CHECK_ARG(aligned_to(ema, 16) && aligned_to(param, 16) && aligned_to(guard, 16), DL_ERR_ARG,
               "dl_ema_update: ema, param and guard must be 16-byte aligned");
  DL_CHECK_ARG(weight >= 0.0f && weight <= 1.0f, DL_ERR_ARG, "dl_ema_update: weight %g is not a finite value in [0, 1]",
               (double)weight);
  DL_CHECK_ARG(ema != param, DL_ERR_ARG, "dl_ema_update: ema and param are the same buffer");
  const int64_t blocks = ((n + 3) / 4 + EMA_THREADS - 1) / EMA_THREADS;
  DL_CHECK_ARG(blocks <= 0x7fffffffLL, DL_ERR_ARG, "dl_ema_update: n = %lld exceeds one grid", (long long)n);
  hipLaunchKernelGGL(ema_update_kernel, dim3((uint32_t)blocks), dim3(EMA_THREADS), 0, s, ema, param, n, weight, guard);
  DL_CHECK_LAUNCH("dl_ema_update");
  return DL_OK;
}
