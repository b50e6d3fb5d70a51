// optim.hip — what runs over the flat fp32 arena after the gradient guard's decision: the fused AdamW update and the weight
// EMA.  Four entry points (contract: include/druglamp_hip.h), two kernels:
//   dl_adamw_step           torch.optim.AdamW on a run of the arena, with an optional low-precision image of the parameters
//   dl_adamw_step_guarded   the same with grad_scale * guard[0]; writes nothing when guard[2] != 0
//   dl_adamw_step_groups    either of the two where the chunk of elements 4q .. 4q+3 uses lr * group_tab[2k] and weight decay
//                           group_tab[2k + 1], k = quad_group[q]
//   dl_ema_update           ema[i] += weight * (param[i] - ema[i]) in lerp form; writes nothing when guard[2] != 0
// The three AdamW entry points launch ONE kernel, adamw_kernel<TL>, from one host launcher, adamw_launch: guard and groups are
// nullable pointers, so "the same bits" between the forms is a property of the source and not of the build flags.
// Both kernels have one launch shape: one 16-byte chunk per thread, the thread that owns the ragged end goes scalar, the grid
// a function of n alone.  No LDS, no atomics: two calls on the same data agree bit for bit.
#include <math.h>
#include "common.cuh"

namespace {

constexpr int OPT_THREADS = 256;
constexpr int OPT_MAX_GROUPS = 64;

// ---------------- what the two kernels share ---------------------------------------------------------------------------------
// The guard record {clip coefficient, norm, skip flag, 0}: one 16-byte load at a wave-uniform address.  A kernel returns on
// skip before any other access: a skipped step writes nothing.
__device__ __forceinline__ bool guard_skips(const float* __restrict__ guard, float* coef) {
  const f32x4 gd = *reinterpret_cast<const f32x4*>(guard);
  *coef = gd[0];
  return gd[2] != 0.0f;
}
// first element of this thread's 16-byte chunk
__device__ __forceinline__ int64_t chunk_index() { return ((int64_t)blockIdx.x * OPT_THREADS + threadIdx.x) * 4; }
// workgroups for n elements (the caller checks that they fit one grid)
inline int64_t chunk_blocks(int64_t n) { return ((n + 3) / 4 + OPT_THREADS - 1) / OPT_THREADS; }

// ---------------- AdamW ----------------------------------------------------------------------------------------------------
// torch.optim.AdamW for ONE element (decoupled weight decay, bias-corrected moments): p, m, v are updated in place.
__device__ __forceinline__ void adamw_update(float& p, float& m, float& v, float g, float lr, float b1, float b2, float eps,
                                             float wd, float bc1, float bc2_sqrt, float gscale) {
  const float grad = g * gscale;
  float x = p * (1.0f - lr * wd);                    // decoupled weight decay
  m = b1 * m + (1.0f - b1) * grad;                   // torch: lerp / mul-add
  v = b2 * v + (1.0f - b2) * grad * grad;
  const float denom = sqrtf(v) / bc2_sqrt + eps;
  x -= (lr / bc1) * (m / denom);
  p = x;
}

// What one thread of an AdamW launch does: the 4 elements from i4 on (16-byte accesses; scalar for the tail of the range).
template <typename TL>
__device__ __forceinline__ void adamw_thread(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                             float* __restrict__ v, int64_t n, int64_t i4, float lr, float b1, float b2,
                                             float eps, float wd, float bc1, float bc2_sqrt, float gscale,
                                             TL* __restrict__ lowp) {
  const int cnt = (int)min((int64_t)4, n - i4);
  float pp[4], gg[4], mm[4], vv[4];
  if (cnt == 4) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(p + i4), b = *reinterpret_cast<const f32x4*>(g + i4);
    const f32x4 c = *reinterpret_cast<const f32x4*>(m + i4), d = *reinterpret_cast<const f32x4*>(v + i4);
    for (int j = 0; j < 4; ++j) { pp[j] = a[j]; gg[j] = b[j]; mm[j] = c[j]; vv[j] = d[j]; }
  } else {
    for (int j = 0; j < cnt; ++j) { pp[j] = p[i4 + j]; gg[j] = g[i4 + j]; mm[j] = m[i4 + j]; vv[j] = v[i4 + j]; }
  }
  for (int j = 0; j < cnt; ++j) adamw_update(pp[j], mm[j], vv[j], gg[j], lr, b1, b2, eps, wd, bc1, bc2_sqrt, gscale);
  if (cnt == 4) {
    *reinterpret_cast<f32x4*>(p + i4) = f32x4{pp[0], pp[1], pp[2], pp[3]};
    *reinterpret_cast<f32x4*>(m + i4) = f32x4{mm[0], mm[1], mm[2], mm[3]};
    *reinterpret_cast<f32x4*>(v + i4) = f32x4{vv[0], vv[1], vv[2], vv[3]};
    if (lowp) store4<TL>(lowp + i4, f32x4{pp[0], pp[1], pp[2], pp[3]});
  } else {
    for (int j = 0; j < cnt; ++j) {
      p[i4 + j] = pp[j]; m[i4 + j] = mm[j]; v[i4 + j] = vv[j];
      if (lowp) lowp[i4 + j] = from_f32<TL>(pp[j]);
    }
  }
}

// host side: the bias corrections dl_adamw_step has always passed to its kernel (fp32 powf, step after increment)
static inline void adamw_bias_corrections(float beta1, float beta2, int64_t step, float* bc1, float* bc2_sqrt) {
  *bc1 = 1.0f - powf(beta1, (float)step);
  *bc2_sqrt = sqrtf(1.0f - powf(beta2, (float)step));
}

// guard and quad_group / group_tab are nullable, each tested once per thread (kernel arguments: wave-uniform).  Without them
// lr, wd and gscale reach adamw_thread as they were passed: no multiply.
template <typename TL>
__global__ __launch_bounds__(OPT_THREADS) void adamw_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                            float* __restrict__ m, float* __restrict__ v, int64_t n, float lr,
                                                            float b1, float b2, float eps, float wd, float bc1, float bc2_sqrt,
                                                            float gscale, TL* __restrict__ lowp,
                                                            const float* __restrict__ guard,
                                                            const uint8_t* __restrict__ quad_group,
                                                            const float* __restrict__ group_tab, int n_groups) {
  if (guard) {
    float coef;
    if (guard_skips(guard, &coef)) return;
    gscale = gscale * coef;                                             // the guarded step's effective scale
  }
  const int64_t i4 = chunk_index();
  if (i4 >= n) return;
  if (quad_group) {
    const int k = quad_group[i4 >> 2];                                  // the chunk's group: one byte per 16-byte chunk
    if (k >= n_groups) return;                                          // no row for this id: no table read, no write
    lr = lr * group_tab[2 * k];                                         // ONE fp32 multiply: the lr a per-group call would receive
    wd = group_tab[2 * k + 1];
  }
  adamw_thread<TL>(p, g, m, v, n, i4, lr, b1, b2, eps, wd, bc1, bc2_sqrt, gscale, lowp);
}

// Every check, the bias corrections, the grid and the launch of the three entry points.  What an entry point requires beyond
// the common arguments (a guard, a group table) it says with need_guard / need_groups; `who` names it in the error text.
static int adamw_launch(const char* who, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float lr,
                        float beta1, float beta2, float eps, float weight_decay, int64_t step, float grad_scale, void* param_lowp,
                        int32_t lowp_dtype, const float* guard, bool need_guard, const uint8_t* quad_group,
                        const float* group_tab, int32_t n_groups, bool need_groups, dl_stream stream) {
  DL_CHECK_ARG(param && grad && exp_avg && exp_avg_sq && (guard || !need_guard) && ((quad_group && group_tab) || !need_groups),
               DL_ERR_ARG, "%s: null pointer", who);
  DL_CHECK_ARG(n > 0 && step >= 1, DL_ERR_ARG, "%s: need n > 0 and step >= 1", who);
  DL_CHECK_ARG(!need_groups || (n_groups >= 1 && n_groups <= OPT_MAX_GROUPS), DL_ERR_ARG, "%s: n_groups = %d is outside [1, %d]",
               who, (int)n_groups, OPT_MAX_GROUPS);
  DL_CHECK_ARG(aligned_to(guard, 16), DL_ERR_ARG, "%s: guard must be 16-byte aligned", who);
  float bc1, bc2s;
  adamw_bias_corrections(beta1, beta2, step, &bc1, &bc2s);
  const int64_t blocks = chunk_blocks(n);
  DL_CHECK_ARG(blocks <= 0x7fffffffLL, DL_ERR_ARG, "%s: n = %lld exceeds one grid", who, (long long)n);
  hipStream_t s = (hipStream_t)stream;
  if (param_lowp && lowp_dtype == DL_BF16)
    hipLaunchKernelGGL((adamw_kernel<bf16_t>), dim3((uint32_t)blocks), dim3(OPT_THREADS), 0, s, param, grad, exp_avg, exp_avg_sq,
                       n, lr, beta1, beta2, eps, weight_decay, bc1, bc2s, grad_scale, (bf16_t*)param_lowp, guard, quad_group,
                       group_tab, (int)n_groups);
  else
    hipLaunchKernelGGL((adamw_kernel<float>), dim3((uint32_t)blocks), dim3(OPT_THREADS), 0, s, param, grad, exp_avg, exp_avg_sq,
                       n, lr, beta1, beta2, eps, weight_decay, bc1, bc2s, grad_scale, (float*)param_lowp, guard, quad_group,
                       group_tab, (int)n_groups);
  DL_CHECK_LAUNCH(who);
  return DL_OK;
}

// ---------------- weight EMA -------------------------------------------------------------------------------------------------
// The lerp form: one rounding of p - e, one of the fma.  e == p gives p - e = +0 and the fma returns e, except for the sign
// of a zero (fma(w, +0, -0) is +0 under round-to-nearest): a zero difference keeps e's bits outright, so that e == p is a
// fixed point bit for bit, (-0, -0) included.  A NaN difference (a NaN operand, inf - inf) is not zero and goes through the fma.
__device__ __forceinline__ float ema_lerp(float e, float p, float w) {
  const float d = p - e;
  return d == 0.0f ? e : fmaf(w, d, e);
}

// 12 B per element, HBM-bound.
__global__ __launch_bounds__(OPT_THREADS) void ema_update_kernel(float* __restrict__ ema, const float* __restrict__ param,
                                                                 int64_t n, float w, const float* __restrict__ guard) {
  float coef;
  if (guard && guard_skips(guard, &coef)) return;
  const int64_t i4 = chunk_index();
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

}  // namespace

extern "C" int dl_adamw_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float lr, float beta1,
                             float beta2, float eps, float weight_decay, int64_t step, float grad_scale, void* param_lowp,
                             int32_t lowp_dtype, dl_stream stream) {
  return adamw_launch("dl_adamw_step", param, grad, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, weight_decay, step, grad_scale,
                      param_lowp, lowp_dtype, nullptr, false, nullptr, nullptr, 0, false, stream);
}

extern "C" int dl_adamw_step_guarded(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float lr,
                                     float beta1, float beta2, float eps, float weight_decay, int64_t step, float grad_scale,
                                     void* param_lowp, int32_t lowp_dtype, const float* guard, dl_stream stream) {
  return adamw_launch("dl_adamw_step_guarded", param, grad, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, weight_decay, step,
                      grad_scale, param_lowp, lowp_dtype, guard, true, nullptr, nullptr, 0, false, stream);
}

extern "C" int dl_adamw_step_groups(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float lr,
                                    float beta1, float beta2, float eps, int64_t step, float grad_scale, void* param_lowp,
                                    int32_t lowp_dtype, const uint8_t* quad_group, const float* group_tab, int32_t n_groups,
                                    const float* guard, dl_stream stream) {
  return adamw_launch("dl_adamw_step_groups", param, grad, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, 0.0f, step, grad_scale,
                      param_lowp, lowp_dtype, guard, false, quad_group, group_tab, n_groups, true, stream);
}

extern "C" int dl_ema_update(float* ema, const float* param, int64_t n, float weight, const float* guard, dl_stream stream) {
  hipStream_t s = (hipStream_t)stream;
  DL_CHECK_ARG(ema && param, DL_ERR_ARG, "dl_ema_update: null pointer");
  DL_CHECK_ARG(n > 0, DL_ERR_ARG, "dl_ema_update: n must be positive");
  DL_CHECK_ARG(aligned_to(ema, 16) && aligned_to(param, 16) && aligned_to(guard, 16), DL_ERR_ARG,
               "dl_ema_update: ema, param and guard must be 16-byte aligned");
  DL_CHECK_ARG(weight >= 0.0f && weight <= 1.0f, DL_ERR_ARG, "dl_ema_update: weight %g is not a finite value in [0, 1]",
               (double)weight);
  DL_CHECK_ARG(ema != param, DL_ERR_ARG, "dl_ema_update: ema and param are the same buffer");
  const int64_t blocks = chunk_blocks(n);
  DL_CHECK_ARG(blocks <= 0x7fffffffLL, DL_ERR_ARG, "dl_ema_update: n = %lld exceeds one grid", (long long)n);
  hipLaunchKernelGGL(ema_update_kernel, dim3((uint32_t)blocks), dim3(OPT_THREADS), 0, s, ema, param, n, weight, guard);
  DL_CHECK_LAUNCH("dl_ema_update");
  return DL_OK;
}
