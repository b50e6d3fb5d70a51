// adamw_groups.hip — fused AdamW with parameter groups: per-group learning-rate scale and weight decay, resolved on the
// device per 16-byte chunk.  One entry point (contract: include/druglamp_hip.h):
//   dl_adamw_step_groups   dl_adamw_step (guard null) or dl_adamw_step_guarded (guard given) where the chunk of elements
//                          4q .. 4q+3 uses lr * group_tab[2k] and weight decay group_tab[2k + 1], k = quad_group[q]
// The arithmetic is adamw.cuh's adamw_thread, the one definition dl_adamw_step and dl_adamw_step_guarded share: a maximal
// segment of equal group id gets the bits of those entry points called on the segment alone with the group's values.
// AdamW's launch shape (one 16-byte chunk per thread, scalar tail, the grid a function of n alone); 0.25 B of ids per element
// on top of the 28 B AdamW moves.  No LDS, no atomics: two calls on the same data agree bit for bit.
#include "adamw.cuh"

namespace {

constexpr int AG_THREADS = 256;
constexpr int AG_MAX_GROUPS = 64;

template <typename TL>
__global__ __launch_bounds__(AG_THREADS) void adamw_groups_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                                  float* __restrict__ m, float* __restrict__ v, int64_t n,
                                                                  float lr, float b1, float b2, float eps, float bc1,
                                                                  float bc2_sqrt, float gscale, TL* __restrict__ lowp,
                                                                  const uint8_t* __restrict__ quad_group,
                                                                  const float* __restrict__ group_tab, int n_groups,
                                                                  const float* __restrict__ guard) {
  float gs = gscale;
  if (guard) {
    const f32x4 gd = *reinterpret_cast<const f32x4*>(guard);            // one load at a wave-uniform address
    if (gd[2] != 0.0f) return;                                          // skipped step: nothing is written
    gs = gscale * gd[0];                                                // (dl_adamw_step_guarded's effective scale)
  }
  const int64_t i4 = ((int64_t)blockIdx.x * AG_THREADS + threadIdx.x) * 4;
  if (i4 >= n) return;
  const int k = quad_group[i4 >> 2];                                    // the chunk's group: one byte per 16-byte chunk
  if (k >= n_groups) return;                                            // no row for this id: no table read, no write
  const float lr_k = lr * group_tab[2 * k];                             // ONE fp32 multiply: the lr a per-group call would receive
  const float wd_k = group_tab[2 * k + 1];
  adamw_thread<TL>(p, g, m, v, n, i4, lr_k, b1, b2, eps, wd_k, bc1, bc2_sqrt, gs, lowp);
}

inline bool aligned_to(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

}  // namespace

extern "C" int dl_adamw_step_groups(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float lr,
                                    float beta1, float beta2, float eps, int64_t step, float grad_scale, void* param_lowp,
                                    int32_t lowp_dtype, const uint8_t* quad_group, const float* group_tab, int32_t n_groups,
                                    const float* guard, dl_stream stream) {
  hipStream_t s = (hipStream_t)stream;
  DL_CHECK_ARG(param && grad && exp_avg && exp_avg_sq && quad_group && group_tab, DL_ERR_ARG,
               "dl_adamw_step_groups: null pointer");
  DL_CHECK_ARG(n > 0 && step >= 1, DL_ERR_ARG, "dl_adamw_step_groups: need n > 0 and step >= 1");
  DL_CHECK_ARG(n_groups >= 1 && n_groups <= AG_MAX_GROUPS, DL_ERR_ARG, "dl_adamw_step_groups: n_groups = %d is outside [1, %d]",
               (int)n_groups, AG_MAX_GROUPS);
  DL_CHECK_ARG(aligned_to(guard, 16), DL_ERR_ARG, "dl_adamw_step_groups: guard must be 16-byte aligned");
  float bc1, bc2s;
  adamw_bias_corrections(beta1, beta2, step, &bc1, &bc2s);
  const int64_t blocks = ((n + 3) / 4 + AG_THREADS - 1) / AG_THREADS;
  DL_CHECK_ARG(blocks <= 0x7fffffffLL, DL_ERR_ARG, "dl_adamw_step_groups: n = %lld exceeds one grid", (long long)n);
  if (param_lowp && lowp_dtype == DL_BF16)
    hipLaunchKernelGGL((adamw_groups_kernel<bf16_t>), dim3((uint32_t)blocks), dim3(AG_THREADS), 0, s, param, grad, exp_avg,
                       exp_avg_sq, n, lr, beta1, beta2, eps, bc1, bc2s, grad_scale, (bf16_t*)param_lowp, quad_group, group_tab,
                       (int)n_groups, guard);
  else
    hipLaunchKernelGGL((adamw_groups_kernel<float>), dim3((uint32_t)blocks), dim3(AG_THREADS), 0, s, param, grad, exp_avg,
                       exp_avg_sq, n, lr, beta1, beta2, eps, bc1, bc2s, grad_scale, (float*)param_lowp, quad_group, group_tab,
                       (int)n_groups, guard);
  DL_CHECK_LAUNCH("dl_adamw_step_groups");
  return DL_OK;
}
