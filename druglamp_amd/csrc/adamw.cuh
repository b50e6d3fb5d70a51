// adamw.cuh — the fused AdamW update, shared by dl_adamw_step (elementwise.hip) and dl_adamw_step_guarded (grad_guard.hip).
// One definition of the arithmetic: both kernels give the same bits for the same effective gradient scale.
#pragma once
#include "common.cuh"

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
