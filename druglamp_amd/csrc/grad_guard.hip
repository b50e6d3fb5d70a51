// grad_guard.hip — the gradient guard of the training step: global-norm clipping and the non-finite step skip, decided on the
// device.  Two entry points (contract: include/druglamp_hip.h):
//   dl_grad_sqnorm          sum of squares of a flat fp32 gradient run, fp64 from the per-element square onward, fixed order
//   dl_grad_guard_finalize  one thread: sum -> {clip coefficient, norm, skip flag} + the caller's cumulative counters
// What consumes the guard record, dl_adamw_step_guarded / dl_adamw_step_groups / dl_ema_update, is optim.hip.
// Nothing here uses an atomic: every sum has one association, so two calls on the same data agree bit for bit.
#include "common.cuh"

namespace {

constexpr int GG_THREADS = 256;
constexpr int GG_UNROLL = 4;                                          // 16-byte loads in flight per thread
constexpr int GG_BLOCK_CHUNKS = GG_THREADS * GG_UNROLL;               // 16-byte chunks per workgroup and grid pass
constexpr int64_t GG_BLOCK_ELEMS = (int64_t)GG_BLOCK_CHUNKS * 4;      // 4096 elements
constexpr int64_t GG_MAX_BLOCKS = 2048;                               // 8 workgroups per CU; beyond that the grid strides

// The launch shape is a function of n alone: `work` block-passes of 4096 elements, spread over the fewest grid passes that
// keep the grid at or below GG_MAX_BLOCKS, then over as few workgroups as those passes need (every workgroup gets the same
// number of passes, up to the ragged end).
inline int64_t gg_blocks(int64_t n) {
  const int64_t work = (n + GG_BLOCK_ELEMS - 1) / GG_BLOCK_ELEMS;
  const int64_t passes = (work + GG_MAX_BLOCKS - 1) / GG_MAX_BLOCKS;
  return (work + passes - 1) / passes;
}

// x . x added to s in fp64: the product of two fp32 values is exact in fp64 (48 significand bits), the largest finite fp32
// squared is 1.2e77.  A NaN or an infinity of x stays one in s.
__device__ __forceinline__ double sq4(f32x4 x, double s) {
  s += (double)x[0] * (double)x[0];
  s += (double)x[1] * (double)x[1];
  s += (double)x[2] * (double)x[2];
  s += (double)x[3] * (double)x[3];
  return s;
}

// Sum over the workgroup's 256 threads, the same value in every association-relevant respect on every call: xor butterfly
// inside a wave (every lane ends with the same sum), the four wave sums through LDS in a fixed order.  Valid in thread 0.
__device__ __forceinline__ double block_sum(double s, double* red) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) red[wave] = s;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(GG_THREADS) void sqnorm_partial_kernel(const float* __restrict__ g, int64_t n,
                                                                    double* __restrict__ partial) {
  __shared__ double red[GG_THREADS / 64];
  const int64_t n4 = n >> 2;                                           // whole 16-byte chunks
  const int64_t stride = (int64_t)gridDim.x * GG_BLOCK_CHUNKS;
  const f32x4* __restrict__ g4 = reinterpret_cast<const f32x4*>(g);
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
  int64_t c = (int64_t)blockIdx.x * GG_BLOCK_CHUNKS + threadIdx.x;
  for (; c + 3 * GG_THREADS < n4; c += stride) {                       // four independent loads in flight
    const f32x4 a = g4[c], b = g4[c + GG_THREADS], d = g4[c + 2 * GG_THREADS], e = g4[c + 3 * GG_THREADS];
    s0 = sq4(a, s0); s1 = sq4(b, s1); s2 = sq4(d, s2); s3 = sq4(e, s3);
  }
  // the ragged end of the range: c + 768 >= n4 here, and every later pass of this thread lies beyond n4
  if (c < n4) s0 = sq4(g4[c], s0);
  if (c + GG_THREADS < n4) s1 = sq4(g4[c + GG_THREADS], s1);
  if (c + 2 * GG_THREADS < n4) s2 = sq4(g4[c + 2 * GG_THREADS], s2);
  if (blockIdx.x == 0 && threadIdx.x == 0)                              // the n % 4 trailing elements, scalar
    for (int64_t i = n4 * 4; i < n; ++i) s3 += (double)g[i] * (double)g[i];
  const double tot = block_sum((s0 + s1) + (s2 + s3), red);
  if (threadIdx.x == 0) partial[blockIdx.x] = tot;
}

// second stage, one workgroup: the partials in a fixed order -> acc[0]
__global__ __launch_bounds__(GG_THREADS) void sqnorm_final_kernel(const double* __restrict__ partial, int nparts,
                                                                  double* __restrict__ acc, int accumulate) {
  __shared__ double red[GG_THREADS / 64];
  double s = 0.0;
  for (int i = threadIdx.x; i < nparts; i += GG_THREADS) s += partial[i];
  const double tot = block_sum(s, red);
  if (threadIdx.x == 0) acc[0] = accumulate ? acc[0] + tot : tot;
}

__global__ void guard_finalize_kernel(const double* __restrict__ acc, float pre_scale, float max_norm, int skip_nonfinite,
                                      float* __restrict__ guard, int64_t* __restrict__ counters) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const double a = acc[0];
  const bool nonfinite = !(fabs(a) <= 1.79769313486231570815e308);     // NaN or infinity
  const double norm = (double)pre_scale * sqrt(a);
  double coef = 1.0;
  if (max_norm > 0.0f) {
    // torch.nn.utils.clip_grad_norm_: clamp(max_norm / (total_norm + 1e-6), max=1.0); a NaN norm stays a NaN coefficient
    const double c = (double)max_norm / (norm + 1e-6);
    coef = c > 1.0 ? 1.0 : c;
  }
  const bool skip = nonfinite && skip_nonfinite != 0;
  const f32x4 out = {skip ? 0.0f : (float)coef, (float)norm, skip ? 1.0f : 0.0f, 0.0f};
  *reinterpret_cast<f32x4*>(guard) = out;
  counters[0] += skip ? 1 : 0;
  counters[1] += (coef < 1.0 && !skip) ? 1 : 0;
}

}  // namespace

extern "C" int dl_grad_sqnorm(const float* g, int64_t n, double* acc, int32_t accumulate, void* workspace,
                              int64_t workspace_bytes, dl_stream stream) {
  hipStream_t s = (hipStream_t)stream;
  DL_CHECK_ARG(g && acc && workspace, DL_ERR_ARG, "dl_grad_sqnorm: null pointer");
  DL_CHECK_ARG(n > 0, DL_ERR_ARG, "dl_grad_sqnorm: n must be positive");
  DL_CHECK_ARG(aligned_to(g, 16), DL_ERR_ARG, "dl_grad_sqnorm: g must be 16-byte aligned");
  DL_CHECK_ARG(aligned_to(acc, 8) && aligned_to(workspace, 8), DL_ERR_ARG, "dl_grad_sqnorm: acc and workspace must be 8-byte aligned");
  const int64_t blocks = gg_blocks(n);
  DL_CHECK_ARG(workspace_bytes >= blocks * 8, DL_ERR_ARG, "dl_grad_sqnorm: workspace too small (%lld bytes, need %lld)",
               (long long)workspace_bytes, (long long)(blocks * 8));
  hipLaunchKernelGGL(sqnorm_partial_kernel, dim3((uint32_t)blocks), dim3(GG_THREADS), 0, s, g, n, (double*)workspace);
  hipLaunchKernelGGL(sqnorm_final_kernel, dim3(1), dim3(GG_THREADS), 0, s, (const double*)workspace, (int)blocks, acc,
                     (int)accumulate);
  DL_CHECK_LAUNCH("dl_grad_sqnorm");
  return DL_OK;
}

extern "C" int dl_grad_guard_finalize(const double* acc, float pre_scale, float max_norm, int32_t skip_nonfinite, float* guard,
                                      int64_t* counters, dl_stream stream) {
  hipStream_t s = (hipStream_t)stream;
  DL_CHECK_ARG(acc && guard && counters, DL_ERR_ARG, "dl_grad_guard_finalize: null pointer");
  DL_CHECK_ARG(aligned_to(acc, 8) && aligned_to(counters, 8) && aligned_to(guard, 16), DL_ERR_ARG,
               "dl_grad_guard_finalize: acc / counters must be 8-byte, guard 16-byte aligned");
  hipLaunchKernelGGL(guard_finalize_kernel, dim3(1), dim3(64), 0, s, acc, pre_scale, max_norm, (int)skip_nonfinite, guard,
                     counters);
  DL_CHECK_LAUNCH("dl_grad_guard_finalize");
  return DL_OK;
}
