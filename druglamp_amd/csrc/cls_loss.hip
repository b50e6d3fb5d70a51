// cls_loss.hip — the imbalance-aware classification loss of the classifier step: weighted / focal binary cross entropy on
// logits, forward and backward, one launch each at the step's batch sizes (contract: include/druglamp_hip.h).
//   dl_cls_loss_fwd   probs[i] = sigmoid(z_i), out2 = [sum_i l_i / den, den]
//   dl_cls_loss_bwd   dscore = gout * d(loss) / d(score), recomputed from z: nothing is saved per row
// Row i: z = score[i][0] (one output) or score[i][1] - score[i][0] (two), y = labels[i], w = weights[i] (1 without weights),
//   p = sigmoid(z), q = sigmoid(-z), d = |y q - (1 - y) p|, m = d^gamma (gamma == 0: 1),
//   l = w m [a_pos y softplus(-z) + a_neg (1 - y) softplus(z)],   den = N without weights, sum of the valid weights with.
// Forms (one host rule, cls_single(N)):
//   N <= CLS_ONE_WG_ROWS (4096): ONE workgroup of 256 threads walks the rows with stride 256 (at most 16 per thread), sums
//       them with the wave tree and four LDS words, divides and writes out2 — one launch.
//   above: one row per thread, a pair of partial sums per 256-row workgroup into the workspace, then cls_loss_final_kernel.
//   The backward is one thread per row in both.
// Fixed summation order, no floating-point atomics: two launches on the same data agree bit for bit.
// A non-finite z, a bad label (outside [0, 1] or not finite) and a bad weight (negative or not finite) poison their row: its
// loss term and its gradient are NaN.  A bad label or weight also ORs the caller's `code` into the caller's flag word (the one
// atomic, an integer OR, as dl_rows_equal_check reports).
#include <math.h>
#include "pair_keys.cuh"

namespace {

constexpr int CLS_THREADS = 256;
constexpr int64_t CLS_ONE_WG_ROWS = 4096;

struct ClsP {
  const void* score; int64_t ld; int n_out;
  const float* labels; const float* weights; int64_t N;
  float a_pos, a_neg, gamma;
  float* probs; float* out2; float* partial; uint32_t* flags; uint32_t code;   // forward
  const float* stat; const float* gout; void* dscore; int64_t ldd;   // backward
};

struct ClsRow { float l, dl, p, wden; bool bad_in; };

template <typename T> __device__ __forceinline__ float cls_z(const ClsP& c, int64_t r) {
  const T* row = reinterpret_cast<const T*>(c.score) + r * c.ld;
  return c.n_out == 2 ? to_f32(row[1]) - to_f32(row[0]) : to_f32(row[0]);
}

// One row.  l and dl = d l / d z without the 1 / den; wden = the row's share of den.
__device__ __forceinline__ ClsRow cls_row(float z, float y, float w, bool has_w, float a_pos, float a_neg, float gamma) {
  const float a = fabsf(z);
  const float e = expf(-a);                          // in (0, 1]
  const float l1 = log1pf(e);
  const float hi = 1.0f / (1.0f + e), lo = e * hi;   // sigmoid(a), sigmoid(-a): no 1 - x in the tails
  const bool pos = z >= 0.0f;
  const float p = pos ? hi : lo, q = pos ? lo : hi;
  const float sp_pos = fmaxf(z, 0.0f) + l1, sp_neg = fmaxf(-z, 0.0f) + l1;   // softplus(z) = -log(1 - p), softplus(-z) = -log p
  const float ny = 1.0f - y;
  const float s = y * q - ny * p;                    // y - p
  const float d = fabsf(s);
  float pm1 = 1.0f, m = 1.0f, dm = 0.0f;             // d^(gamma - 1), d^gamma, d m / d z
  if (gamma != 0.0f) {
    const int gi = (int)gamma;
    if ((float)gi == gamma) {
      for (int k = 1; k < gi; ++k) pm1 *= d;
    } else {
      pm1 = d > 0.0f ? powf(d, gamma - 1.0f) : 0.0f;
    }
    m = pm1 * d;
    const float sg = s > 0.0f ? 1.0f : (s < 0.0f ? -1.0f : 0.0f);
    dm = -(gamma * pm1) * sg * p * q;
  }
  const float cp = a_pos * y, cn = a_neg * ny;
  const float B = cp * sp_neg + cn * sp_pos;
  const float dB = cn * p - cp * q;
  ClsRow o;
  o.p = p;
  o.l = (w * m) * B;
  o.dl = w * (dm * B + m * dB);
  o.wden = has_w ? w : 1.0f;
  const bool bad_in = !(y >= 0.0f && y <= 1.0f) || !(w >= 0.0f && w < INFINITY);
  o.bad_in = bad_in;
  if (bad_in || !(a < INFINITY)) { o.l = __builtin_nanf(""); o.dl = __builtin_nanf(""); }
  if (!(w >= 0.0f && w < INFINITY)) o.wden = 0.0f;   // a bad weight stays out of den: the other rows keep their gradient
  return o;
}

__device__ __forceinline__ void cls_block_sum(float& a, float& b, float (&red)[2][4]) {
  a = wave_sum(a); b = wave_sum(b);
  if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = a; red[1][threadIdx.x >> 6] = b; }
  __syncthreads();
  a = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
  b = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
}

// grid 1: every row, then out2.  grid ceil(N / 256): one row per thread, then partial[2 b], partial[2 b + 1].
template <typename T>
__global__ __launch_bounds__(CLS_THREADS) void cls_loss_fwd_kernel(const ClsP c) {
  __shared__ float red[2][4];
  float loss = 0.f, den = 0.f;
  bool bad = false;
  const int64_t step = (int64_t)gridDim.x * CLS_THREADS;
  for (int64_t r = (int64_t)blockIdx.x * CLS_THREADS + threadIdx.x; r < c.N; r += step) {
    const float z = cls_z<T>(c, r);
    const ClsRow o = cls_row(z, c.labels[r], c.weights ? c.weights[r] : 1.0f, c.weights != nullptr, c.a_pos, c.a_neg, c.gamma);
    if (c.probs) c.probs[r] = o.p;
    loss += o.l; den += o.wden; bad |= o.bad_in;
  }
  if (bad && c.flags) atomicOr(c.flags, c.code);
  cls_block_sum(loss, den, red);
  if (threadIdx.x == 0) {
    if (c.partial) { c.partial[2 * (int64_t)blockIdx.x] = loss; c.partial[2 * (int64_t)blockIdx.x + 1] = den; }
    else { c.out2[0] = loss / den; c.out2[1] = den; }
  }
}

__global__ __launch_bounds__(CLS_THREADS) void cls_loss_final_kernel(const float* __restrict__ partial, int64_t nblocks,
                                                                     float* __restrict__ out2) {
  __shared__ float red[2][4];
  float a = 0.f, b = 0.f;
  for (int64_t i = threadIdx.x; i < nblocks; i += CLS_THREADS) { a += partial[2 * i]; b += partial[2 * i + 1]; }
  cls_block_sum(a, b, red);
  if (threadIdx.x == 0) { out2[0] = a / b; out2[1] = b; }
}

// dscore[r] = g (one output) or (-g, +g) (two), g = gout / den * d l / d z
template <typename T>
__global__ __launch_bounds__(CLS_THREADS) void cls_loss_bwd_kernel(const ClsP c) {
  const int64_t r = (int64_t)blockIdx.x * CLS_THREADS + threadIdx.x;
  if (r >= c.N) return;
  const float z = cls_z<T>(c, r);
  const ClsRow o = cls_row(z, c.labels[r], c.weights ? c.weights[r] : 1.0f, c.weights != nullptr, c.a_pos, c.a_neg, c.gamma);
  const float g = (c.gout[0] / c.stat[1]) * o.dl;
  T* drow = reinterpret_cast<T*>(c.dscore) + r * c.ldd;
  if (c.n_out == 2) { drow[0] = from_f32<T>(-g); drow[1] = from_f32<T>(g); }
  else drow[0] = from_f32<T>(g);
}

inline bool cls_single(int64_t N) { return N <= CLS_ONE_WG_ROWS; }

int cls_check(const char* who, const void* score, int64_t ld, int32_t n_out, int32_t dtype, const float* labels, int64_t N,
              float a_pos, float a_neg, float gamma) {
  DL_CHECK_ARG(score && labels && N > 0, DL_ERR_ARG, "%s: null pointer or N <= 0", who);
  DL_CHECK_ARG((n_out == 1 || n_out == 2) && ld >= n_out, DL_ERR_ARG, "%s: n_out must be 1 or 2 and ld >= n_out", who);
  DL_CHECK_ARG(dtype == DL_F32 || dtype == DL_BF16, DL_ERR_ARG, "%s: bad dtype", who);
  DL_CHECK_ARG(a_pos >= 0.f && a_pos < INFINITY && a_neg >= 0.f && a_neg < INFINITY && a_pos + a_neg > 0.f, DL_ERR_ARG,
               "%s: a_pos = %g, a_neg = %g must be finite, >= 0 and not both 0", who, (double)a_pos, (double)a_neg);
  DL_CHECK_ARG(gamma == 0.f || (gamma >= 1.f && gamma <= 8.f), DL_ERR_ARG, "%s: gamma = %g must be 0 or in [1, 8]", who, (double)gamma);
  DL_CHECK_ARG((N + CLS_THREADS - 1) / CLS_THREADS <= 0x7fffffffLL, DL_ERR_ARG, "%s: N = %lld exceeds one grid", who, (long long)N);
  return DL_OK;
}

}  // namespace

extern "C" size_t dl_cls_loss_workspace_bytes(int64_t N) {
  return cls_single(N) ? 0 : (size_t)((N + CLS_THREADS - 1) / CLS_THREADS) * 2 * sizeof(float);
}

extern "C" int dl_cls_loss_fwd(const void* score, int64_t ld, int32_t n_out, int32_t dtype, const float* labels, const float* weights,
                               int64_t N, float a_pos, float a_neg, float gamma, float* probs, float* out2, void* workspace,
                               size_t workspace_bytes, uint32_t code, uint32_t* flags, dl_stream stream) {
  hipStream_t s = (hipStream_t)stream;
  const int rc = cls_check("dl_cls_loss_fwd", score, ld, n_out, dtype, labels, N, a_pos, a_neg, gamma);
  if (rc != DL_OK) return rc;
  DL_CHECK_ARG(out2, DL_ERR_ARG, "dl_cls_loss_fwd: out2 is null");
  DL_CHECK_ARG(((uintptr_t)flags & 3) == 0, DL_ERR_ALIGN, "dl_cls_loss_fwd: flags not 4-byte aligned");
  const bool single = cls_single(N);
  DL_CHECK_ARG(single || (workspace && workspace_bytes >= dl_cls_loss_workspace_bytes(N)), DL_ERR_WORKSPACE,
               "dl_cls_loss_fwd: workspace too small");
  const int64_t nb = (N + CLS_THREADS - 1) / CLS_THREADS;
  ClsP c{};
  c.score = score; c.ld = ld; c.n_out = n_out; c.labels = labels; c.weights = weights; c.N = N;
  c.a_pos = a_pos; c.a_neg = a_neg; c.gamma = gamma;
  c.probs = probs; c.out2 = out2; c.partial = single ? nullptr : (float*)workspace; c.flags = flags; c.code = code;
  dlpairs::launch_by_dtype(dtype, cls_loss_fwd_kernel<bf16_t>, cls_loss_fwd_kernel<float>, single ? 1u : (uint32_t)nb, CLS_THREADS, s, c);
  if (!single) hipLaunchKernelGGL(cls_loss_final_kernel, dim3(1), dim3(CLS_THREADS), 0, s, (const float*)workspace, nb, out2);
  DL_CHECK_LAUNCH("dl_cls_loss_fwd");
  return DL_OK;
}

extern "C" int dl_cls_loss_bwd(const void* score, int64_t ld, int32_t n_out, int32_t dtype, const float* labels, const float* weights,
                               int64_t N, float a_pos, float a_neg, float gamma, const float* out2, const float* gout, void* dscore,
                               int64_t ldd, dl_stream stream) {
  hipStream_t s = (hipStream_t)stream;
  const int rc = cls_check("dl_cls_loss_bwd", score, ld, n_out, dtype, labels, N, a_pos, a_neg, gamma);
  if (rc != DL_OK) return rc;
  DL_CHECK_ARG(out2 && gout && dscore && ldd >= n_out, DL_ERR_ARG, "dl_cls_loss_bwd: null pointer or ldd < n_out");
  ClsP c{};
  c.score = score; c.ld = ld; c.n_out = n_out; c.labels = labels; c.weights = weights; c.N = N;
  c.a_pos = a_pos; c.a_neg = a_neg; c.gamma = gamma;
  c.stat = out2; c.gout = gout; c.dscore = dscore; c.ldd = ldd;
  dlpairs::launch_by_dtype(dtype, cls_loss_bwd_kernel<bf16_t>, cls_loss_bwd_kernel<float>, (uint32_t)((N + CLS_THREADS - 1) / CLS_THREADS),
                           CLS_THREADS, s, c);
  DL_CHECK_LAUNCH("dl_cls_loss_bwd");
  return DL_OK;
}
