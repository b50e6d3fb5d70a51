// attn_probs.hip — attention probability maps: P[q][k] = exp(scale q.k + log w_k - LSE_q), written as fp32 without touching V.
// See include/druglamp_hip.h (dl_attn_probs) for the problem / segment addressing, which is dl_attn_fwd's.
//
//   attn_lse_kernel   : LSE only — dl_attn_fwd's online max / sum over streamed key tiles, no V, no O.
//   attn_probs_kernel : one workgroup owns 64 query rows x up to 256 keys of one (segment, problem); a wave owns 16 query
//                       rows.  Scores are formed in the forward's transposed layout (S^T = K Q^T, lane (il, g) holds keys
//                       4g + r of query il), turned into probabilities with the KNOWN LSE (no online rescaling: key tiles are
//                       independent), and passed through a per-wave LDS tile so that the stores run along rows: one store
//                       instruction covers four rows x 64 consecutive floats (16 bytes per lane), not 16 rows x 16 bytes as
//                       the forward's raw-logit write does.  The kernel is bound by these stores.
//                       head_mean: the workgroup loops over the heads in ascending order and accumulates in registers
//                       (no atomics, fixed order); expand_tail: the tail keys' per-copy probabilities are written at their
//                       own columns (copy 0) and then streamed from the LDS tile to the columns of the further copies.
#include "tiles.cuh"

namespace {
using namespace dltile;

struct ProbsP {
  const char *Q, *K;
  const float* LSE;      // statistics the map kernel reads
  float* LSE_out;        // statistics kernel's output
  float* out;
  int64_t out_ld;
  int64_t q_ps, q_hs, q_rs, k_ps, k_hs, k_rs;
  int P, H, S, shift, Lq, Lk;
  float scale;
  int tail_start;        // Lk - key_tail_rows (== Lk: no key multiplicities)
  float tail_bias;       // log(w) / scale, added to the UNSCALED score of a tail key (as attention.hip)
  int tail_rows, copies; // expand_tail: every tail key is written `copies` times, `tail_rows` columns apart
  int expand;
  int vec;               // out and out_ld allow 16-byte stores
};

constexpr int KVB = 64, NKT = KVB / 16;   // keys per LDS tile, 16-key score tiles in it

// S^T = K Q^T of one 64-key tile for the wave's 16 query rows: lane (il, g) gets keys kt * 16 + 4 g + r of query il
template <typename T, int HD>
__device__ __forceinline__ void score_tile(const char* Ks, const u32x4 (&qf)[HD / Mma<T>::KF], f32x4 (&s)[NKT], int il, int g) {
  constexpr int NKF = HD / Mma<T>::KF;
#pragma unroll
  for (int kt = 0; kt < NKT; ++kt) {
    s[kt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kf = 0; kf < NKF; ++kf) s[kt] = Mma<T>::mma(frag_kc<T, HD>(Ks, kt * 16, kf, il, g), qf[kf], s[kt]);
  }
}

// =================================== statistics ================================================
// work item: (segment, problem, head, 64 query rows); the arithmetic of attn_fwd_kernel's running maximum and sum
template <typename T, int HD>
__global__ __launch_bounds__(ATT_THREADS, 2) void attn_lse_kernel(const ProbsP p) {
  using TL = ATile<T, HD>;
  constexpr int NKF = HD / Mma<T>::KF;
  constexpr int BUF = KVB * TL::RB;
  __shared__ __attribute__((aligned(16))) char smem[2 * BUF];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, il = lane & 15, g = lane >> 4;
  const int bps = (p.Lq + 63) / 64;
  const int seg = blockIdx.x / bps, qb = blockIdx.x % bps;
  const int h = blockIdx.y, pr = blockIdx.z;
  const int qprob = seg == 0 ? pr : (pr + p.shift) % p.P;
  const T* Qb = reinterpret_cast<const T*>(p.Q) + (int64_t)qprob * p.q_ps + (int64_t)h * p.q_hs;
  const T* Kb = reinterpret_cast<const T*>(p.K) + (int64_t)pr * p.k_ps + (int64_t)h * p.k_hs;
  const int q = qb * 64 + wave * 16 + il;
  u32x4 qf[1][NKF];                                     // (QT = 1 forms of the arrays the tile steps of tiles.cuh take)
#pragma unroll
  for (int kf = 0; kf < NKF; ++kf) qf[0][kf] = frag_global<T>(Qb + (int64_t)q * p.q_rs, q < p.Lq, kf, g);
  float m_run[1] = {-INFINITY}, l_run[1] = {0.f};
  const float c = p.scale * LOG2E;
  const int nt = (p.Lk + KVB - 1) / KVB;
  dma_rows<T, HD, ATT_THREADS>(smem, Kb, p.k_rs, p.Lk, KVB);
  for (int t = 0; t < nt; ++t) {
    const int k0 = t * KVB;
    vm_wait<0>();                                       // this wave's share of tile t (the compiler's own wait in front of the
    __syncthreads();                                    // barrier covers LDS only); then: tile t has landed, the other buffer is free
    if (t + 1 < nt)
      dma_rows<T, HD, ATT_THREADS>(smem + ((t + 1) & 1) * BUF, Kb + (int64_t)(k0 + KVB) * p.k_rs, p.k_rs, p.Lk - k0 - KVB, KVB);
    f32x4 s[1][NKT];
    score_tile<T, HD>(smem + (t & 1) * BUF, qf[0], s[0], il, g);
    mask_keys(s, k0, p.Lk, p.tail_start, p.tail_bias, g);
    sweep_stats(s, m_run, l_run, c);
  }
  const float l = group4_sum(l_run[0]);
  if (q < p.Lq && g == 0) p.LSE_out[(((int64_t)seg * p.P + pr) * p.H + h) * p.Lq + q] = m_run[0] * p.scale + logf(l);
}

// =================================== probabilities =============================================
constexpr int KCT = 4;                    // key tiles per workgroup (256 keys): the head-mean accumulators of a lane
constexpr int SP = KVB + 4;               // pitch of the per-wave staging tile in floats: 16-byte writes of 16 rows spread over the banks

// HM: one workgroup per (segment, problem, query block, key chunk) loops over all heads; else one per head as well.
// LDS: two K tiles + the staging tiles = 33 KB (bf16, head_dim 64), 49 KB (bf16 128 / fp32 64), 81 KB (fp32, head_dim 128:
// ONE workgroup per CU there, whatever the launch bounds allow — the parity dtype, not the timed one)
template <typename T, int HD, bool HM>
__global__ __launch_bounds__(ATT_THREADS, 2) void attn_probs_kernel(const ProbsP p) {
  using TL = ATile<T, HD>;
  constexpr int NKF = HD / Mma<T>::KF;
  constexpr int BUF = KVB * TL::RB;
  __shared__ __attribute__((aligned(16))) char smem[2 * BUF];
  __shared__ __attribute__((aligned(16))) float stage_all[4 * 16 * SP];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, il = lane & 15, g = lane >> 4;
  const int nqb = (p.Lq + 63) / 64, nkc = (p.Lk + KCT * KVB - 1) / (KCT * KVB);
  int bx = blockIdx.x;
  const int kc = bx % nkc; bx /= nkc;
  const int qb = bx % nqb, seg = bx / nqb;
  const int h0 = HM ? 0 : (int)blockIdx.y, nh = HM ? p.H : 1;
  const int pr = blockIdx.z;
  const int qprob = seg == 0 ? pr : (pr + p.shift) % p.P;
  const int qw0 = qb * 64 + wave * 16, q = qw0 + il;
  const int kbase = kc * KCT * KVB;
  const int ntl = min(KCT, (p.Lk - kbase + KVB - 1) / KVB);
  const int total = nh * ntl;
  const float c = p.scale * LOG2E;
  float* st = stage_all + wave * 16 * SP;
  float* orow0 = p.out + (((int64_t)seg * p.P + pr) * (HM ? 1 : p.H) + (HM ? 0 : h0)) * p.Lq * p.out_ld;   // row q = 0 of this map

  // one 16 x 64 tile of the wave (lane (il, g): keys 4 g + r of each 16-key tile of query il) -> rows of the output
  auto emit = [&](const f32x4 (&v)[NKT], int k0) {
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt) *reinterpret_cast<f32x4*>(st + il * SP + kt * 16 + 4 * g) = v[kt];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const int c4 = il * 4, col = k0 + c4;
#pragma unroll
    for (int ps = 0; ps < 4; ++ps) {
      const int r = ps * 4 + g, qq = qw0 + r;
      if (qq < p.Lq && col < p.Lk) {
        const f32x4 x = *reinterpret_cast<const f32x4*>(st + r * SP + c4);
        float* dst = orow0 + (int64_t)qq * p.out_ld + col;
        if (p.vec && col + 4 <= p.Lk) {
          *reinterpret_cast<f32x4*>(dst) = x;
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (col + e < p.Lk) dst[e] = x[e];
        }
      }
    }
    if (p.expand && p.copies > 1 && k0 + KVB > p.tail_start) {
      // the tail keys [a, b) of this tile: copy i of tail key j lives at column lead + i t + j, i.e. (i t) columns to the
      // right of copy 0.  Lanes walk the (copy, key) pairs of a row in column order: consecutive lanes write consecutive
      // columns (one run per copy; ONE run for the whole row when the tile holds the whole tail)
      const int a = max(k0, p.tail_start), b = min(k0 + KVB, p.Lk), n = b - a;
      // units of 4 columns (16-byte stores) when the tile holds the whole tail and every copy starts on a 16-byte boundary
      const bool quad = p.vec && n == p.tail_rows && ((n | a) & 3) == 0;
      const int nu = quad ? n >> 2 : n;
      const int pairs = nu * (p.copies - 1);
      const int i0 = lane / nu, j0 = lane - i0 * nu, di = 64 / nu, dj = 64 - di * nu;
      const int rows = min(16, p.Lq - qw0);
      for (int r = 0; r < rows; ++r) {
        const float* src = st + r * SP + (a - k0);
        float* dst = orow0 + (int64_t)(qw0 + r) * p.out_ld + a;
        int ii = i0 + 1, jj = j0;
        for (int e = lane; e < pairs; e += 64) {
          if (quad) *reinterpret_cast<f32x4*>(dst + (int64_t)ii * p.tail_rows + 4 * jj) = *reinterpret_cast<const f32x4*>(src + 4 * jj);
          else dst[(int64_t)ii * p.tail_rows + jj] = src[jj];
          ii += di; jj += dj;
          if (jj >= nu) { jj -= nu; ++ii; }
        }
      }
    }
  };

  auto stage_tile = [&](int i) {
    const int hh = h0 + i / ntl, k0 = kbase + (i % ntl) * KVB;
    const T* Kb = reinterpret_cast<const T*>(p.K) + (int64_t)pr * p.k_ps + (int64_t)hh * p.k_hs + (int64_t)k0 * p.k_rs;
    dma_rows<T, HD, ATT_THREADS>(smem + (i & 1) * BUF, Kb, p.k_rs, p.Lk - k0, KVB);
  };

  f32x4 acc[HM ? KCT : 1][NKT];
  stage_tile(0);
  int i = 0;
  for (int hh = 0; hh < nh; ++hh) {
    const int h = h0 + hh;
    const T* Qb = reinterpret_cast<const T*>(p.Q) + (int64_t)qprob * p.q_ps + (int64_t)h * p.q_hs;
    u32x4 qf[NKF];
#pragma unroll
    for (int kf = 0; kf < NKF; ++kf) qf[kf] = frag_global<T>(Qb + (int64_t)q * p.q_rs, q < p.Lq, kf, g);
    const float lse2 = q < p.Lq ? p.LSE[(((int64_t)seg * p.P + pr) * p.H + h) * p.Lq + q] * LOG2E : INFINITY;
#pragma unroll
    for (int t = 0; t < KCT; ++t) {
      if (t < ntl) {                                    // (the same for the whole workgroup)
        const int k0 = kbase + t * KVB;
        vm_wait<0>();                                   // this wave's share of tile i's LDS-DMA (not implied by the barrier)
        __syncthreads();                                // tile i has landed; everyone is done with the other buffer
        if (i + 1 < total) stage_tile(i + 1);
        f32x4 s[NKT];
        score_tile<T, HD>(smem + (i & 1) * BUF, qf, s, il, g);
        // key multiplicities: a tail key carries the mass of the keys it stands for, except where each copy gets its own column
        if (!p.expand && k0 + KVB > p.tail_start) {
#pragma unroll
          for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r)
              if (k0 + kt * 16 + 4 * g + r >= p.tail_start) s[kt][r] += p.tail_bias;
        }
#pragma unroll
        for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
          for (int r = 0; r < 4; ++r) s[kt][r] = fast_exp2(s[kt][r] * c - lse2);
        if constexpr (HM) {
#pragma unroll
          for (int kt = 0; kt < NKT; ++kt) acc[t][kt] = hh == 0 ? s[kt] : acc[t][kt] + s[kt];
        } else {
          emit(s, k0);
        }
        ++i;
      }
    }
  }
  if constexpr (HM) {
    const float inv = 1.0f / (float)p.H;
#pragma unroll
    for (int t = 0; t < KCT; ++t)
      if (t < ntl) {
#pragma unroll
        for (int kt = 0; kt < NKT; ++kt) acc[t][kt] *= inv;
        emit(acc[t], kbase + t * KVB);
      }
  }
}

template <typename T, int HD>
void launch_probs(const ProbsP& p, bool need_lse, bool head_mean, hipStream_t s) {
  const uint32_t nqb = (uint32_t)((p.Lq + 63) / 64), nkc = (uint32_t)((p.Lk + KCT * KVB - 1) / (KCT * KVB));
  if (need_lse)
    hipLaunchKernelGGL((attn_lse_kernel<T, HD>), dim3((uint32_t)p.S * nqb, (uint32_t)p.H, (uint32_t)p.P), dim3(ATT_THREADS), 0, s, p);
  if (head_mean && p.H > 1)
    hipLaunchKernelGGL((attn_probs_kernel<T, HD, true>), dim3((uint32_t)p.S * nqb * nkc, 1u, (uint32_t)p.P), dim3(ATT_THREADS), 0, s, p);
  else                                                  // (the mean over one head is that head's map, and the layouts coincide)
    hipLaunchKernelGGL((attn_probs_kernel<T, HD, false>), dim3((uint32_t)p.S * nqb * nkc, (uint32_t)p.H, (uint32_t)p.P), dim3(ATT_THREADS), 0, s, p);
}

// columns of a row of the map; < 0: not representable
int64_t probs_columns(const dl_attn_probs_args* a) {
  if (!a->expand_tail || a->key_tail_rows <= 0) return a->Lk;
  return (int64_t)(a->Lk - a->key_tail_rows) + (int64_t)a->key_tail_rows * (int64_t)a->key_tail_weight;
}

}  // namespace

extern "C" size_t dl_attn_probs_workspace_bytes(const dl_attn_probs_args* a) {
  if (!a || a->n_segments <= 0 || a->n_problems <= 0 || a->n_heads <= 0 || a->Lq <= 0) return 0;
  return sizeof(float) * (size_t)a->n_segments * (size_t)a->n_problems * (size_t)a->n_heads * (size_t)a->Lq;
}

extern "C" int dl_attn_probs(const dl_attn_probs_args* a, dl_stream stream) {
  hipStream_t s = (hipStream_t)stream;
  const char* who = "dl_attn_probs";
  DL_CHECK_ARG(a && a->Q && a->K && a->out, DL_ERR_ARG, "%s: null pointer", who);
  DL_CHECK_ARG(a->dtype == DL_F32 || a->dtype == DL_BF16, DL_ERR_ARG, "%s: bad dtype", who);
  DL_CHECK_ARG(a->head_dim == 64 || a->head_dim == 128, DL_ERR_UNSUPPORTED, "%s: head_dim %d not in {64,128}", who, a->head_dim);
  DL_CHECK_ARG(a->n_segments == 1 || a->n_segments == 2, DL_ERR_ARG, "%s: n_segments must be 1 or 2", who);
  DL_CHECK_ARG(a->n_problems > 0 && a->n_heads > 0 && a->Lq > 0 && a->Lk > 0 && a->n_problems <= 65535 && a->n_heads <= 65535,
               DL_ERR_SHAPE, "%s: bad sizes", who);
  DL_CHECK_ARG(a->n_segments == 1 || (a->partner_shift >= 0 && a->partner_shift < a->n_problems), DL_ERR_ARG,
               "%s: bad partner_shift", who);
  const int epc = 16 / (int)dl_dtype_size(a->dtype);
  const int64_t st[] = {a->q_ps, a->q_hs, a->q_rs, a->k_ps, a->k_hs, a->k_rs};
  for (int i = 0; i < 6; ++i)
    DL_CHECK_ARG(st[i] % epc == 0, DL_ERR_ALIGN, "%s: stride #%d (%ld) not a multiple of %d elements", who, i, (long)st[i], epc);
  DL_CHECK_ARG(((uintptr_t)a->Q & 15) == 0 && ((uintptr_t)a->K & 15) == 0, DL_ERR_ALIGN, "%s: Q / K not 16-byte aligned", who);
  DL_CHECK_ARG(((uintptr_t)a->out & 3) == 0, DL_ERR_ALIGN, "%s: out not 4-byte aligned", who);
  DL_CHECK_ARG(a->scale > 0.f, DL_ERR_ARG, "%s: scale must be positive", who);
  DL_CHECK_ARG((a->head_mean == 0 || a->head_mean == 1) && (a->expand_tail == 0 || a->expand_tail == 1), DL_ERR_ARG,
               "%s: head_mean and expand_tail are 0 or 1", who);
  DL_CHECK_ARG(a->key_tail_rows >= 0 && a->key_tail_rows <= a->Lk && (a->key_tail_rows == 0 || a->key_tail_weight >= 1.f),
               DL_ERR_ARG, "%s: key_tail_rows in [0, Lk], key_tail_weight >= 1", who);
  DL_CHECK_ARG(a->key_tail_rows == 0 || a->n_segments == 1, DL_ERR_UNSUPPORTED, "%s: key multiplicities with one segment only", who);
  const bool expand = a->expand_tail && a->key_tail_rows > 0;
  DL_CHECK_ARG(!expand || (a->key_tail_weight <= 16777216.f && a->key_tail_weight == (float)(int64_t)a->key_tail_weight), DL_ERR_ARG,
               "%s: expand_tail needs a whole key_tail_weight (got %g)", who, (double)a->key_tail_weight);
  const int64_t cols = probs_columns(a);
  DL_CHECK_ARG(cols <= INT32_MAX, DL_ERR_SHAPE, "%s: %ld expanded columns", who, (long)cols);
  DL_CHECK_ARG(a->out_ld >= cols, DL_ERR_SHAPE, "%s: out_ld %ld below the %ld columns of a row", who, (long)a->out_ld, (long)cols);
  const int nqb = (a->Lq + 63) / 64, nkc = (a->Lk + KCT * KVB - 1) / (KCT * KVB);
  DL_CHECK_ARG((int64_t)a->n_segments * nqb * nkc <= INT32_MAX, DL_ERR_SHAPE, "%s: too many workgroups", who);
  if (!a->LSE) {
    DL_CHECK_ARG(a->workspace && a->workspace_bytes >= dl_attn_probs_workspace_bytes(a), DL_ERR_WORKSPACE,
                 "%s: LSE == NULL needs a workspace of %zu bytes (got %zu)", who, dl_attn_probs_workspace_bytes(a),
                 a->workspace ? a->workspace_bytes : (size_t)0);
    DL_CHECK_ARG(((uintptr_t)a->workspace & 3) == 0, DL_ERR_ALIGN, "%s: workspace not 4-byte aligned", who);
  }
  ProbsP p = {};
  p.Q = (const char*)a->Q; p.K = (const char*)a->K;
  p.LSE_out = a->LSE ? nullptr : (float*)a->workspace;
  p.LSE = a->LSE ? a->LSE : (const float*)a->workspace;
  p.out = a->out; p.out_ld = a->out_ld;
  p.q_ps = a->q_ps; p.q_hs = a->q_hs; p.q_rs = a->q_rs; p.k_ps = a->k_ps; p.k_hs = a->k_hs; p.k_rs = a->k_rs;
  p.P = a->n_problems; p.H = a->n_heads; p.S = a->n_segments; p.shift = a->n_segments == 2 ? a->partner_shift : 0;
  p.Lq = a->Lq; p.Lk = a->Lk; p.scale = a->scale;
  p.tail_start = a->Lk - a->key_tail_rows;
  p.tail_bias = a->key_tail_rows ? logf(a->key_tail_weight) / a->scale : 0.f;
  p.tail_rows = a->key_tail_rows;
  p.expand = expand ? 1 : 0;
  p.copies = expand ? (int)a->key_tail_weight : 1;
  p.vec = (((uintptr_t)a->out & 15) == 0 && a->out_ld % 4 == 0) ? 1 : 0;
  const bool need_lse = a->LSE == nullptr, hm = a->head_mean != 0;
  if (a->dtype == DL_BF16) {
    if (a->head_dim == 64) launch_probs<bf16_t, 64>(p, need_lse, hm, s);
    else launch_probs<bf16_t, 128>(p, need_lse, hm, s);
  } else {
    if (a->head_dim == 64) launch_probs<float, 64>(p, need_lse, hm, s);
    else launch_probs<float, 128>(p, need_lse, hm, s);
  }
  DL_CHECK_LAUNCH("dl_attn_probs");
  return DL_OK;
}
