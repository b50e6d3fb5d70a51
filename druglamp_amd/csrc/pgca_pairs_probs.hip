// pgca_pairs_probs.hip — pair-indexed PGCA probability maps of the screening path: for pair n the softmax weights
// P[r][k] = exp(scale q_r.k_k + log w_k - LSE_r) of protein q_index[n] over the keys of drug kv_index[n], written as fp32,
// over dense per-entity codes (dl_pgca_pairs_probs) or over a packed per-drug row store (dl_pgca_pairs_ragged_probs: the
// resident drug library).  See include/druglamp_hip.h for the addressing of both.  No value row is read.
//
//   The operands, the `Keys` types and the guards are pair_keys.cuh's; what is written is what attn_probs.hip writes for one
//   (problem, head) — here with every drug's own key count and multiplicity.
//
//   pgca_pairs_probs_kernel : one workgroup owns 64 * QT query rows of one pair; a wave owns 16 * QT of them.  It sweeps the
//                       drug's 64-key tiles TWICE through two LDS buffers by LDS-DMA (one pipeline of 2 * nt tiles):
//                         sweep 1  scores in the transposed layout (S^T = K Q^T, lane (il, g) holds keys 4g + r of query
//                                  il), running maximum and sum; the LSE stays in registers;
//                         sweep 2  the scores again (a drug has at most ~520 distinct keys: the second read comes from L2),
//                                  exp2(s c - lse2), passed through a per-wave LDS tile so that the stores run along rows
//                                  (16 bytes per lane where `out` allows it) — attn_probs_kernel's emit, with the tail keys'
//                                  further copies streamed from that tile under expand_tail.
//                       No workspace, no second launch, no atomics on `out`: two calls agree bitwise.  The columns between
//                       the drug's own count and out_cols are zero filled by the same workgroup (plain vector stores, under
//                       the first tile's DMA).  The grid is n_pairs x ceil(Lq / (64 QT)).
//                       The multiplicity is tested under expand_tail only, and the tail bias is KeySeg's (the host's for dense
//                       keys); there is no bound on the stored keys.
#include "pair_keys.cuh"

namespace {
using namespace dltile;
using namespace dlpairs;

// the part of the launch that does not depend on where a pair's keys lie
struct MapCommon {
  const char *Q, *K;
  float* out;
  const int32_t *qi, *ki;
  uint32_t* flags;
  int64_t q_es, q_rs, k_rs, out_ps, out_rs;
  int n_q, n_kv, Lq, bps;          // bps: workgroups per pair
  int out_cols;
  int expand;                      // expand_tail: every copy of a tail key gets its own column
  int vec;                         // out, out_ps and out_rs allow 16-byte stores
  float scale;
  float dense_w;                   // DenseKeys: the launch-wide multiplicity (RaggedKeys reads the drug's own)
};
template <typename Keys> struct MapP : MapCommon {
  Keys keys;
};

constexpr int SP = KVB + 4;               // pitch of the per-wave staging tile in floats (as attn_probs.hip)

// LDS: two K tiles + the staging tiles = 49 KB in bf16 (three workgroups per CU), 81 KB in fp32 (one: the parity dtype)
template <typename T, int HD, int QT, typename Keys>
__global__ __launch_bounds__(ATT_THREADS, 2) void pgca_pairs_probs_kernel(const MapP<Keys> p) {
  using TL = ATile<T, HD>;
  constexpr int NKF = HD / Mma<T>::KF;
  constexpr int QB = 4 * QT * 16;
  constexpr int BUF = KVB * TL::RB;
  __shared__ __attribute__((aligned(16))) char smem[2 * BUF];
  __shared__ __attribute__((aligned(16))) float stage_all[4 * 16 * SP];

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, il = lane & 15, g = lane >> 4;
  const int n = blockIdx.x / p.bps, qb = blockIdx.x % p.bps;
  const int pi = p.qi[n], di = p.ki[n];
  KeySeg ks = {};
  int copies, cols;
  float unused_bias;
  const uint32_t bad = map_guard(p, pi, di, p.expand != 0, INT32_MAX, ks, copies, cols, unused_bias);
  if (bad) {
    flag_pair(p.flags, bad, qb == 0 && threadIdx.x == 0);
    return;
  }
  const int Lk = ks.Lk, tail_start = ks.tail_start, tail_rows = Lk - tail_start;
  const float tail_bias = ks.tail_bias;
  const T* Qb = reinterpret_cast<const T*>(p.Q) + (int64_t)pi * p.q_es;
  const T* Kb = reinterpret_cast<const T*>(p.K) + ks.k_off;
  float* Ob = p.out + (int64_t)n * p.out_ps;            // row 0 of this pair's map

  const int qw0 = qb * QB + wave * QT * 16;
  u32x4 qf[QT][NKF];
  load_q_frags(qf, Qb, p.q_rs, qw0, p.Lq, il, g);
  const float c = p.scale * LOG2E;
  const int nt = (Lk + KVB - 1) / KVB;
  auto stage = [&](int i) {                             // pipeline step i: tile i % nt into buffer i & 1
    const int t = i < nt ? i : i - nt;
    dma_rows<T, HD, ATT_THREADS>(smem + (i & 1) * BUF, Kb + (int64_t)t * KVB * p.k_rs, p.k_rs, Lk - t * KVB, KVB);
  };
  stage(0);

  // columns cols .. out_cols - 1 of the workgroup's rows <- +0.0f (under the first tile's DMA).  A wave takes every fourth row,
  // its lanes consecutive columns: 16 bytes each between the first and the last 16-byte boundary where `out` allows it.
  if (cols < p.out_cols) {
    const int r0 = qb * QB, rows = min(QB, p.Lq - r0);
    const int a4 = p.vec ? min(p.out_cols, (cols + 3) & ~3) : p.out_cols;     // first 16-byte boundary (vec only)
    const int b4 = a4 + ((p.out_cols - a4) & ~3);                             // last one
    for (int r = wave; r < rows; r += 4) {
      float* row = Ob + (int64_t)(r0 + r) * p.out_rs;
      for (int col = cols + lane; col < a4; col += 64) row[col] = 0.f;
      for (int col = a4 + 4 * lane; col < b4; col += 256) *reinterpret_cast<f32x4*>(row + col) = f32x4{0.f, 0.f, 0.f, 0.f};
      for (int col = b4 + lane; col < p.out_cols; col += 64) row[col] = 0.f;
    }
  }

  float* st = stage_all + wave * 16 * SP;
  // one 16 x 64 tile of the wave's query tile at row qr0 (lane (il, g): keys 4 g + r of each 16-key tile of query il) -> rows of
  // the output; attn_probs_kernel's emit with this drug's Lk, tail and copies
  auto emit = [&](const f32x4 (&v)[NKT], int qr0, int k0) {
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt) *reinterpret_cast<f32x4*>(st + il * SP + kt * 16 + 4 * g) = v[kt];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const int c4 = il * 4, col = k0 + c4;
#pragma unroll
    for (int ps = 0; ps < 4; ++ps) {
      const int r = ps * 4 + g, qq = qr0 + r;
      if (qq < p.Lq && col < Lk) {
        const f32x4 x = *reinterpret_cast<const f32x4*>(st + r * SP + c4);
        float* dst = Ob + (int64_t)qq * p.out_rs + col;
        if (p.vec && col + 4 <= Lk) {
          *reinterpret_cast<f32x4*>(dst) = x;
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (col + e < Lk) dst[e] = x[e];
        }
      }
    }
    if (copies > 1 && k0 + KVB > tail_start) {
      // the tail keys [a, b) of this tile: copy i of tail key j lives at column lead + i t + j, i.e. (i t) columns to the
      // right of copy 0.  Lanes walk the (copy, key) pairs of a row in column order: consecutive lanes write consecutive
      // columns (one run per copy; ONE run for the whole row when the tile holds the whole tail)
      const int a = max(k0, tail_start), b = min(k0 + KVB, Lk), nk = b - a;
      // units of 4 columns (16-byte stores) when the tile holds the whole tail and every copy starts on a 16-byte boundary
      const bool quad = p.vec && nk == tail_rows && ((nk | a) & 3) == 0;
      const int nu = quad ? nk >> 2 : nk;
      const int pairs = nu * (copies - 1);
      const int i0 = lane / nu, j0 = lane - i0 * nu, di_ = 64 / nu, dj = 64 - di_ * nu;
      const int rows = min(16, p.Lq - qr0);
      for (int r = 0; r < rows; ++r) {
        const float* src = st + r * SP + (a - k0);
        float* dst = Ob + (int64_t)(qr0 + r) * p.out_rs + a;
        int ii = i0 + 1, jj = j0;
        for (int e = lane; e < pairs; e += 64) {
          if (quad) *reinterpret_cast<f32x4*>(dst + (int64_t)ii * tail_rows + 4 * jj) = *reinterpret_cast<const f32x4*>(src + 4 * jj);
          else dst[(int64_t)ii * tail_rows + jj] = src[jj];
          ii += di_; jj += dj;
          if (jj >= nu) { jj -= nu; ++ii; }
        }
      }
    }
  };

  float m_run[QT], l_run[QT], lse2[QT];
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) { m_run[qt] = -INFINITY; l_run[qt] = 0.f; lse2[qt] = 0.f; }

  for (int i = 0; i < 2 * nt; ++i) {
    const bool second = i >= nt;                        // (the same for the whole workgroup)
    const int k0 = (second ? i - nt : i) * KVB;
    vm_wait<0>();                                       // this wave's share of step i's LDS-DMA (not implied by the barrier)
    __syncthreads();                                    // the tile has landed; everyone is done with the other buffer
    if (i + 1 < 2 * nt) stage(i + 1);
    if (i == nt) {                                      // between the sweeps
#pragma unroll
      for (int qt = 0; qt < QT; ++qt) lse2_join(m_run[qt], l_run[qt], p.scale, lse2[qt]);
    }
    f32x4 s[QT][NKT];
    fwd_scores<T, HD>(smem + (i & 1) * BUF, qf, s, il, g);      // S^T = K Q^T
    if (!second) {
      // ---- sweep 1: key multiplicities, key masking (mask_keys(), kept in place), running maximum and sum ----
      if (k0 + KVB > tail_start || k0 + KVB > Lk) {
#pragma unroll
        for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int key = k0 + kt * 16 + 4 * g + r;
#pragma unroll
            for (int qt = 0; qt < QT; ++qt) {
              if (key >= tail_start) s[qt][kt][r] += tail_bias;
              if (key >= Lk) s[qt][kt][r] = -INFINITY;
            }
          }
      }
      sweep_stats(s, m_run, l_run, c);
    } else {
      // ---- sweep 2: a tail key carries the mass of the keys it stands for, except where each copy gets its own column ----
      if (!p.expand) bias_tail_keys(s, k0, tail_start, tail_bias, g);
#pragma unroll
      for (int qt = 0; qt < QT; ++qt) {
#pragma unroll
        for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
          for (int r = 0; r < 4; ++r) s[qt][kt][r] = fast_exp2(s[qt][kt][r] * c - lse2[qt]);
        emit(s[qt], qw0 + qt * 16, k0);
      }
    }
    // (no barrier here: the one at the top of the next iteration is what separates this tile's reads from the DMA that
    //  refills its buffer two iterations later; the staging tiles are per wave)
  }
}

template <typename Keys>
void launch_maps(int dtype, const MapP<Keys>& p, int n_pairs, hipStream_t s) {
  launch_by_dtype(dtype, pgca_pairs_probs_kernel<bf16_t, 128, pair_qt<bf16_t>(), Keys>, pgca_pairs_probs_kernel<float, 128, pair_qt<float>(), Keys>,
                  (uint32_t)n_pairs * (uint32_t)p.bps, ATT_THREADS, s, p);
}

// What dl_pgca_pairs_probs_args and dl_pgca_pairs_ragged_probs_args share (same field names): the checks, and the common block
// of the launch.  st / stn: the entry point's operand strides and their names.
template <typename Args>
int maps_common(const char* who, const Args* a, const int64_t* st, const char* const* stn, int n_st, MapCommon& p) {
  DL_TRY(pair_head_checks(who, a));
  DL_CHECK_ARG(a->out_cols > 0, DL_ERR_SHAPE, "%s: out_cols %d must be positive", who, a->out_cols);
  DL_CHECK_ARG(a->expand_tail == 0 || a->expand_tail == 1, DL_ERR_ARG, "%s: expand_tail %d is not 0 or 1", who, a->expand_tail);
  if (a->n_pairs == 0) return DL_OK;
  DL_CHECK_ARG(a->Q && a->K && a->out && a->q_index && a->kv_index, DL_ERR_ARG, "%s: null pointer (Q, K, out, q_index, kv_index)", who);
  DL_TRY(pair_stride_checks(who, a->dtype, st, stn, n_st));
  DL_CHECK_ARG((((uintptr_t)a->Q | (uintptr_t)a->K) & 15) == 0, DL_ERR_ALIGN, "%s: Q / K not 16-byte aligned", who);
  DL_CHECK_ARG(((uintptr_t)a->out & 3) == 0, DL_ERR_ALIGN, "%s: out not 4-byte aligned", who);
  DL_TRY(pair_index_checks(who, a));
  DL_CHECK_ARG(a->out_ps >= 0, DL_ERR_SHAPE, "%s: out_ps %ld is negative", who, (long)a->out_ps);
  DL_CHECK_ARG(a->out_rs >= (int64_t)a->out_cols, DL_ERR_SHAPE, "%s: out_rs %ld below out_cols = %d", who, (long)a->out_rs, a->out_cols);
  DL_TRY(pair_blocks(who, a, p.bps));
  fill_pair_head(a, p);
  p.out = a->out; p.out_ps = a->out_ps; p.out_rs = a->out_rs;
  p.out_cols = a->out_cols;
  p.expand = a->expand_tail;
  p.vec = (((uintptr_t)a->out & 15) == 0 && a->out_ps % 4 == 0 && a->out_rs % 4 == 0) ? 1 : 0;
  p.dense_w = 1.f;
  return DL_OK;
}

}  // namespace

extern "C" int dl_pgca_pairs_probs(const dl_pgca_pairs_probs_args* a, dl_stream stream) {
  const char* who = "dl_pgca_pairs_probs";
  DL_TRY(dense_head_checks(who, a));
  const int64_t st[] = {a->q_es, a->q_rs, a->k_es, a->k_rs};
  const char* stn[] = {"q_es", "q_rs", "k_es", "k_rs"};
  MapP<DenseKeys> p = {};
  DL_TRY(maps_common(who, a, st, stn, 4, p));
  DL_TRY(dense_cols_check(who, a, a->expand_tail && a->key_tail_rows > 0, "expand_tail needs", "map"));
  if (a->n_pairs == 0) return DL_OK;
  p.dense_w = fill_dense_keys(a, 0, true, p.keys);
  launch_maps(a->dtype, p, a->n_pairs, (hipStream_t)stream);
  DL_CHECK_LAUNCH("dl_pgca_pairs_probs");
  return DL_OK;
}

extern "C" int dl_pgca_pairs_ragged_probs(const dl_pgca_pairs_ragged_probs_args* a, dl_stream stream) {
  const char* who = "dl_pgca_pairs_ragged_probs";
  DL_TRY(ragged_head_checks(who, a));
  const int64_t st[] = {a->q_es, a->q_rs, a->k_rs};
  const char* stn[] = {"q_es", "q_rs", "k_rs"};
  MapP<RaggedKeys> p = {};
  const int rc = maps_common(who, a, st, stn, 3, p);
  if (rc != DL_OK || a->n_pairs == 0) return rc;
  DL_TRY(fill_ragged_keys(who, a, p.keys));
  launch_maps(a->dtype, p, a->n_pairs, (hipStream_t)stream);
  DL_CHECK_LAUNCH("dl_pgca_pairs_ragged_probs");
  return DL_OK;
}
