// pgca_pairs.hip — pair-indexed PGCA attention core of the screening path (forward only), over dense per-entity codes
// (dl_pgca_pairs_fwd) or over a packed per-drug row store (dl_pgca_pairs_ragged_fwd: the resident drug library).
// See include/druglamp_hip.h for the addressing of both.
//
//   Pair n reads its queries from entity q_index[n] of Q and its keys / values from the segment of K / V that entity
//   kv_index[n] owns: the operands are the cached per-entity codes (druglamp_amd/screening.py), nothing is gathered per pair.
//   Where that segment lies is the one thing the two entry points differ in, and the kernel takes it from its `Keys` type
//   (pair_keys.cuh).  The workgroups of a short drug run fewer tiles; rows >= Lk of the last tile read the zero page, never the
//   next drug's rows.
//
//   pgca_pairs_kernel : one workgroup owns 64 * QT query rows of one pair; a wave owns 16 * QT of them.  The arithmetic is
//                       attention.hip's streamed forward (the three tile steps of tiles.cuh): 64-key tiles of K and V pass
//                       through two LDS buffers by LDS-DMA, scores in the transposed layout (S^T = K Q^T, lane (il, g) holds
//                       keys 4g + r of query il), online maximum / sum, O^T += V^T P^T with P^T straight from the
//                       accumulators.  The epilogue adds the fp32 bias and stores O at columns out_col0.. of the pair's rows;
//                       the same workgroup copies its rows of `left` (the protein sites) to columns 0..left_cols-1, so that
//                       `out` is the [sites | guided] concat the MHLA block takes.  The grid is n_pairs x ceil(Lq / (64 QT)).
//                       Workgroups of one pair are consecutive in the grid, and so are the pairs of a caller that orders
//                       them by key entity: they find K | V in L2.
//                       A pair whose index is out of range (DL_FLAG_PAIR_INDEX), or whose drug's table entry does not
//                       describe rows inside the store (DL_FLAG_KEY_TABLE), returns before it reads anything through the
//                       entry or writes anything; both tests are uniform for the workgroup.
#include "pair_keys.cuh"
#include "tiles.cuh"

namespace {
using namespace dltile;
using namespace dlpairs;

// the part of the launch that does not depend on where a pair's keys lie
struct PairsCommon {
  const char *Q, *K, *V, *left;
  char* out;
  const float* bias;
  const int32_t *qi, *ki;
  uint32_t* flags;
  int64_t q_es, q_rs, k_rs, v_rs, left_es, left_rs, out_ps, out_rs;
  int n_q, n_kv, Lq, bps;          // bps: workgroups per pair
  int left_chunks;                 // 16-byte chunks of a row of `left` (0: no copy)
  int out_col0;
  float scale;
};
template <typename Keys> struct PairsP : PairsCommon {
  Keys keys;
};

// LDS: two (K tile, V tile) pairs = 64 KB in bf16 (two workgroups per CU), 128 KB in fp32 (one: the parity dtype)
template <typename T, int HD, int QT, typename Keys>
__global__ __launch_bounds__(ATT_THREADS, 2) void pgca_pairs_kernel(const PairsP<Keys> p) {
  using TL = ATile<T, HD>;
  constexpr int NKF = HD / Mma<T>::KF, NDT = HD / 16;
  constexpr int QB = 4 * QT * 16;
  constexpr int BUF = 2 * KVB * TL::RB;                 // one (K tile, V tile) pair
  __shared__ __attribute__((aligned(16))) char smem[2 * BUF];

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, il = lane & 15, g = lane >> 4;
  const int n = blockIdx.x / p.bps, qb = blockIdx.x % p.bps;
  const int pi = p.qi[n], di = p.ki[n];
  KeySeg ks = {};
  const uint32_t bad = pair_guard(p, pi, di, p.v_rs, ks);
  if (bad) {
    flag_pair(p.flags, bad, qb == 0 && threadIdx.x == 0);
    return;
  }
  const int Lk = ks.Lk, tail_start = ks.tail_start;
  const float tail_bias = ks.tail_bias;
  const T* Qb = reinterpret_cast<const T*>(p.Q) + (int64_t)pi * p.q_es;
  const T* Kb = reinterpret_cast<const T*>(p.K) + ks.k_off;
  const T* Vb = reinterpret_cast<const T*>(p.V) + ks.v_off;
  T* Ob = reinterpret_cast<T*>(p.out) + (int64_t)n * p.out_ps;

  const int qw0 = qb * QB + wave * QT * 16;
  u32x4 qf[QT][NKF];
  load_q_frags(qf, Qb, p.q_rs, qw0, p.Lq, il, g);

  f32x4 o[NDT][QT];
#pragma unroll
  for (int d = 0; d < NDT; ++d)
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) o[d][qt] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m_run[QT], l_run[QT];
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) { m_run[qt] = -INFINITY; l_run[qt] = 0.f; }
  const float c = p.scale * LOG2E;

  const int nt = (Lk + KVB - 1) / KVB;
  auto stage = [&](int t, int buf) {
    char* b = smem + buf * BUF;
    dma_rows<T, HD, ATT_THREADS>(b, Kb + (int64_t)t * KVB * p.k_rs, p.k_rs, Lk - t * KVB, KVB);
    dma_rows<T, HD, ATT_THREADS>(b + KVB * TL::RB, Vb + (int64_t)t * KVB * p.v_rs, p.v_rs, Lk - t * KVB, KVB);
  };
  stage(0, 0);

  // the workgroup's rows of `left` -> columns 0 .. left_cols - 1 of the pair's rows, 16 bytes at a time (under the first tile's DMA)
  if (p.left_chunks) {
    const int r0 = qb * QB, rows = min(QB, p.Lq - r0), total = rows * p.left_chunks;
    const char* Lb = p.left + ((int64_t)pi * p.left_es + (int64_t)r0 * p.left_rs) * (int64_t)sizeof(T);
    char* Db = reinterpret_cast<char*>(Ob + (int64_t)r0 * p.out_rs);
    for (int e = threadIdx.x; e < total; e += ATT_THREADS) {
      const int r = e / p.left_chunks, ch = e - r * p.left_chunks;
      const u32x4 v = *reinterpret_cast<const u32x4*>(Lb + (int64_t)r * p.left_rs * (int64_t)sizeof(T) + ch * 16);
      *reinterpret_cast<u32x4*>(Db + (int64_t)r * p.out_rs * (int64_t)sizeof(T) + ch * 16) = v;
    }
  }

  for (int t = 0; t < nt; ++t) {
    const int k0 = t * KVB;
    vm_wait<0>();                                       // this wave's share of tile t's LDS-DMA (not implied by the barrier)
    __syncthreads();                                    // tile t has landed; everyone is done with the other buffer
    if (t + 1 < nt) stage(t + 1, (t + 1) & 1);
    const char* Ks = smem + (t & 1) * BUF;
    const char* Vs = Ks + KVB * TL::RB;
    f32x4 s[QT][NKT];
    fwd_scores<T, HD>(Ks, qf, s, il, g);                // S^T = K Q^T
    mask_keys(s, k0, Lk, tail_start, tail_bias, g);     // key multiplicities, key masking
    fwd_softmax(s, m_run, l_run, o, c);                 // online maximum / sum, rescale of o
    fwd_accumulate<T, HD>(Vs, s, o, il, g);             // O^T += V^T P^T
    // (no barrier here: the one at the top of the next iteration is what separates this tile's reads from the DMA that
    //  refills its buffer two iterations later)
  }
  // ---- epilogue: normalise, add the bias, store at columns out_col0 + d ----
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) {
    const int q = qw0 + qt * 16 + il;
    const float l = group4_sum(l_run[qt]);
    const float inv = 1.0f / l;
    if (q < p.Lq) {
      T* orow = Ob + (int64_t)q * p.out_rs + p.out_col0;
#pragma unroll
      for (int d = 0; d < NDT; ++d) {
        f32x4 v = o[d][qt] * inv;
        if (p.bias) v += *reinterpret_cast<const f32x4*>(p.bias + d * 16 + 4 * g);
        store4<T>(orow + d * 16 + 4 * g, v);
      }
    }
  }
}

template <typename Keys>
void launch_pairs(int dtype, const PairsP<Keys>& p, int n_pairs, hipStream_t s) {
  launch_by_dtype(dtype, pgca_pairs_kernel<bf16_t, 128, pair_qt<bf16_t>(), Keys>, pgca_pairs_kernel<float, 128, pair_qt<float>(), Keys>,
                  (uint32_t)n_pairs * (uint32_t)p.bps, ATT_THREADS, s, p);
}

// What dl_pgca_pairs_args and dl_pgca_pairs_ragged_args share (same field names): the checks, and the common block of the
// launch.  st / stn: the entry point's strides and their names, left_es and left_rs at st[left_at] and st[left_at + 1].
template <typename Args>
int pairs_common(const char* who, const Args* a, const int64_t* st, const char* const* stn, int n_st, int left_at, PairsCommon& p) {
  DL_TRY(pair_head_checks(who, a));
  DL_CHECK_ARG(a->left_cols >= 0 && a->left_cols % 8 == 0, DL_ERR_ALIGN, "%s: left_cols %d not a non-negative multiple of 8 elements", who,
               a->left_cols);
  DL_CHECK_ARG(a->out_col0 >= 0 && a->out_col0 % 8 == 0, DL_ERR_ALIGN, "%s: out_col0 %d not a non-negative multiple of 8 elements", who,
               a->out_col0);
  DL_CHECK_ARG((a->left != nullptr) == (a->left_cols > 0), DL_ERR_ARG, "%s: left and left_cols (%d) go together", who, a->left_cols);
  DL_CHECK_ARG(a->out_col0 >= a->left_cols, DL_ERR_ARG, "%s: out_col0 %d overlaps the left_cols %d copied columns", who, a->out_col0,
               a->left_cols);
  if (a->n_pairs == 0) return DL_OK;
  DL_CHECK_ARG(a->Q && a->K && a->V && a->out && a->q_index && a->kv_index, DL_ERR_ARG, "%s: null pointer (Q, K, V, out, q_index, kv_index)", who);
  DL_TRY(pair_stride_checks(who, a->dtype, st, stn, n_st, a->left ? -2 : left_at));    // (left_es / left_rs are not read without left)
  DL_CHECK_ARG((((uintptr_t)a->Q | (uintptr_t)a->K | (uintptr_t)a->V | (uintptr_t)a->out | (uintptr_t)a->left | (uintptr_t)a->bias) & 15) == 0,
               DL_ERR_ALIGN, "%s: Q / K / V / left / out / bias not 16-byte aligned", who);
  DL_TRY(pair_index_checks(who, a));
  DL_CHECK_ARG(a->out_rs >= (int64_t)a->out_col0 + a->head_dim, DL_ERR_SHAPE, "%s: out_rs %ld below out_col0 + head_dim = %d", who,
               (long)a->out_rs, a->out_col0 + a->head_dim);
  DL_TRY(pair_blocks(who, a, p.bps));
  fill_pair_head(a, p);
  p.V = (const char*)a->V; p.left = (const char*)a->left;
  p.out = (char*)a->out; p.bias = a->bias;
  p.v_rs = a->v_rs;
  p.left_es = a->left_es; p.left_rs = a->left_rs; p.out_ps = a->out_ps; p.out_rs = a->out_rs;
  p.left_chunks = a->left ? a->left_cols / (16 / (int)dl_dtype_size(a->dtype)) : 0;
  p.out_col0 = a->out_col0;
  return DL_OK;
}

}  // namespace

extern "C" int dl_pgca_pairs_fwd(const dl_pgca_pairs_args* a, dl_stream stream) {
  const char* who = "dl_pgca_pairs_fwd";
  DL_TRY(dense_head_checks(who, a));
  const int64_t st[] = {a->q_es, a->q_rs, a->k_es, a->k_rs, a->v_es, a->v_rs, a->left_es, a->left_rs, a->out_ps, a->out_rs};
  const char* stn[] = {"q_es", "q_rs", "k_es", "k_rs", "v_es", "v_rs", "left_es", "left_rs", "out_ps", "out_rs"};
  PairsP<DenseKeys> p = {};
  const int rc = pairs_common(who, a, st, stn, 10, 6, p);
  if (rc != DL_OK || a->n_pairs == 0) return rc;
  fill_dense_keys(a, a->v_es, true, p.keys);
  launch_pairs(a->dtype, p, a->n_pairs, (hipStream_t)stream);
  DL_CHECK_LAUNCH("dl_pgca_pairs_fwd");
  return DL_OK;
}

extern "C" int dl_pgca_pairs_ragged_fwd(const dl_pgca_pairs_ragged_args* a, dl_stream stream) {
  const char* who = "dl_pgca_pairs_ragged_fwd";
  DL_TRY(ragged_head_checks(who, a));
  const int64_t st[] = {a->q_es, a->q_rs, a->k_rs, a->v_rs, a->left_es, a->left_rs, a->out_ps, a->out_rs};
  const char* stn[] = {"q_es", "q_rs", "k_rs", "v_rs", "left_es", "left_rs", "out_ps", "out_rs"};
  PairsP<RaggedKeys> p = {};
  const int rc = pairs_common(who, a, st, stn, 8, 4, p);
  if (rc != DL_OK || a->n_pairs == 0) return rc;
  DL_TRY(fill_ragged_keys(who, a, p.keys));
  launch_pairs(a->dtype, p, a->n_pairs, (hipStream_t)stream);
  DL_CHECK_LAUNCH("dl_pgca_pairs_ragged_fwd");
  return DL_OK;
}
