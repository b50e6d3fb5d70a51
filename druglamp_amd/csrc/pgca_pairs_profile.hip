// pgca_pairs_profile.hip — hit profiles of the screening path: for pair n the two reductions of the PGCA probability map that
// interpretation asks for, computed WITHOUT writing the map.  With P (Lq, F) the map pgca_pairs_probs.hip writes under
// expand_tail (F = lead + t w columns; every copy of tail key j carries exp(scale q.k_j - LSE)):
//     key_mass [n][c]  = (1 / Lq) sum_r P[r][c]        c < F, +0.0f for F <= c < out_cols    (fp32; sums to 1 over c)
//     site_peak[n][r]  = max_c P[r][c]                 r < Lq                                 (fp32)
//     site_key [n][r]  = the smallest column at which the computed P[r][.] attains it (int32): copy 0 of a tail key is at column
//                        lead + j, in front of every further copy, so this is an index into the drug's STORED keys.
// over dense per-entity codes (dl_pgca_pairs_profile) or the packed per-drug row store (dl_pgca_pairs_ragged_profile); see
// include/druglamp_hip.h for the addressing.  About 4 KB per pair instead of the map's 512 KB.
//
//   pgca_pairs_profile_kernel : ONE workgroup of eight waves per pair (the one-workgroup scaffolding of pair_keys.cuh); it loops
//                       over the pair's blocks of 128 * QT query rows (a wave owns 16 * QT of a block) and sweeps the drug's
//                       64-key tiles twice per block through two LDS buffers by LDS-DMA (one pipeline over all blocks; from the
//                       second pass on the tiles come from L2):
//                         sweep 1  the tile steps of tiles.cuh with the tail bias (taken on the device for both Keys types, so
//                                  that the two entry points agree bitwise); the LSE stays in registers;
//                         sweep 2  the scores again, p = exp2(s c - lse2) WITHOUT the tail bias (one copy's probability), and
//                                  instead of a store: (a) per lane the largest p over keys < Lk with its smallest key, joined
//                                  over the four g lanes of a query at the block's end -> site_peak / site_key; (b) p of rows
//                                  < Lq summed over the wave's queries (registers over QT, then a DPP row reduction over il) and
//                                  added into the wave's OWN row of column sums in LDS.
//                       After the last block the column sums are finished over Lq.  Every addition has a fixed place in a fixed
//                       order: no atomics on data, two calls agree bitwise.  No workspace.  The grid is n_pairs.
//                       site_peak is the maximum of the very values key_mass sums, and site_key the smallest column attaining
//                       it in that arithmetic (distinct scores can round to one p).
//                       The multiplicity is always tested (a profile is over the full key set) and a drug has at most MAX_KEYS
//                       stored keys: DL_FLAG_MAP_COLS otherwise.
#include "pair_keys.cuh"

namespace {
using namespace dltile;
using namespace dlpairs;

// the part of the launch that does not depend on where a pair's keys lie
struct ProfCommon {
  const char *Q, *K;
  float *mass, *peak;
  int32_t* skey;
  const int32_t *qi, *ki;
  uint32_t* flags;
  int64_t q_es, q_rs, k_rs, mass_ps, site_ps;
  int n_q, n_kv, Lq;
  int out_cols;
  float scale;
  float dense_w;                   // DenseKeys: the launch-wide multiplicity (RaggedKeys reads the drug's own)
};
template <typename Keys> struct ProfP : ProfCommon {
  Keys keys;
};

// 256 query rows per block in bf16: ONE block at the model's n_site
// LDS: two K tiles + the column sums = 50 KB in bf16, 82 KB in fp32 (the parity dtype)
template <typename T, int HD, int QT, typename Keys>
__global__ __launch_bounds__(PAIR1_THREADS) void pgca_pairs_profile_kernel(const ProfP<Keys> p) {
  using TL = ATile<T, HD>;
  constexpr int NKF = HD / Mma<T>::KF;
  constexpr int QB = PAIR1_WAVES * QT * 16;
  constexpr int BUF = KVB * TL::RB;
  __shared__ __attribute__((aligned(16))) char smem[2 * BUF];
  __shared__ __attribute__((aligned(16))) float colsum[PAIR1_WAVES * MAX_KEYS];     // [wave][stored key]

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, il = lane & 15, g = lane >> 4;
  const int n = blockIdx.x;
  const int pi = p.qi[n], di = p.ki[n];
  KeySeg ks = {};
  int copies, cols;
  float tail_bias;
  const uint32_t bad = map_guard(p, pi, di, true, MAX_KEYS, ks, copies, cols, tail_bias);
  if (bad) {
    flag_pair(p.flags, bad, threadIdx.x == 0);
    return;
  }
  const int Lk = ks.Lk, tail_start = ks.tail_start, tail_rows = Lk - tail_start;
  const T* Qb = reinterpret_cast<const T*>(p.Q) + (int64_t)pi * p.q_es;
  const T* Kb = reinterpret_cast<const T*>(p.K) + ks.k_off;
  float* peak = p.peak + (int64_t)n * p.site_ps;
  int32_t* skey = p.skey + (int64_t)n * p.site_ps;

  const float c = p.scale * LOG2E;
  const int nt = (Lk + KVB - 1) / KVB;                  // <= MAX_TILES
  const int nqb = (p.Lq + QB - 1) / QB;
  auto stage = [&](int t, int buf) {                    // tile t into buffer buf
    dma_rows<T, HD, PAIR1_THREADS>(smem + buf * BUF, Kb + (int64_t)t * KVB * p.k_rs, p.k_rs, Lk - t * KVB, KVB);
  };
  stage(0, 0);

  float* cw = colsum_begin(colsum, wave, lane, nt);

  int step = 0;                                         // pipeline step over all blocks: tile step % nt of sweep (step / nt) & 1
  for (int qb = 0; qb < nqb; ++qb) {
    const int qw0 = qb * QB + wave * QT * 16;
    u32x4 qf[QT][NKF];
    bool valid[QT];                                     // this lane's query row of tile qt exists
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {                   // (load_q_frags() with valid[] kept: the loop stays here)
      const int q = qw0 + qt * 16 + il;
      valid[qt] = q < p.Lq;
#pragma unroll
      for (int kf = 0; kf < NKF; ++kf) qf[qt][kf] = frag_global<T>(Qb + (int64_t)q * p.q_rs, valid[qt], kf, g);
    }
    float m_run[QT], l_run[QT], lse2[QT], best_p[QT];
    int best_k[QT];
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) { m_run[qt] = -INFINITY; l_run[qt] = 0.f; lse2[qt] = 0.f; best_p[qt] = -1.f; best_k[qt] = 0; }

    for (int j = 0; j < 2 * nt; ++j, ++step) {
      const bool second = j >= nt;                      // (the same for the whole workgroup)
      const int k0 = (second ? j - nt : j) * KVB;
      vm_wait<0>();                                     // this wave's share of this step's LDS-DMA (not implied by the barrier)
      __syncthreads();                                  // the tile has landed; everyone is done with the other buffer
      if (j + 1 < 2 * nt || qb + 1 < nqb) stage(next_tile(j, nt), (step + 1) & 1);
      if (j == nt) {                                    // between the sweeps
#pragma unroll
        for (int qt = 0; qt < QT; ++qt) lse2_join(m_run[qt], l_run[qt], p.scale, lse2[qt]);
      }
      f32x4 s[QT][NKT];
      fwd_scores<T, HD>(smem + (step & 1) * BUF, qf, s, il, g);      // S^T = K Q^T
      if (!second) {
        // ---- sweep 1: key multiplicities, key masking, running maximum and sum ----
        mask_keys(s, k0, Lk, tail_start, tail_bias, g);
        sweep_stats(s, m_run, l_run, c);
      } else {
        // ---- sweep 2: one copy's probability of every key; its maximum per query, its sum over the queries ----
#pragma unroll
        for (int kt = 0; kt < NKT; ++kt) {
          f32x4 cs;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int key = k0 + kt * 16 + 4 * g + r;
            float v = 0.f;
#pragma unroll
            for (int qt = 0; qt < QT; ++qt) {
              const float pv = fast_exp2(s[qt][kt][r] * c - lse2[qt]);
              // keys ascend per lane: > keeps the smallest.  A NaN probability wins and then stays (nothing compares above it): the
              // maximum of a row that holds a NaN is NaN, as torch.max gives, where the bare compare left the initial -1 in place
              if (key < Lk && (pv > best_p[qt] || pv != pv)) { best_p[qt] = pv; best_k[qt] = key; }
              v += valid[qt] ? pv : 0.f;
            }
            cs[r] = row16_sum(v);                       // over the 16 queries il of the row (every lane gets the sum)
          }
          colsum_add(cw, k0, kt, il, g, cs);
        }
      }
      // (no barrier here: the one at the top of the next step is what separates this tile's reads from the DMA that refills
      //  its buffer two steps later; a wave's column sums are its own)
    }
    // the block's site outputs: join the four g lanes of a query (larger p; on equal p the smaller key)
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
      float bp = best_p[qt];
      int bk = best_k[qt];
#pragma unroll
      for (int off = 16; off <= 32; off <<= 1) {
        const float op = __shfl_xor(bp, off, 64);
        const int ok = __shfl_xor(bk, off, 64);
        if (op > bp || op != op || (op == bp && ok < bk)) { bp = op; bk = ok; }
      }
      const int q = qw0 + qt * 16 + il;
      if (g == 0 && valid[qt]) { peak[q] = bp; skey[q] = bk; }
    }
  }

  // key_mass: the mean of the map's columns over the query rows
  colsum_finish<true>(colsum, p.mass + (int64_t)n * p.mass_ps, p.out_cols, cols, tail_start, tail_rows, (float)p.Lq);
}

template <typename Keys>
void launch_profile(int dtype, const ProfP<Keys>& p, int n_pairs, hipStream_t s) {
  launch_by_dtype(dtype, pgca_pairs_profile_kernel<bf16_t, 128, pair_qt<bf16_t>(), Keys>, pgca_pairs_profile_kernel<float, 128, pair_qt<float>(), Keys>,
                  (uint32_t)n_pairs, PAIR1_THREADS, s, p);
}

// What dl_pgca_pairs_profile_args and dl_pgca_pairs_ragged_profile_args share (same field names): the checks, and the common
// block of the launch.  st / stn: the entry point's operand strides and their names.
template <typename Args>
int profile_common(const char* who, const Args* a, const int64_t* st, const char* const* stn, int n_st, ProfCommon& p) {
  DL_TRY(pair_head_checks(who, a));
  DL_CHECK_ARG(a->out_cols > 0, DL_ERR_SHAPE, "%s: out_cols %d must be positive", who, a->out_cols);
  DL_CHECK_ARG(a->reserved == 0, DL_ERR_ARG, "%s: reserved %d must be 0", who, a->reserved);
  if (a->n_pairs == 0) return DL_OK;
  DL_CHECK_ARG(a->Q && a->K && a->key_mass && a->site_peak && a->site_key && a->q_index && a->kv_index, DL_ERR_ARG,
               "%s: null pointer (Q, K, key_mass, site_peak, site_key, q_index, kv_index)", who);
  DL_TRY(pair_stride_checks(who, a->dtype, st, stn, n_st));
  DL_CHECK_ARG((((uintptr_t)a->Q | (uintptr_t)a->K) & 15) == 0, DL_ERR_ALIGN, "%s: Q / K not 16-byte aligned", who);
  DL_CHECK_ARG((((uintptr_t)a->key_mass | (uintptr_t)a->site_peak | (uintptr_t)a->site_key) & 3) == 0, DL_ERR_ALIGN,
               "%s: key_mass / site_peak / site_key not 4-byte aligned", who);
  DL_TRY(pair_index_checks(who, a));
  DL_CHECK_ARG(a->mass_ps >= (int64_t)a->out_cols, DL_ERR_SHAPE, "%s: mass_ps %ld below out_cols = %d", who, (long)a->mass_ps, a->out_cols);
  DL_CHECK_ARG(a->site_ps >= (int64_t)a->Lq, DL_ERR_SHAPE, "%s: site_ps %ld below Lq = %d", who, (long)a->site_ps, a->Lq);
  fill_pair_head(a, p);
  p.mass = a->key_mass; p.peak = a->site_peak; p.skey = a->site_key;
  p.mass_ps = a->mass_ps; p.site_ps = a->site_ps;
  p.out_cols = a->out_cols;
  p.dense_w = 1.f;
  return DL_OK;
}

}  // namespace

extern "C" int dl_pgca_pairs_profile(const dl_pgca_pairs_profile_args* a, dl_stream stream) {
  const char* who = "dl_pgca_pairs_profile";
  DL_TRY(dense_head_checks(who, a, "a profile"));
  const int64_t st[] = {a->q_es, a->q_rs, a->k_es, a->k_rs};
  const char* stn[] = {"q_es", "q_rs", "k_es", "k_rs"};
  ProfP<DenseKeys> p = {};
  DL_TRY(profile_common(who, a, st, stn, 4, p));
  DL_TRY(dense_cols_check(who, a, a->key_tail_rows > 0, "a profile needs", "map"));
  if (a->n_pairs == 0) return DL_OK;
  p.dense_w = fill_dense_keys(a, 0, false, p.keys);
  launch_profile(a->dtype, p, a->n_pairs, (hipStream_t)stream);
  DL_CHECK_LAUNCH("dl_pgca_pairs_profile");
  return DL_OK;
}

extern "C" int dl_pgca_pairs_ragged_profile(const dl_pgca_pairs_ragged_profile_args* a, dl_stream stream) {
  const char* who = "dl_pgca_pairs_ragged_profile";
  DL_TRY(ragged_head_checks(who, a, "a profile"));
  const int64_t st[] = {a->q_es, a->q_rs, a->k_rs};
  const char* stn[] = {"q_es", "q_rs", "k_rs"};
  ProfP<RaggedKeys> p = {};
  const int rc = profile_common(who, a, st, stn, 3, p);
  if (rc != DL_OK || a->n_pairs == 0) return rc;
  DL_TRY(fill_ragged_keys(who, a, p.keys));
  launch_profile(a->dtype, p, a->n_pairs, (hipStream_t)stream);
  DL_CHECK_LAUNCH("dl_pgca_pairs_ragged_profile");
  return DL_OK;
}
