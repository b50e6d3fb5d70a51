// pgca_pairs_attr.hip — hit attributions of the screening path: gradient x code of a target logit at the pair stage, per drug
// key and per protein site, computed WITHOUT forming dQ, dK or dV'.  For pair n = (protein pi, drug di), with q_r the protein's
// projected queries, K_c | V'_c the drug's stored rows, w_c the multiplicity of stored key c (1 in front of the tail, the drug's
// tail weight on its last key_tail_rows rows) and dO_r the gradient of the target w.r.t. the guided half of the pair's concat row:
//     s[r,c]  = scale <q_r, K_c>
//     p[r,c]  = exp(s[r,c]) / sum_c' w_c' exp(s[r,c'])        one copy's probability (the profile kernel's sweep 2)
//     g[r,c]  = <dO_r, V'_c>
//     D[r]    = sum_c w_c p[r,c] g[r,c]
//     ds[r,c] = p[r,c] (g[r,c] - D[r])                        the gradient w.r.t. one copy's logit
//     key_attr [n][col] = sum_r ( ds[r,c] s[r,c] + p[r,c] g[r,c] )      = (<dK_c, K_c> + <dV'_c, V'_c>) / w_c, one copy's value;
//                         expanded to the drug's full columns as key_mass is (copy i of tail key j at lead + i t + j), +0.0f
//                         from the drug's own count up to out_cols
//     site_attr[n][r]   = sum_c w_c ds[r,c] s[r,c]  (+ <d_sites_r, sites_r>)   = <dq_r, q_r> + <dsites_r, sites_r>
// The tail bias log w / scale enters the softmax normaliser only, never the factor s[r,c]; rows r >= Lq and keys c >= Lk
// never enter a sum.  Over dense per-entity codes (dl_pgca_pairs_attr) or the packed per-drug row store
// (dl_pgca_pairs_ragged_attr); see include/druglamp_hip.h for the addressing.
//
//   pgca_pairs_attr_kernel : ONE workgroup of eight waves per pair (the one-workgroup scaffolding of pair_keys.cuh, the guards of
//                       the profile kernel), two sweeps per block of 128 * QT query rows, with a second operand pair: every tile
//                       step stages the K half AND the V' half (columns 128..255 of the same rows) of the tile, and the wave keeps
//                       the fragments of dO next to those of q, so that one step yields S^T = K Q^T and G^T = V' dO^T.
//                         sweep 1  running maximum and sum with the tail bias, and under the same rescale the running
//                                  sum of w e g: between the sweeps the LSE and D[r] (fp32, never from the forward's rounded
//                                  output: g - D cancels) are in registers;
//                         sweep 2  p WITHOUT the tail bias, ds = p (g - D); ds s + p g of rows < Lq summed over the wave's
//                                  queries into the wave's OWN row of column sums in LDS (one copy's value per stored key);
//                                  w ds s of keys < Lk summed per query, the four g lanes joined at the block's end.
//                       No atomics on data, no workspace: two calls agree bitwise.  The grid is n_pairs.
//                       LDS: four tiles + the column sums = 82 KB in bf16, 146 KB in fp32.
#include "pair_keys.cuh"

namespace {
using namespace dltile;
using namespace dlpairs;

struct AttrCommon {
  const char *Q, *K, *dO, *sites, *dsites;
  float *kattr, *sattr;
  const int32_t *qi, *ki;
  uint32_t* flags;
  int64_t q_es, q_rs, k_rs, do_ps, do_rs, left_es, left_rs, dl_ps, dl_rs, mass_ps, site_ps;
  int n_q, n_kv, Lq;
  int out_cols, left_cols;
  float scale;
  float dense_w;                   // DenseKeys: the launch-wide multiplicity (RaggedKeys reads the drug's own)
};
template <typename Keys> struct AttrP : AttrCommon {
  Keys keys;
};

// acc + <a, b> over one 16-byte chunk, in element order
template <typename T> __device__ __forceinline__ float chunk_dot(u32x4 a, u32x4 b, float acc) {
  if constexpr (sizeof(T) == 2) {
    const f32x4 al = __builtin_bit_cast(f32x4, a << 16), bl = __builtin_bit_cast(f32x4, b << 16);
    const f32x4 ah = __builtin_bit_cast(f32x4, a & 0xffff0000u), bh = __builtin_bit_cast(f32x4, b & 0xffff0000u);
    acc = fmaf(al[0], bl[0], acc); acc = fmaf(ah[0], bh[0], acc);
    acc = fmaf(al[1], bl[1], acc); acc = fmaf(ah[1], bh[1], acc);
    acc = fmaf(al[2], bl[2], acc); acc = fmaf(ah[2], bh[2], acc);
    acc = fmaf(al[3], bl[3], acc); acc = fmaf(ah[3], bh[3], acc);
  } else {
    // (whole-vector views, element by element: see the note at Mma<float>::mma in common.cuh)
    const f32x4 af = __builtin_bit_cast(f32x4, a), bf = __builtin_bit_cast(f32x4, b);
    acc = fmaf(af[0], bf[0], acc);
    acc = fmaf(af[1], bf[1], acc);
    acc = fmaf(af[2], bf[2], acc);
    acc = fmaf(af[3], bf[3], acc);
  }
  return acc;
}

template <typename T, int HD, int QT, typename Keys>
__global__ __launch_bounds__(PAIR1_THREADS) void pgca_pairs_attr_kernel(const AttrP<Keys> p) {
  using TL = ATile<T, HD>;
  constexpr int NKF = HD / Mma<T>::KF;
  constexpr int QB = PAIR1_WAVES * QT * 16;
  constexpr int BUF = KVB * TL::RB;                     // one tile image; a buffer is the K tile followed by the V' tile
  __shared__ __attribute__((aligned(16))) char smem[4 * BUF];
  __shared__ __attribute__((aligned(16))) float colsum[PAIR1_WAVES * MAX_KEYS];      // [wave][stored key]

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
  const float wf = (float)copies;
  const T* Qb = reinterpret_cast<const T*>(p.Q) + (int64_t)pi * p.q_es;
  const T* Gb = reinterpret_cast<const T*>(p.dO) + (int64_t)n * p.do_ps;
  const T* Kb = reinterpret_cast<const T*>(p.K) + ks.k_off;
  float* sattr = p.sattr + (int64_t)n * p.site_ps;

  const float c = p.scale * LOG2E;
  const int nt = (Lk + KVB - 1) / KVB;                  // <= MAX_TILES
  const int nqb = (p.Lq + QB - 1) / QB;
  auto stage = [&](int t, int buf) {                    // tile t: K half and V' half of its rows into buffer buf
    const T* rows = Kb + (int64_t)t * KVB * p.k_rs;
    dma_rows<T, HD, PAIR1_THREADS>(smem + (2 * buf) * BUF, rows, p.k_rs, Lk - t * KVB, KVB);
    dma_rows<T, HD, PAIR1_THREADS>(smem + (2 * buf + 1) * BUF, rows + HD, p.k_rs, Lk - t * KVB, KVB);
  };
  stage(0, 0);

  float* cw = colsum_begin(colsum, wave, lane, nt);

  int step = 0;                                         // pipeline step over all blocks: tile step % nt of sweep (step / nt) & 1
  for (int qb = 0; qb < nqb; ++qb) {
    const int qw0 = qb * QB + wave * QT * 16;
    u32x4 qf[QT][NKF], gf[QT][NKF];
    bool valid[QT];                                     // this lane's query row of tile qt exists
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {                   // (load_q_frags() for two operands, valid[] kept)
      const int q = qw0 + qt * 16 + il;
      valid[qt] = q < p.Lq;
#pragma unroll
      for (int kf = 0; kf < NKF; ++kf) {
        qf[qt][kf] = frag_global<T>(Qb + (int64_t)q * p.q_rs, valid[qt], kf, g);
        gf[qt][kf] = frag_global<T>(Gb + (int64_t)q * p.do_rs, valid[qt], kf, g);
      }
    }
    float m_run[QT], l_run[QT], d_run[QT], lse2[QT], dd[QT], site[QT];
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) { m_run[qt] = -INFINITY; l_run[qt] = 0.f; d_run[qt] = 0.f; lse2[qt] = 0.f; dd[qt] = 0.f; site[qt] = 0.f; }

    for (int j = 0; j < 2 * nt; ++j, ++step) {
      const bool second = j >= nt;                      // (the same for the whole workgroup)
      const int k0 = (second ? j - nt : j) * KVB;
      vm_wait<0>();                                     // this wave's share of this step's LDS-DMA (not implied by the barrier)
      __syncthreads();                                  // the tiles have landed; everyone is done with the other buffer
      if (j + 1 < 2 * nt || qb + 1 < nqb) stage(next_tile(j, nt), (step + 1) & 1);
      if (j == nt) {                                    // between the sweeps: LSE_q and D_q from the lanes' partials
#pragma unroll
        for (int qt = 0; qt < QT; ++qt) {
          const float l = lse2_join(m_run[qt], l_run[qt], p.scale, lse2[qt]);
          dd[qt] = group4_sum(d_run[qt]) / l;
        }
      }
      f32x4 s[QT][NKT], gs[QT][NKT];
      const char* buf = smem + (2 * (step & 1)) * BUF;
      fwd_scores<T, HD>(buf, qf, s, il, g);             // S^T = K Q^T
      fwd_scores<T, HD>(buf + BUF, gf, gs, il, g);      // G^T = V' dO^T
      if (!second) {
        // ---- sweep 1: key multiplicities, key masking, running maximum, sum and sum of e g ----
        // (mask_keys() that also takes the masked keys out of the sum of e g)
        if (k0 + KVB > tail_start || k0 + KVB > Lk) {
#pragma unroll
          for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int key = k0 + kt * 16 + 4 * g + r;
#pragma unroll
              for (int qt = 0; qt < QT; ++qt) {
                if (key >= tail_start) s[qt][kt][r] += tail_bias;
                if (key >= Lk) { s[qt][kt][r] = -INFINITY; gs[qt][kt][r] = 0.f; }
              }
            }
        }
        sweep_stats<true>(s, m_run, l_run, c, gs, d_run);
      } else {
        // ---- sweep 2: one copy's p and ds of every key; ds s + p g over the queries, w ds s over the keys ----
#pragma unroll
        for (int kt = 0; kt < NKT; ++kt) {
          f32x4 cs;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int key = k0 + kt * 16 + 4 * g + r;
            const float wk = key >= tail_start ? wf : 1.f;
            float v = 0.f;
#pragma unroll
            for (int qt = 0; qt < QT; ++qt) {
              const float sv = s[qt][kt][r];
              const float gv = gs[qt][kt][r];
              const float pv = fast_exp2(sv * c - lse2[qt]);
              const float ds = pv * (gv - dd[qt]);
              const float t = ds * (sv * p.scale);
              if (key < Lk) site[qt] = fmaf(wk, t, site[qt]);
              v += valid[qt] ? fmaf(pv, gv, t) : 0.f;
            }
            cs[r] = row16_sum(v);                       // over the 16 queries il of the row (every lane gets the sum)
          }
          colsum_add(cw, k0, kt, il, g, cs);
        }
      }
      // (no barrier here: the one at the top of the next step separates this tile's reads from the DMA that refills its
      //  buffer two steps later; a wave's column sums are its own)
    }
    // the block's site output: join the four g lanes of a query; the left half's row dot in fp32
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
      const int q = qw0 + qt * 16 + il;
      float left = 0.f;
      if (p.sites && valid[qt]) {
        const T* sr = reinterpret_cast<const T*>(p.sites) + (int64_t)pi * p.left_es + (int64_t)q * p.left_rs;
        const T* dr = reinterpret_cast<const T*>(p.dsites) + (int64_t)n * p.dl_ps + (int64_t)q * p.dl_rs;
        for (int ch = g; ch * TL::EPC < p.left_cols; ch += 4)
          left = chunk_dot<T>(*reinterpret_cast<const u32x4*>(sr + ch * TL::EPC), *reinterpret_cast<const u32x4*>(dr + ch * TL::EPC), left);
      }
      const float v = group4_sum(site[qt]) + group4_sum(left);
      if (g == 0 && valid[qt]) sattr[q] = v;
    }
  }

  // key_attr: one copy's value at every copy's column
  colsum_finish<false>(colsum, p.kattr + (int64_t)n * p.mass_ps, p.out_cols, cols, tail_start, tail_rows, 1.f);
}

template <typename Keys>
void launch_attr(int dtype, const AttrP<Keys>& p, int n_pairs, hipStream_t s) {
  launch_by_dtype(dtype, pgca_pairs_attr_kernel<bf16_t, 128, pair_qt<bf16_t>(), Keys>, pgca_pairs_attr_kernel<float, 128, pair_qt<float>(), Keys>,
                  (uint32_t)n_pairs, PAIR1_THREADS, s, p);
}

// What dl_pgca_pairs_attr_args and dl_pgca_pairs_ragged_attr_args share (same field names): the checks, and the common block of
// the launch.  st / stn: the entry point's operand strides and their names.
template <typename Args>
int attr_common(const char* who, const Args* a, const int64_t* st, const char* const* stn, int n_st, AttrCommon& p) {
  DL_TRY(pair_head_checks(who, a));
  DL_CHECK_ARG(a->out_cols > 0, DL_ERR_SHAPE, "%s: out_cols %d must be positive", who, a->out_cols);
  DL_CHECK_ARG(a->reserved == 0, DL_ERR_ARG, "%s: reserved %d must be 0", who, a->reserved);
  if (a->n_pairs == 0) return DL_OK;
  DL_CHECK_ARG(a->Q && a->K && a->dO && a->key_attr && a->site_attr && a->q_index && a->kv_index, DL_ERR_ARG,
               "%s: null pointer (Q, K, dO, key_attr, site_attr, q_index, kv_index)", who);
  DL_CHECK_ARG((a->sites == nullptr) == (a->d_sites == nullptr), DL_ERR_ARG, "%s: sites and d_sites are given both or neither", who);
  const int epc = 16 / (int)dl_dtype_size(a->dtype);
  DL_TRY(pair_stride_checks(who, a->dtype, st, stn, n_st));
  DL_CHECK_ARG(a->k_rs >= 2 * (int64_t)a->head_dim, DL_ERR_SHAPE, "%s: k_rs %ld below the %d columns of a [K | V'] row", who,
               (long)a->k_rs, 2 * a->head_dim);
  DL_CHECK_ARG((((uintptr_t)a->Q | (uintptr_t)a->K | (uintptr_t)a->dO | (uintptr_t)a->sites | (uintptr_t)a->d_sites) & 15) == 0, DL_ERR_ALIGN,
               "%s: Q / K / dO / sites / d_sites not 16-byte aligned", who);
  DL_CHECK_ARG((((uintptr_t)a->key_attr | (uintptr_t)a->site_attr) & 3) == 0, DL_ERR_ALIGN, "%s: key_attr / site_attr not 4-byte aligned", who);
  DL_TRY(pair_index_checks(who, a));
  DL_CHECK_ARG(a->mass_ps >= (int64_t)a->out_cols, DL_ERR_SHAPE, "%s: mass_ps %ld below out_cols = %d", who, (long)a->mass_ps, a->out_cols);
  DL_CHECK_ARG(a->site_ps >= (int64_t)a->Lq, DL_ERR_SHAPE, "%s: site_ps %ld below Lq = %d", who, (long)a->site_ps, a->Lq);
  if (a->sites) {
    DL_CHECK_ARG(a->left_cols > 0 && a->left_cols % epc == 0, DL_ERR_SHAPE, "%s: left_cols %d not a positive multiple of %d elements", who,
                 a->left_cols, epc);
    const int64_t ls[] = {a->left_es, a->left_rs, a->dl_ps, a->dl_rs};
    for (int i = 0; i < 4; ++i)
      DL_CHECK_ARG(ls[i] >= 0 && ls[i] % epc == 0, DL_ERR_ALIGN, "%s: a stride of sites / d_sites (%ld) not a non-negative multiple of %d elements",
                   who, (long)ls[i], epc);
  }
  fill_pair_head(a, p);
  p.dO = (const char*)a->dO; p.sites = (const char*)a->sites; p.dsites = (const char*)a->d_sites;
  p.kattr = a->key_attr; p.sattr = a->site_attr;
  p.do_ps = a->do_ps; p.do_rs = a->do_rs;
  p.left_es = a->left_es; p.left_rs = a->left_rs; p.dl_ps = a->dl_ps; p.dl_rs = a->dl_rs;
  p.mass_ps = a->mass_ps; p.site_ps = a->site_ps;
  p.out_cols = a->out_cols; p.left_cols = a->sites ? a->left_cols : 0;
  p.dense_w = 1.f;
  return DL_OK;
}

}  // namespace

extern "C" int dl_pgca_pairs_attr(const dl_pgca_pairs_attr_args* a, dl_stream stream) {
  const char* who = "dl_pgca_pairs_attr";
  DL_TRY(dense_head_checks(who, a, "an attribution"));
  const int64_t st[] = {a->q_es, a->q_rs, a->k_es, a->k_rs, a->do_ps, a->do_rs};
  const char* stn[] = {"q_es", "q_rs", "k_es", "k_rs", "do_ps", "do_rs"};
  AttrP<DenseKeys> p = {};
  DL_TRY(attr_common(who, a, st, stn, 6, p));
  DL_TRY(dense_cols_check(who, a, a->key_tail_rows > 0, "attributions need", "drug"));
  if (a->n_pairs == 0) return DL_OK;
  p.dense_w = fill_dense_keys(a, 0, false, p.keys);
  launch_attr(a->dtype, p, a->n_pairs, (hipStream_t)stream);
  DL_CHECK_LAUNCH("dl_pgca_pairs_attr");
  return DL_OK;
}

extern "C" int dl_pgca_pairs_ragged_attr(const dl_pgca_pairs_ragged_attr_args* a, dl_stream stream) {
  const char* who = "dl_pgca_pairs_ragged_attr";
  DL_TRY(ragged_head_checks(who, a, "an attribution"));
  const int64_t st[] = {a->q_es, a->q_rs, a->k_rs, a->do_ps, a->do_rs};
  const char* stn[] = {"q_es", "q_rs", "k_rs", "do_ps", "do_rs"};
  AttrP<RaggedKeys> p = {};
  const int rc = attr_common(who, a, st, stn, 5, p);
  if (rc != DL_OK || a->n_pairs == 0) return rc;
  DL_TRY(fill_ragged_keys(who, a, p.keys));
  launch_attr(a->dtype, p, a->n_pairs, (hipStream_t)stream);
  DL_CHECK_LAUNCH("dl_pgca_pairs_ragged_attr");
  return DL_OK;
}
