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
//   pgca_pairs_attr_kernel : the skeleton of pgca_pairs_profile_kernel — ONE workgroup of eight waves per pair, one locate(),
//                       64-key tiles by LDS-DMA through two buffers, the transposed score layout (lane (il, g): keys 4g + r of
//                       query il), two sweeps per block of 128 * QT query rows — with a second operand pair: every tile step
//                       stages the K half AND the V' half (columns 128..255 of the same rows) of the tile, and the wave keeps
//                       the fragments of dO next to those of q, so that one step yields S^T = K Q^T and G^T = V' dO^T.
//                         sweep 1  running maximum and sum with the tail bias, and under the same rescale the running
//                                  sum of w e g: between the sweeps the LSE and D[r] (fp32, never from the forward's rounded
//                                  output: g - D cancels) are in registers;
//                         sweep 2  p WITHOUT the tail bias, ds = p (g - D); ds s + p g of rows < Lq summed over the wave's
//                                  queries into the wave's OWN row of column sums in LDS (one copy's value per stored key);
//                                  w ds s of keys < Lk summed per query, the four g lanes joined at the block's end.
//                       After the last block the eight waves' column sums are added in a fixed order and written with the tail
//                       keys' sums replicated to their copies' columns.  No atomics on data, no workspace: two calls agree
//                       bitwise.  The grid is n_pairs.  Guards and flags are the profile kernel's.
//                       LDS: four tiles + the column sums = 82 KB in bf16, 146 KB in fp32.
#include "pair_keys.cuh"
#include "tiles.cuh"

namespace {
using namespace dltile;
using namespace dlpairs;

constexpr int KVB = 64, NKT = KVB / 16;   // keys per streamed tile, 16-key score tiles in it
constexpr int MAX_TILES = 9;              // 576 stored keys, as the profile kernel
constexpr int MAX_KEYS = MAX_TILES * KVB;
constexpr int ATTR_WAVES = 8, ATTR_THREADS = ATTR_WAVES * 64;

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

__device__ __forceinline__ float tail_weight(const DenseKeys&, int, float dense_w) { return dense_w; }
__device__ __forceinline__ float tail_weight(const RaggedKeys& k, int di, float) { return k.tailw[di]; }

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
__global__ __launch_bounds__(ATTR_THREADS) void pgca_pairs_attr_kernel(const AttrP<Keys> p) {
  using TL = ATile<T, HD>;
  constexpr int NKF = HD / Mma<T>::KF;
  constexpr int QB = ATTR_WAVES * QT * 16;
  constexpr int BUF = KVB * TL::RB;                     // one tile image; a buffer is the K tile followed by the V' tile
  __shared__ __attribute__((aligned(16))) char smem[4 * BUF];
  __shared__ __attribute__((aligned(16))) float colsum[ATTR_WAVES * MAX_KEYS];      // [wave][stored key]

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, il = lane & 15, g = lane >> 4;
  const int n = blockIdx.x;
  const int pi = p.qi[n], di = p.ki[n];
  // All guards are uniform for the workgroup (pgca_pairs_profile_kernel's), all of them in front of the one atomic.
  KeySeg ks = {};
  const bool in_range = (unsigned)pi < (unsigned)p.n_q && (unsigned)di < (unsigned)p.n_kv;
  uint32_t bad = in_range ? p.keys.locate(di, p.k_rs, 0, p.scale, ks) : (uint32_t)DL_FLAG_PAIR_INDEX;
  int copies = 1;
  float tail_bias = 0.f;
  int64_t cols64 = ks.Lk;
  if (!bad && ks.Lk > ks.tail_start) {
    const float w = tail_weight(p.keys, di, p.dense_w);
    if (w <= 16777216.f && w == truncf(w)) {
      copies = (int)w;
      cols64 = (int64_t)ks.tail_start + (int64_t)(ks.Lk - ks.tail_start) * copies;
      tail_bias = logf(w) / p.scale;
    } else {
      bad = DL_FLAG_MAP_COLS;
    }
  }
  if (!bad && (cols64 > (int64_t)p.out_cols || ks.Lk > MAX_KEYS)) bad = DL_FLAG_MAP_COLS;
  if (bad) {                                            // the pair is skipped: nothing read through the entry, nothing written
    if (p.flags && threadIdx.x == 0) atomicOr(p.flags, bad);
    return;
  }
  const int Lk = ks.Lk, tail_start = ks.tail_start, tail_rows = Lk - tail_start, cols = (int)cols64;
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
    dma_rows<T, HD, ATTR_THREADS>(smem + (2 * buf) * BUF, rows, p.k_rs, Lk - t * KVB, KVB);
    dma_rows<T, HD, ATTR_THREADS>(smem + (2 * buf + 1) * BUF, rows + HD, p.k_rs, Lk - t * KVB, KVB);
  };
  stage(0, 0);

  float* cw = colsum + wave * MAX_KEYS;                 // this wave's column sums (only this wave touches them until the end)
  for (int k = lane; k < nt * KVB; k += 64) cw[k] = 0.f;

  int step = 0;                                         // pipeline step over all blocks: tile step % nt of sweep (step / nt) & 1
  for (int qb = 0; qb < nqb; ++qb) {
    const int qw0 = qb * QB + wave * QT * 16;
    u32x4 qf[QT][NKF], gf[QT][NKF];
    bool valid[QT];                                     // this lane's query row of tile qt exists
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
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
      if (j + 1 < 2 * nt || qb + 1 < nqb) {
        const int jn = j + 1;
        stage(jn >= 2 * nt ? 0 : (jn >= nt ? jn - nt : jn), (step + 1) & 1);
      }
      if (j == nt) {                                    // between the sweeps: LSE_q and D_q from the lanes' partials
#pragma unroll
        for (int qt = 0; qt < QT; ++qt) {
          const float l = group4_sum(l_run[qt]);
          lse2[qt] = (m_run[qt] * p.scale + logf(l)) * LOG2E;
          dd[qt] = group4_sum(d_run[qt]) / l;
        }
      }
      f32x4 s[QT][NKT], gs[QT][NKT];
      const char* buf = smem + (2 * (step & 1)) * BUF;
      fwd_scores<T, HD>(buf, qf, s, il, g);             // S^T = K Q^T
      fwd_scores<T, HD>(buf + BUF, gf, gs, il, g);      // G^T = V' dO^T
      if (!second) {
        // ---- sweep 1: key multiplicities, key masking, running maximum, sum and sum of e g ----
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
#pragma unroll
        for (int qt = 0; qt < QT; ++qt) {
          float mx = -INFINITY;
#pragma unroll
          for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r) mx = fmaxf(mx, s[qt][kt][r]);
          mx = group4_max(mx);
          const float m_new = fmaxf(m_run[qt], mx);
          const float alpha = fast_exp2((m_run[qt] - m_new) * c);
          const float mc = m_new * c;
          float rs = 0.f, rd = 0.f;
#pragma unroll
          for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const float e = fast_exp2(s[qt][kt][r] * c - mc);   // w exp(..) on a tail key: the bias is inside
              rs += e;
              rd = fmaf(e, gs[qt][kt][r], rd);
            }
          l_run[qt] = l_run[qt] * alpha + rs;           // per-lane partials (own keys); reduced between the sweeps
          d_run[qt] = d_run[qt] * alpha + rd;
          m_run[qt] = m_new;
        }
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
          if (il == 0) {                                // keys >= Lk collect sums too; they are never read
            f32x4* a = reinterpret_cast<f32x4*>(cw + k0 + kt * 16 + 4 * g);
            *a = *a + cs;
          }
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

  // key_attr: the waves' column sums in a fixed order; tail key j's sum goes to every copy's column lead + i t + j
  __syncthreads();
  float* kattr = p.kattr + (int64_t)n * p.mass_ps;
  for (int col = threadIdx.x; col < p.out_cols; col += ATTR_THREADS) {
    float v = 0.f;
    if (col < cols) {
      const int key = col < tail_start ? col : tail_start + (col - tail_start) % tail_rows;
      const float* cs = colsum + key;
      static_assert(ATTR_WAVES == 8, "the fixed order below adds eight waves");
      v = ((cs[0] + cs[MAX_KEYS]) + (cs[2 * MAX_KEYS] + cs[3 * MAX_KEYS])) +
          ((cs[4 * MAX_KEYS] + cs[5 * MAX_KEYS]) + (cs[6 * MAX_KEYS] + cs[7 * MAX_KEYS]));
    }
    kattr[col] = v;
  }
}

template <typename T> constexpr int attr_qt() { return sizeof(T) == 2 ? 2 : 1; }

template <typename Keys>
void launch_attr(int dtype, const AttrP<Keys>& p, int n_pairs, hipStream_t s) {
  const dim3 grid((uint32_t)n_pairs);
  if (dtype == DL_BF16) hipLaunchKernelGGL((pgca_pairs_attr_kernel<bf16_t, 128, attr_qt<bf16_t>(), Keys>), grid, dim3(ATTR_THREADS), 0, s, p);
  else hipLaunchKernelGGL((pgca_pairs_attr_kernel<float, 128, attr_qt<float>(), Keys>), grid, dim3(ATTR_THREADS), 0, s, p);
}

// What dl_pgca_pairs_attr_args and dl_pgca_pairs_ragged_attr_args share (same field names): the checks, and the common block of
// the launch.  st / stn: the entry point's operand strides and their names.  Nothing behind a pointer is looked at, and with
// n_pairs == 0 (no launch) no pointer or stride either.
template <typename Args>
int attr_common(const char* who, const Args* a, const int64_t* st, const char* const* stn, int n_st, AttrCommon& p) {
  DL_CHECK_ARG(a->dtype == DL_F32 || a->dtype == DL_BF16, DL_ERR_ARG, "%s: bad dtype %d", who, a->dtype);
  DL_CHECK_ARG(a->head_dim == 128, DL_ERR_UNSUPPORTED, "%s: head_dim %d (one head of 128 only)", who, a->head_dim);
  DL_CHECK_ARG(a->n_pairs >= 0 && a->n_q >= 0 && a->n_kv >= 0, DL_ERR_SHAPE, "%s: negative count (n_pairs %d, n_q %d, n_kv %d)", who,
               a->n_pairs, a->n_q, a->n_kv);
  DL_CHECK_ARG(a->Lq > 0, DL_ERR_SHAPE, "%s: Lq %d must be positive", who, a->Lq);
  DL_CHECK_ARG(a->scale > 0.f, DL_ERR_ARG, "%s: scale must be positive", who);
  DL_CHECK_ARG(a->out_cols > 0, DL_ERR_SHAPE, "%s: out_cols %d must be positive", who, a->out_cols);
  DL_CHECK_ARG(a->reserved == 0, DL_ERR_ARG, "%s: reserved %d must be 0", who, a->reserved);
  if (a->n_pairs == 0) return DL_OK;
  DL_CHECK_ARG(a->Q && a->K && a->dO && a->key_attr && a->site_attr && a->q_index && a->kv_index, DL_ERR_ARG,
               "%s: null pointer (Q, K, dO, key_attr, site_attr, q_index, kv_index)", who);
  DL_CHECK_ARG((a->sites == nullptr) == (a->d_sites == nullptr), DL_ERR_ARG, "%s: sites and d_sites are given both or neither", who);
  const int epc = 16 / (int)dl_dtype_size(a->dtype);
  for (int i = 0; i < n_st; ++i)
    DL_CHECK_ARG(st[i] >= 0 && st[i] % epc == 0, DL_ERR_ALIGN, "%s: stride %s (%ld) not a non-negative multiple of %d elements", who,
                 stn[i], (long)st[i], epc);
  DL_CHECK_ARG(a->k_rs >= 2 * (int64_t)a->head_dim, DL_ERR_SHAPE, "%s: k_rs %ld below the %d columns of a [K | V'] row", who,
               (long)a->k_rs, 2 * a->head_dim);
  DL_CHECK_ARG((((uintptr_t)a->Q | (uintptr_t)a->K | (uintptr_t)a->dO | (uintptr_t)a->sites | (uintptr_t)a->d_sites) & 15) == 0, DL_ERR_ALIGN,
               "%s: Q / K / dO / sites / d_sites not 16-byte aligned", who);
  DL_CHECK_ARG((((uintptr_t)a->key_attr | (uintptr_t)a->site_attr) & 3) == 0, DL_ERR_ALIGN, "%s: key_attr / site_attr not 4-byte aligned", who);
  DL_CHECK_ARG((((uintptr_t)a->q_index | (uintptr_t)a->kv_index | (uintptr_t)a->flags) & 3) == 0, DL_ERR_ALIGN,
               "%s: q_index / kv_index / flags not 4-byte aligned", who);
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
  p.Q = (const char*)a->Q; p.K = (const char*)a->K; p.dO = (const char*)a->dO;
  p.sites = (const char*)a->sites; p.dsites = (const char*)a->d_sites;
  p.kattr = a->key_attr; p.sattr = a->site_attr;
  p.qi = a->q_index; p.ki = a->kv_index; p.flags = a->flags;
  p.q_es = a->q_es; p.q_rs = a->q_rs; p.k_rs = a->k_rs; p.do_ps = a->do_ps; p.do_rs = a->do_rs;
  p.left_es = a->left_es; p.left_rs = a->left_rs; p.dl_ps = a->dl_ps; p.dl_rs = a->dl_rs;
  p.mass_ps = a->mass_ps; p.site_ps = a->site_ps;
  p.n_q = a->n_q; p.n_kv = a->n_kv; p.Lq = a->Lq;
  p.out_cols = a->out_cols; p.left_cols = a->sites ? a->left_cols : 0;
  p.scale = a->scale;
  p.dense_w = 1.f;
  return DL_OK;
}

}  // namespace

extern "C" int dl_pgca_pairs_attr(const dl_pgca_pairs_attr_args* a, dl_stream stream) {
  const char* who = "dl_pgca_pairs_attr";
  DL_CHECK_ARG(a, DL_ERR_ARG, "%s: null argument block", who);
  DL_CHECK_ARG(a->Lq > 0 && a->Lk > 0, DL_ERR_SHAPE, "%s: Lq %d, Lk %d must be positive", who, a->Lq, a->Lk);
  DL_CHECK_ARG(a->Lk <= MAX_KEYS, DL_ERR_UNSUPPORTED, "%s: Lk %d above the %d stored keys an attribution launch serves", who, a->Lk, MAX_KEYS);
  DL_CHECK_ARG(a->key_tail_rows >= 0 && a->key_tail_rows <= a->Lk, DL_ERR_ARG, "%s: key_tail_rows %d not in [0, Lk = %d]", who,
               a->key_tail_rows, a->Lk);
  DL_CHECK_ARG(a->key_tail_rows == 0 || a->key_tail_weight >= 1.f, DL_ERR_ARG, "%s: key_tail_weight %g below 1", who,
               (double)a->key_tail_weight);
  const int64_t st[] = {a->q_es, a->q_rs, a->k_es, a->k_rs, a->do_ps, a->do_rs};
  const char* stn[] = {"q_es", "q_rs", "k_es", "k_rs", "do_ps", "do_rs"};
  AttrP<DenseKeys> p = {};
  const int rc = attr_common(who, a, st, stn, 6, p);
  if (rc != DL_OK) return rc;
  // the column count is launch-wide here: checked on the host (the kernel's DL_FLAG_MAP_COLS guard then never trips)
  const bool tail = a->key_tail_rows > 0;
  DL_CHECK_ARG(!tail || (a->key_tail_weight <= 16777216.f && a->key_tail_weight == (float)(int64_t)a->key_tail_weight), DL_ERR_ARG,
               "%s: attributions need a whole key_tail_weight (got %g)", who, (double)a->key_tail_weight);
  const int64_t cols = tail ? (int64_t)(a->Lk - a->key_tail_rows) + (int64_t)a->key_tail_rows * (int64_t)a->key_tail_weight : (int64_t)a->Lk;
  DL_CHECK_ARG(cols <= (int64_t)a->out_cols, DL_ERR_SHAPE, "%s: a drug of %ld columns does not fit out_cols = %d", who, (long)cols, a->out_cols);
  if (a->n_pairs == 0) return DL_OK;
  p.keys.k_es = a->k_es; p.keys.v_es = 0;
  p.keys.Lk = a->Lk;
  p.keys.tail_start = a->Lk - a->key_tail_rows;
  p.keys.tail_bias = 0.f;                               // (not read: the kernel takes log(dense_w) / scale itself)
  p.dense_w = tail ? a->key_tail_weight : 1.f;
  launch_attr(a->dtype, p, a->n_pairs, (hipStream_t)stream);
  DL_CHECK_LAUNCH("dl_pgca_pairs_attr");
  return DL_OK;
}

extern "C" int dl_pgca_pairs_ragged_attr(const dl_pgca_pairs_ragged_attr_args* a, dl_stream stream) {
  const char* who = "dl_pgca_pairs_ragged_attr";
  DL_CHECK_ARG(a, DL_ERR_ARG, "%s: null argument block", who);
  DL_CHECK_ARG(a->kv_total_rows >= 0, DL_ERR_SHAPE, "%s: kv_total_rows %ld is negative", who, (long)a->kv_total_rows);
  DL_CHECK_ARG(a->key_tail_rows >= 0, DL_ERR_ARG, "%s: key_tail_rows %d is negative", who, a->key_tail_rows);
  DL_CHECK_ARG(a->key_tail_rows <= MAX_KEYS, DL_ERR_UNSUPPORTED, "%s: key_tail_rows %d above the %d stored keys an attribution launch serves", who,
               a->key_tail_rows, MAX_KEYS);
  const int64_t st[] = {a->q_es, a->q_rs, a->k_rs, a->do_ps, a->do_rs};
  const char* stn[] = {"q_es", "q_rs", "k_rs", "do_ps", "do_rs"};
  AttrP<RaggedKeys> p = {};
  const int rc = attr_common(who, a, st, stn, 5, p);
  if (rc != DL_OK || a->n_pairs == 0) return rc;
  DL_CHECK_ARG(a->kv_row0 && a->kv_keys && a->kv_tail_weight, DL_ERR_ARG, "%s: null pointer (kv_row0, kv_keys, kv_tail_weight)", who);
  DL_CHECK_ARG(((uintptr_t)a->kv_row0 & 7) == 0, DL_ERR_ALIGN, "%s: kv_row0 not 8-byte aligned", who);
  DL_CHECK_ARG((((uintptr_t)a->kv_keys | (uintptr_t)a->kv_tail_weight) & 3) == 0, DL_ERR_ALIGN,
               "%s: kv_keys / kv_tail_weight not 4-byte aligned", who);
  p.keys.row0 = a->kv_row0; p.keys.keys = a->kv_keys; p.keys.tailw = a->kv_tail_weight;
  p.keys.total_rows = a->kv_total_rows;
  p.keys.tail_rows = a->key_tail_rows;
  launch_attr(a->dtype, p, a->n_pairs, (hipStream_t)stream);
  DL_CHECK_LAUNCH("dl_pgca_pairs_ragged_attr");
  return DL_OK;
}
