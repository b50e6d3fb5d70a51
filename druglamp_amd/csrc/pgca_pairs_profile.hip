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
//   The operands and the way a workgroup finds its keys are those of pgca_pairs_probs.hip (the `Keys` types of pair_keys.cuh,
//   one locate()), and so are the tile loader, the score step and sweep 1.
//
//   pgca_pairs_profile_kernel : ONE workgroup of eight waves per pair; it loops over the pair's blocks of 128 * QT query rows (a wave
//                       owns 16 * QT of a block) and sweeps the drug's 64-key tiles twice per block through two LDS buffers by LDS-DMA (one
//                       pipeline over all blocks; from the second pass on the tiles come from L2):
//                         sweep 1  scores in the transposed layout (lane (il, g): keys 4g + r of query il), running maximum and
//                                  sum with the tail bias; the LSE stays in registers;
//                         sweep 2  the scores again, p = exp2(s c - lse2) WITHOUT the tail bias (one copy's probability), and
//                                  instead of a store: (a) per lane the largest p over keys < Lk with its smallest key, joined
//                                  over the four g lanes of a query at the block's end -> site_peak / site_key; (b) p of rows
//                                  < Lq summed over the wave's queries (registers over QT, then a DPP row reduction over il) and
//                                  added into the wave's OWN row of column sums in LDS.
//                       After the last block the eight waves' column sums are added in a fixed order, divided by Lq and written
//                       with the tail keys' sums replicated to their copies' columns.  Every addition has a fixed place in a
//                       fixed order: no atomics on data, two calls agree bitwise.  No workspace.  The grid is n_pairs.
//                       site_peak is the maximum of the very values key_mass sums, and site_key the smallest column attaining
//                       it in that arithmetic (distinct scores can round to one p).
//                       A pair whose index is out of range (DL_FLAG_PAIR_INDEX), whose drug's table entry does not describe
//                       rows inside the store (DL_FLAG_KEY_TABLE), or whose profile cannot be served (more columns than out_cols,
//                       a multiplicity that is no whole number <= 2^24, more than MAX_KEYS stored keys:
//                       DL_FLAG_MAP_COLS) returns before it reads anything through the entry or writes anything; all tests are
//                       uniform for the workgroup.
#include "pair_keys.cuh"
#include "tiles.cuh"

namespace {
using namespace dltile;
using namespace dlpairs;

constexpr int KVB = 64, NKT = KVB / 16;   // keys per streamed tile, 16-key score tiles in it
constexpr int MAX_TILES = 9;              // 576 stored keys: the library's drugs have at most 520
constexpr int MAX_KEYS = MAX_TILES * KVB;
constexpr int PROF_WAVES = 8, PROF_THREADS = PROF_WAVES * 64;   // 256 query rows per block in bf16: ONE block at the model's n_site

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

// the multiplicity of drug di's tail keys (only read for an entry that locate() accepted)
__device__ __forceinline__ float tail_weight(const DenseKeys&, int, float dense_w) { return dense_w; }
__device__ __forceinline__ float tail_weight(const RaggedKeys& k, int di, float) { return k.tailw[di]; }

// LDS: two K tiles + the column sums = 50 KB in bf16, 82 KB in fp32 (the parity dtype)
template <typename T, int HD, int QT, typename Keys>
__global__ __launch_bounds__(PROF_THREADS) void pgca_pairs_profile_kernel(const ProfP<Keys> p) {
  using TL = ATile<T, HD>;
  constexpr int NKF = HD / Mma<T>::KF;
  constexpr int QB = PROF_WAVES * QT * 16;
  constexpr int BUF = KVB * TL::RB;
  __shared__ __attribute__((aligned(16))) char smem[2 * BUF];
  __shared__ __attribute__((aligned(16))) float colsum[PROF_WAVES * MAX_KEYS];      // [wave][stored key]

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, il = lane & 15, g = lane >> 4;
  const int n = blockIdx.x;
  const int pi = p.qi[n], di = p.ki[n];
  // All guards are uniform for the workgroup: the indices, what locate() reads and the multiplicity are scalar loads (the
  // keys' entry is read only through an index in range), all of them in front of the one atomic.
  KeySeg ks = {};
  const bool in_range = (unsigned)pi < (unsigned)p.n_q && (unsigned)di < (unsigned)p.n_kv;
  uint32_t bad = in_range ? p.keys.locate(di, p.k_rs, 0, p.scale, ks) : (uint32_t)DL_FLAG_PAIR_INDEX;
  int copies = 1;
  float tail_bias = 0.f;
  int64_t cols64 = ks.Lk;                               // columns of this drug's map
  if (!bad && ks.Lk > ks.tail_start) {
    const float w = tail_weight(p.keys, di, p.dense_w);
    if (w <= 16777216.f && w == truncf(w)) {
      copies = (int)w;
      cols64 = (int64_t)ks.tail_start + (int64_t)(ks.Lk - ks.tail_start) * copies;
      tail_bias = logf(w) / p.scale;                    // (on the device for both Keys types: the two entry points agree bitwise)
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
  const T* Qb = reinterpret_cast<const T*>(p.Q) + (int64_t)pi * p.q_es;
  const T* Kb = reinterpret_cast<const T*>(p.K) + ks.k_off;
  float* peak = p.peak + (int64_t)n * p.site_ps;
  int32_t* skey = p.skey + (int64_t)n * p.site_ps;

  const float c = p.scale * LOG2E;
  const int nt = (Lk + KVB - 1) / KVB;                  // <= MAX_TILES
  const int nqb = (p.Lq + QB - 1) / QB;
  auto stage = [&](int t, int buf) {                    // tile t into buffer buf
    dma_rows<T, HD, PROF_THREADS>(smem + buf * BUF, Kb + (int64_t)t * KVB * p.k_rs, p.k_rs, Lk - t * KVB, KVB);
  };
  stage(0, 0);

  float* cw = colsum + wave * MAX_KEYS;                 // this wave's column sums (only this wave touches them until the end)
  for (int k = lane; k < nt * KVB; k += 64) cw[k] = 0.f;

  int step = 0;                                         // pipeline step over all blocks: tile step % nt of sweep (step / nt) & 1
  for (int qb = 0; qb < nqb; ++qb) {
    const int qw0 = qb * QB + wave * QT * 16;
    u32x4 qf[QT][NKF];
    bool valid[QT];                                     // this lane's query row of tile qt exists
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
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
      if (j + 1 < 2 * nt || qb + 1 < nqb) {
        const int jn = j + 1;
        stage(jn >= 2 * nt ? 0 : (jn >= nt ? jn - nt : jn), (step + 1) & 1);
      }
      if (j == nt) {                                    // between the sweeps: LSE_q = m scale + log l, as attn_lse_kernel
#pragma unroll
        for (int qt = 0; qt < QT; ++qt) lse2[qt] = (m_run[qt] * p.scale + logf(group4_sum(l_run[qt]))) * LOG2E;
      }
      f32x4 s[QT][NKT];
      fwd_scores<T, HD>(smem + (step & 1) * BUF, qf, s, il, g);      // S^T = K Q^T
      if (!second) {
        // ---- sweep 1: key multiplicities, key masking, running maximum and sum (pgca_pairs_probs_kernel's) ----
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
          float rs = 0.f;
#pragma unroll
          for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r) rs += fast_exp2(s[qt][kt][r] * c - mc);
          l_run[qt] = l_run[qt] * alpha + rs;           // per-lane partial (own keys); reduced between the sweeps
          m_run[qt] = m_new;
        }
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
          if (il == 0) {                                // keys >= Lk collect sums too; they are never read
            f32x4* a = reinterpret_cast<f32x4*>(cw + k0 + kt * 16 + 4 * g);
            *a = *a + cs;
          }
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

  // key_mass: the waves' column sums in a fixed order, over Lq; tail key j's sum goes to every copy's column lead + i t + j
  __syncthreads();
  float* mass = p.mass + (int64_t)n * p.mass_ps;
  const float lq = (float)p.Lq;
  for (int col = threadIdx.x; col < p.out_cols; col += PROF_THREADS) {
    float v = 0.f;
    if (col < cols) {
      const int key = col < tail_start ? col : tail_start + (col - tail_start) % tail_rows;
      const float* cs = colsum + key;
      static_assert(PROF_WAVES == 8, "the fixed order below adds eight waves");
      v = (((cs[0] + cs[MAX_KEYS]) + (cs[2 * MAX_KEYS] + cs[3 * MAX_KEYS])) +
           ((cs[4 * MAX_KEYS] + cs[5 * MAX_KEYS]) + (cs[6 * MAX_KEYS] + cs[7 * MAX_KEYS]))) / lq;
    }
    mass[col] = v;
  }
}

template <typename T> constexpr int prof_qt() { return sizeof(T) == 2 ? 2 : 1; }

template <typename Keys>
void launch_profile(int dtype, const ProfP<Keys>& p, int n_pairs, hipStream_t s) {
  const dim3 grid((uint32_t)n_pairs);
  if (dtype == DL_BF16) hipLaunchKernelGGL((pgca_pairs_profile_kernel<bf16_t, 128, prof_qt<bf16_t>(), Keys>), grid, dim3(PROF_THREADS), 0, s, p);
  else hipLaunchKernelGGL((pgca_pairs_profile_kernel<float, 128, prof_qt<float>(), Keys>), grid, dim3(PROF_THREADS), 0, s, p);
}

// What dl_pgca_pairs_profile_args and dl_pgca_pairs_ragged_profile_args share (same field names): the checks, and the common
// block of the launch.  st / stn: the entry point's operand strides and their names.  Nothing behind a pointer is looked at, and
// with n_pairs == 0 (no launch) no pointer or stride either.
template <typename Args>
int profile_common(const char* who, const Args* a, const int64_t* st, const char* const* stn, int n_st, ProfCommon& p) {
  DL_CHECK_ARG(a->dtype == DL_F32 || a->dtype == DL_BF16, DL_ERR_ARG, "%s: bad dtype %d", who, a->dtype);
  DL_CHECK_ARG(a->head_dim == 128, DL_ERR_UNSUPPORTED, "%s: head_dim %d (one head of 128 only)", who, a->head_dim);
  DL_CHECK_ARG(a->n_pairs >= 0 && a->n_q >= 0 && a->n_kv >= 0, DL_ERR_SHAPE, "%s: negative count (n_pairs %d, n_q %d, n_kv %d)", who,
               a->n_pairs, a->n_q, a->n_kv);
  DL_CHECK_ARG(a->Lq > 0, DL_ERR_SHAPE, "%s: Lq %d must be positive", who, a->Lq);
  DL_CHECK_ARG(a->scale > 0.f, DL_ERR_ARG, "%s: scale must be positive", who);
  DL_CHECK_ARG(a->out_cols > 0, DL_ERR_SHAPE, "%s: out_cols %d must be positive", who, a->out_cols);
  DL_CHECK_ARG(a->reserved == 0, DL_ERR_ARG, "%s: reserved %d must be 0", who, a->reserved);
  if (a->n_pairs == 0) return DL_OK;
  DL_CHECK_ARG(a->Q && a->K && a->key_mass && a->site_peak && a->site_key && a->q_index && a->kv_index, DL_ERR_ARG,
               "%s: null pointer (Q, K, key_mass, site_peak, site_key, q_index, kv_index)", who);
  const int epc = 16 / (int)dl_dtype_size(a->dtype);
  for (int i = 0; i < n_st; ++i)
    DL_CHECK_ARG(st[i] >= 0 && st[i] % epc == 0, DL_ERR_ALIGN, "%s: stride %s (%ld) not a non-negative multiple of %d elements", who,
                 stn[i], (long)st[i], epc);
  DL_CHECK_ARG((((uintptr_t)a->Q | (uintptr_t)a->K) & 15) == 0, DL_ERR_ALIGN, "%s: Q / K not 16-byte aligned", who);
  DL_CHECK_ARG((((uintptr_t)a->key_mass | (uintptr_t)a->site_peak | (uintptr_t)a->site_key) & 3) == 0, DL_ERR_ALIGN,
               "%s: key_mass / site_peak / site_key not 4-byte aligned", who);
  DL_CHECK_ARG((((uintptr_t)a->q_index | (uintptr_t)a->kv_index | (uintptr_t)a->flags) & 3) == 0, DL_ERR_ALIGN,
               "%s: q_index / kv_index / flags not 4-byte aligned", who);
  DL_CHECK_ARG(a->mass_ps >= (int64_t)a->out_cols, DL_ERR_SHAPE, "%s: mass_ps %ld below out_cols = %d", who, (long)a->mass_ps, a->out_cols);
  DL_CHECK_ARG(a->site_ps >= (int64_t)a->Lq, DL_ERR_SHAPE, "%s: site_ps %ld below Lq = %d", who, (long)a->site_ps, a->Lq);
  p.Q = (const char*)a->Q; p.K = (const char*)a->K;
  p.mass = a->key_mass; p.peak = a->site_peak; p.skey = a->site_key;
  p.qi = a->q_index; p.ki = a->kv_index; p.flags = a->flags;
  p.q_es = a->q_es; p.q_rs = a->q_rs; p.k_rs = a->k_rs; p.mass_ps = a->mass_ps; p.site_ps = a->site_ps;
  p.n_q = a->n_q; p.n_kv = a->n_kv; p.Lq = a->Lq;
  p.out_cols = a->out_cols;
  p.scale = a->scale;
  p.dense_w = 1.f;
  return DL_OK;
}

}  // namespace

extern "C" int dl_pgca_pairs_profile(const dl_pgca_pairs_profile_args* a, dl_stream stream) {
  const char* who = "dl_pgca_pairs_profile";
  DL_CHECK_ARG(a, DL_ERR_ARG, "%s: null argument block", who);
  DL_CHECK_ARG(a->Lq > 0 && a->Lk > 0, DL_ERR_SHAPE, "%s: Lq %d, Lk %d must be positive", who, a->Lq, a->Lk);
  DL_CHECK_ARG(a->Lk <= MAX_KEYS, DL_ERR_UNSUPPORTED, "%s: Lk %d above the %d stored keys a profile launch serves", who, a->Lk, MAX_KEYS);
  DL_CHECK_ARG(a->key_tail_rows >= 0 && a->key_tail_rows <= a->Lk, DL_ERR_ARG, "%s: key_tail_rows %d not in [0, Lk = %d]", who,
               a->key_tail_rows, a->Lk);
  DL_CHECK_ARG(a->key_tail_rows == 0 || a->key_tail_weight >= 1.f, DL_ERR_ARG, "%s: key_tail_weight %g below 1", who,
               (double)a->key_tail_weight);
  const int64_t st[] = {a->q_es, a->q_rs, a->k_es, a->k_rs};
  const char* stn[] = {"q_es", "q_rs", "k_es", "k_rs"};
  ProfP<DenseKeys> p = {};
  const int rc = profile_common(who, a, st, stn, 4, p);
  if (rc != DL_OK) return rc;
  // the column count is launch-wide here: checked on the host (the kernel's DL_FLAG_MAP_COLS guard then never trips)
  const bool tail = a->key_tail_rows > 0;
  DL_CHECK_ARG(!tail || (a->key_tail_weight <= 16777216.f && a->key_tail_weight == (float)(int64_t)a->key_tail_weight), DL_ERR_ARG,
               "%s: a profile needs a whole key_tail_weight (got %g)", who, (double)a->key_tail_weight);
  const int64_t cols = tail ? (int64_t)(a->Lk - a->key_tail_rows) + (int64_t)a->key_tail_rows * (int64_t)a->key_tail_weight : (int64_t)a->Lk;
  DL_CHECK_ARG(cols <= (int64_t)a->out_cols, DL_ERR_SHAPE, "%s: a map of %ld columns does not fit out_cols = %d", who, (long)cols, a->out_cols);
  if (a->n_pairs == 0) return DL_OK;
  p.keys.k_es = a->k_es; p.keys.v_es = 0;
  p.keys.Lk = a->Lk;
  p.keys.tail_start = a->Lk - a->key_tail_rows;
  p.keys.tail_bias = 0.f;                               // (not read: the kernel takes log(dense_w) / scale itself)
  p.dense_w = tail ? a->key_tail_weight : 1.f;
  launch_profile(a->dtype, p, a->n_pairs, (hipStream_t)stream);
  DL_CHECK_LAUNCH("dl_pgca_pairs_profile");
  return DL_OK;
}

extern "C" int dl_pgca_pairs_ragged_profile(const dl_pgca_pairs_ragged_profile_args* a, dl_stream stream) {
  const char* who = "dl_pgca_pairs_ragged_profile";
  DL_CHECK_ARG(a, DL_ERR_ARG, "%s: null argument block", who);
  DL_CHECK_ARG(a->kv_total_rows >= 0, DL_ERR_SHAPE, "%s: kv_total_rows %ld is negative", who, (long)a->kv_total_rows);
  DL_CHECK_ARG(a->key_tail_rows >= 0, DL_ERR_ARG, "%s: key_tail_rows %d is negative", who, a->key_tail_rows);
  DL_CHECK_ARG(a->key_tail_rows <= MAX_KEYS, DL_ERR_UNSUPPORTED, "%s: key_tail_rows %d above the %d stored keys a profile launch serves", who,
               a->key_tail_rows, MAX_KEYS);
  const int64_t st[] = {a->q_es, a->q_rs, a->k_rs};
  const char* stn[] = {"q_es", "q_rs", "k_rs"};
  ProfP<RaggedKeys> p = {};
  const int rc = profile_common(who, a, st, stn, 3, p);
  if (rc != DL_OK || a->n_pairs == 0) return rc;
  DL_CHECK_ARG(a->kv_row0 && a->kv_keys && a->kv_tail_weight, DL_ERR_ARG, "%s: null pointer (kv_row0, kv_keys, kv_tail_weight)", who);
  DL_CHECK_ARG(((uintptr_t)a->kv_row0 & 7) == 0, DL_ERR_ALIGN, "%s: kv_row0 not 8-byte aligned", who);
  DL_CHECK_ARG((((uintptr_t)a->kv_keys | (uintptr_t)a->kv_tail_weight) & 3) == 0, DL_ERR_ALIGN,
               "%s: kv_keys / kv_tail_weight not 4-byte aligned", who);
  p.keys.row0 = a->kv_row0; p.keys.keys = a->kv_keys; p.keys.tailw = a->kv_tail_weight;
  p.keys.total_rows = a->kv_total_rows;
  p.keys.tail_rows = a->key_tail_rows;
  launch_profile(a->dtype, p, a->n_pairs, (hipStream_t)stream);
  DL_CHECK_LAUNCH("dl_pgca_pairs_ragged_profile");
  return DL_OK;
}
