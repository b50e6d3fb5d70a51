// pair_keys.cuh — how a pair-indexed PGCA kernel starts and ends, shared by the four kernel families of the screening path
// (pgca_pairs.hip: the attention core, pgca_pairs_probs.hip: the probability maps, pgca_pairs_profile.hip: the hit profiles,
// pgca_pairs_attr.hip: the hit attributions).  The tile steps in between are those of tiles.cuh.
//   Device: the `Keys` types a kernel is instantiated with (where the keys of one pair lie: one locate()), the guards in front
//   of the one atomic, the Q-fragment loader, and the per-wave column sums of the one-workgroup kernels with their finish.
//     DenseKeys  : entity d of K / V, k_es / v_es elements apart; Lk, the tail rows and their weight are launch-wide.
//     RaggedKeys : rows kv_row0[d] .. kv_row0[d] + kv_keys[d] - 1 of one packed [K | V'] row store, whose last key_tail_rows
//                  rows stand for kv_tail_weight[d] identical keys each (DrugLibrary); the table entry is read at the top of
//                  the workgroup (scalar loads: the entry's index is a scalar load itself).
//   Host: the checks and fills that the eight entry points share (every message starts with the entry point's name, `who`),
//   and the dtype launcher.
#pragma once
#include <math.h>
#include "common.cuh"
#include "tiles.cuh"

namespace dlpairs {

constexpr int KVB = 64, NKT = KVB / 16;   // keys per streamed tile, 16-key score tiles in it
constexpr int MAX_TILES = 9;              // the one-workgroup kernels keep a column sum per stored key: 576, the library's drugs have at most 520
constexpr int MAX_KEYS = MAX_TILES * KVB;
// 16-query tiles per wave: two in bf16, one in fp32 (the parity dtype)
template <typename T> constexpr int pair_qt() { return sizeof(T) == 2 ? 2 : 1; }

// the keys / values of one pair, as Keys::locate() finds them
struct KeySeg {
  int64_t k_off, v_off;            // elements from K / V to the segment's first row
  int Lk;
  int tail_start;                  // Lk - key_tail_rows (== Lk: no key multiplicities)
  float tail_bias;                 // log(w) / scale, added to the UNSCALED score of a tail key (as attention.hip)
};

struct DenseKeys {
  int64_t k_es, v_es;
  int Lk, tail_start;
  float tail_bias;
  __device__ __forceinline__ uint32_t locate(int di, int64_t, int64_t, float, KeySeg& s) const {
    s.k_off = (int64_t)di * k_es;
    s.v_off = (int64_t)di * v_es;
    s.Lk = Lk; s.tail_start = tail_start; s.tail_bias = tail_bias;
    return 0;
  }
};

struct RaggedKeys {
  const int64_t* row0;             // per drug: first row of its segment of the row store
  const int32_t* keys;             //           rows of the segment (Lk_d)
  const float* tailw;              //           multiplicity of each of the segment's last tail_rows rows
  int64_t total_rows;
  int tail_rows;                   // launch-wide key_tail_rows (0: no key multiplicities)
  // an entry that does not describe rows inside the store is not used
  __device__ __forceinline__ uint32_t locate(int di, int64_t k_rs, int64_t v_rs, float scale, KeySeg& s) const {
    const int64_t r0 = row0[di];
    const int Lk = keys[di];
    const float tw = tailw[di];
    if (r0 < 0 || Lk < max(1, tail_rows) || r0 > total_rows - (int64_t)Lk || !(tw >= 1.f && tw < INFINITY)) return DL_FLAG_KEY_TABLE;
    s.k_off = r0 * k_rs;
    s.v_off = r0 * v_rs;
    s.Lk = Lk; s.tail_start = Lk - tail_rows; s.tail_bias = logf(tw) / scale;
    return 0;
  }
};

// the multiplicity of drug di's tail keys (only read for an entry that locate() accepted)
__device__ __forceinline__ float tail_weight(const DenseKeys&, int, float dense_w) { return dense_w; }
__device__ __forceinline__ float tail_weight(const RaggedKeys& k, int di, float) { return k.tailw[di]; }

// ---- the guards.  All of them are uniform for the workgroup: the indices, what locate() reads and the multiplicity are scalar
//      loads (the keys' entry is read only through an index in range), and all of them stand in front of the one atomic, so
//      that nothing the compiler must treat as a store precedes them.  A pair with a flag is skipped: nothing is read through
//      its entry, nothing written.  p: the kernel's argument block (n_q, n_kv, k_rs, scale, keys; dense_w, out_cols). ----
// the index range (DL_FLAG_PAIR_INDEX) and the drug's table entry (DL_FLAG_KEY_TABLE)
template <typename P>
__device__ __forceinline__ uint32_t pair_guard(const P& p, int pi, int di, int64_t v_rs, KeySeg& ks) {
  const bool in_range = (unsigned)pi < (unsigned)p.n_q && (unsigned)di < (unsigned)p.n_kv;
  return in_range ? p.keys.locate(di, p.k_rs, v_rs, p.scale, ks) : (uint32_t)DL_FLAG_PAIR_INDEX;
}
// pair_guard(), then the columns of the pair's map: every copy of a tail key has its own column under `expand`, which needs a
// whole multiplicity <= 2^24; the map must fit out_cols and the drug max_keys stored keys (DL_FLAG_MAP_COLS).  tail_bias is
// log(w) / scale taken HERE, for both Keys types (ks.tail_bias is the host's for dense keys): 0 without `expand`.
template <typename P>
__device__ __forceinline__ uint32_t map_guard(const P& p, int pi, int di, bool expand, int max_keys, KeySeg& ks, int& copies, int& cols,
                                              float& tail_bias) {
  uint32_t bad = pair_guard(p, pi, di, 0, ks);
  copies = 1;
  tail_bias = 0.f;
  int64_t cols64 = ks.Lk;
  if (!bad && expand && ks.Lk > ks.tail_start) {
    const float w = tail_weight(p.keys, di, p.dense_w);
    if (w <= 16777216.f && w == truncf(w)) {
      copies = (int)w;
      cols64 = (int64_t)ks.tail_start + (int64_t)(ks.Lk - ks.tail_start) * copies;
      tail_bias = logf(w) / p.scale;
    } else {
      bad = DL_FLAG_MAP_COLS;
    }
  }
  if (!bad && (cols64 > (int64_t)p.out_cols || ks.Lk > max_keys)) bad = DL_FLAG_MAP_COLS;
  cols = (int)cols64;
  return bad;
}
// the one atomic of a skipped pair; writer: one thread of the pair's workgroups
__device__ __forceinline__ void flag_pair(uint32_t* flags, uint32_t bad, bool writer) {
  if (flags && writer) atomicOr(flags, bad);
}

// the Q fragments of a wave's QT 16-query tiles, kept in registers: this lane's query of tile qt is row qw0 + 16 qt + il
template <typename T, int QT, int NKF>
__device__ __forceinline__ void load_q_frags(u32x4 (&qf)[QT][NKF], const T* Qb, int64_t q_rs, int qw0, int Lq, int il, int g) {
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) {
    const int q = qw0 + qt * 16 + il;
#pragma unroll
    for (int kf = 0; kf < NKF; ++kf) qf[qt][kf] = dltile::frag_global<T>(Qb + (int64_t)q * q_rs, q < Lq, kf, g);
  }
}

// ---- the one-workgroup kernels (eight waves per pair, two sweeps per block of query rows, one pipeline over all blocks) ----
constexpr int PAIR1_WAVES = 8, PAIR1_THREADS = PAIR1_WAVES * 64;
// the tile that the step after step j of a block's 2 nt needs: sweep 2 starts over, and so does the next block
__device__ __forceinline__ int next_tile(int j, int nt) {
  const int jn = j + 1;
  return jn >= 2 * nt ? 0 : (jn >= nt ? jn - nt : jn);
}
// this wave's row of colsum[PAIR1_WAVES][MAX_KEYS], zeroed over the drug's nt tiles (only this wave touches it until the finish)
__device__ __forceinline__ float* colsum_begin(float* colsum, int wave, int lane, int nt) {
  float* cw = colsum + wave * MAX_KEYS;
  for (int k = lane; k < nt * KVB; k += 64) cw[k] = 0.f;
  return cw;
}
// cs, the sums of keys 4 g + r of 16-key tile kt at key k0 over the wave's queries -> the wave's row (keys >= Lk collect sums
// too; they are never read)
__device__ __forceinline__ void colsum_add(float* cw, int k0, int kt, int il, int g, f32x4 cs) {
  if (il == 0) {
    f32x4* a = reinterpret_cast<f32x4*>(cw + k0 + kt * 16 + 4 * g);
    *a = *a + cs;
  }
}
// after the last block: the waves' column sums in a fixed order (MEAN: over lq) -> out[0 .. out_cols); tail key j's sum goes to
// every copy's column lead + i t + j, +0.0f from `cols` on
template <bool MEAN>
__device__ __forceinline__ void colsum_finish(const float* colsum, float* out, int out_cols, int cols, int tail_start, int tail_rows, float lq) {
  __syncthreads();
  for (int col = threadIdx.x; col < out_cols; col += PAIR1_THREADS) {
    float v = 0.f;
    if (col < cols) {
      const int key = col < tail_start ? col : tail_start + (col - tail_start) % tail_rows;
      const float* cs = colsum + key;
      static_assert(PAIR1_WAVES == 8, "the fixed order below adds eight waves");
      v = ((cs[0] + cs[MAX_KEYS]) + (cs[2 * MAX_KEYS] + cs[3 * MAX_KEYS])) +
          ((cs[4 * MAX_KEYS] + cs[5 * MAX_KEYS]) + (cs[6 * MAX_KEYS] + cs[7 * MAX_KEYS]));
      if constexpr (MEAN) v /= lq;
    }
    out[col] = v;
  }
}

// =================================== host ======================================================
#define DL_TRY(call)                  \
  do {                                \
    const int rc_ = (call);           \
    if (rc_ != DL_OK) return rc_;     \
  } while (0)

// Nothing behind a pointer is looked at by any of these, and with n_pairs == 0 (no launch) an entry point looks at no pointer
// or stride either.
// what every argument block has
template <typename Args> int pair_head_checks(const char* who, const Args* a) {
  DL_CHECK_ARG(a->dtype == DL_F32 || a->dtype == DL_BF16, DL_ERR_ARG, "%s: bad dtype %d", who, a->dtype);
  DL_CHECK_ARG(a->head_dim == 128, DL_ERR_UNSUPPORTED, "%s: head_dim %d (one head of 128 only)", who, a->head_dim);
  DL_CHECK_ARG(a->n_pairs >= 0 && a->n_q >= 0 && a->n_kv >= 0, DL_ERR_SHAPE, "%s: negative count (n_pairs %d, n_q %d, n_kv %d)", who,
               a->n_pairs, a->n_q, a->n_kv);
  DL_CHECK_ARG(a->Lq > 0, DL_ERR_SHAPE, "%s: Lq %d must be positive", who, a->Lq);
  DL_CHECK_ARG(a->scale > 0.f, DL_ERR_ARG, "%s: scale must be positive", who);
  return DL_OK;
}
// st / stn: the entry point's strides and their names; skip, skip + 1: not looked at (strides of an absent operand)
inline int pair_stride_checks(const char* who, int dtype, const int64_t* st, const char* const* stn, int n_st, int skip = -2) {
  const int epc = 16 / (int)dl_dtype_size(dtype);
  for (int i = 0; i < n_st; ++i) {
    if (i == skip || i == skip + 1) continue;
    DL_CHECK_ARG(st[i] >= 0 && st[i] % epc == 0, DL_ERR_ALIGN, "%s: stride %s (%ld) not a non-negative multiple of %d elements", who,
                 stn[i], (long)st[i], epc);
  }
  return DL_OK;
}
template <typename Args> int pair_index_checks(const char* who, const Args* a) {
  DL_CHECK_ARG((((uintptr_t)a->q_index | (uintptr_t)a->kv_index | (uintptr_t)a->flags) & 3) == 0, DL_ERR_ALIGN,
               "%s: q_index / kv_index / flags not 4-byte aligned", who);
  return DL_OK;
}
// workgroups per pair of the kernels whose workgroup owns 64 * QT query rows
template <typename Args> int pair_blocks(const char* who, const Args* a, int& bps) {
  const int qt = a->dtype == DL_BF16 ? pair_qt<bf16_t>() : pair_qt<float>();
  bps = (a->Lq + 64 * qt - 1) / (64 * qt);
  DL_CHECK_ARG((int64_t)a->n_pairs * bps <= INT32_MAX, DL_ERR_SHAPE, "%s: too many workgroups (%d pairs x %d)", who, a->n_pairs, bps);
  return DL_OK;
}
// the fields of the launch block that every kernel has, from the fields that every argument block has
template <typename Args, typename P> void fill_pair_head(const Args* a, P& p) {
  p.Q = (const char*)a->Q; p.K = (const char*)a->K;
  p.qi = a->q_index; p.ki = a->kv_index; p.flags = a->flags;
  p.q_es = a->q_es; p.q_rs = a->q_rs; p.k_rs = a->k_rs;
  p.n_q = a->n_q; p.n_kv = a->n_kv; p.Lq = a->Lq;
  p.scale = a->scale;
}

// ---- dense keys: what an entry point checks first (serves, e.g. "a profile": Lk is held to MAX_KEYS), the launch-wide
//      column count (needs / what: the entry point's wording), the Keys fill ----
template <typename Args> int dense_head_checks(const char* who, const Args* a, const char* serves = nullptr) {
  DL_CHECK_ARG(a, DL_ERR_ARG, "%s: null argument block", who);
  DL_CHECK_ARG(a->Lq > 0 && a->Lk > 0, DL_ERR_SHAPE, "%s: Lq %d, Lk %d must be positive", who, a->Lq, a->Lk);
  DL_CHECK_ARG(!serves || a->Lk <= MAX_KEYS, DL_ERR_UNSUPPORTED, "%s: Lk %d above the %d stored keys %s launch serves", who, a->Lk, MAX_KEYS,
               serves);
  DL_CHECK_ARG(a->key_tail_rows >= 0 && a->key_tail_rows <= a->Lk, DL_ERR_ARG, "%s: key_tail_rows %d not in [0, Lk = %d]", who,
               a->key_tail_rows, a->Lk);
  DL_CHECK_ARG(a->key_tail_rows == 0 || a->key_tail_weight >= 1.f, DL_ERR_ARG, "%s: key_tail_weight %g below 1", who,
               (double)a->key_tail_weight);
  return DL_OK;
}
// (the kernel's DL_FLAG_MAP_COLS guard then never trips)
template <typename Args> int dense_cols_check(const char* who, const Args* a, bool expand, const char* needs, const char* what) {
  DL_CHECK_ARG(!expand || (a->key_tail_weight <= 16777216.f && a->key_tail_weight == (float)(int64_t)a->key_tail_weight), DL_ERR_ARG,
               "%s: %s a whole key_tail_weight (got %g)", who, needs, (double)a->key_tail_weight);
  const int64_t cols = expand ? (int64_t)(a->Lk - a->key_tail_rows) + (int64_t)a->key_tail_rows * (int64_t)a->key_tail_weight : (int64_t)a->Lk;
  DL_CHECK_ARG(cols <= (int64_t)a->out_cols, DL_ERR_SHAPE, "%s: a %s of %ld columns does not fit out_cols = %d", who, what, (long)cols, a->out_cols);
  return DL_OK;
}
// host_bias: the kernel reads KeySeg::tail_bias (else it takes log(dense_w) / scale itself).  Returns the launch-wide multiplicity.
template <typename Args> float fill_dense_keys(const Args* a, int64_t v_es, bool host_bias, DenseKeys& k) {
  k.k_es = a->k_es; k.v_es = v_es;
  k.Lk = a->Lk;
  k.tail_start = a->Lk - a->key_tail_rows;
  k.tail_bias = host_bias && a->key_tail_rows ? logf(a->key_tail_weight) / a->scale : 0.f;
  return a->key_tail_rows ? a->key_tail_weight : 1.f;
}

// ---- ragged keys: what an entry point checks first (serves: key_tail_rows is held to MAX_KEYS), and after the shared checks
//      the key table and the Keys fill ----
template <typename Args> int ragged_head_checks(const char* who, const Args* a, const char* serves = nullptr) {
  DL_CHECK_ARG(a, DL_ERR_ARG, "%s: null argument block", who);
  DL_CHECK_ARG(a->kv_total_rows >= 0, DL_ERR_SHAPE, "%s: kv_total_rows %ld is negative", who, (long)a->kv_total_rows);
  DL_CHECK_ARG(a->key_tail_rows >= 0, DL_ERR_ARG, "%s: key_tail_rows %d is negative", who, a->key_tail_rows);
  DL_CHECK_ARG(!serves || a->key_tail_rows <= MAX_KEYS, DL_ERR_UNSUPPORTED, "%s: key_tail_rows %d above the %d stored keys %s launch serves", who,
               a->key_tail_rows, MAX_KEYS, serves);
  return DL_OK;
}
template <typename Args> int fill_ragged_keys(const char* who, const Args* a, RaggedKeys& k) {
  DL_CHECK_ARG(a->kv_row0 && a->kv_keys && a->kv_tail_weight, DL_ERR_ARG, "%s: null pointer (kv_row0, kv_keys, kv_tail_weight)", who);
  DL_CHECK_ARG(((uintptr_t)a->kv_row0 & 7) == 0, DL_ERR_ALIGN, "%s: kv_row0 not 8-byte aligned", who);
  DL_CHECK_ARG((((uintptr_t)a->kv_keys | (uintptr_t)a->kv_tail_weight) & 3) == 0, DL_ERR_ALIGN,
               "%s: kv_keys / kv_tail_weight not 4-byte aligned", who);
  k.row0 = a->kv_row0; k.keys = a->kv_keys; k.tailw = a->kv_tail_weight;
  k.total_rows = a->kv_total_rows;
  k.tail_rows = a->key_tail_rows;
  return DL_OK;
}

// one kernel per dtype, the same launch
template <typename P>
void launch_by_dtype(int dtype, void (*k_bf16)(const P), void (*k_f32)(const P), uint32_t n_blocks, int threads, hipStream_t s, const P& p) {
  hipLaunchKernelGGL(dtype == DL_BF16 ? k_bf16 : k_f32, dim3(n_blocks), dim3(threads), 0, s, p);
}

}  // namespace dlpairs
