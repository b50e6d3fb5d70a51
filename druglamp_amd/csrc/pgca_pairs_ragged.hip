// pgca_pairs_ragged.hip — pair-indexed PGCA attention core over a packed per-drug row store (forward only): the resident
// drug library of the screening path.  See include/druglamp_hip.h (dl_pgca_pairs_ragged_fwd) for the addressing.
//
//   Pair n reads its queries from entity q_index[n] of Q, exactly as dl_pgca_pairs_fwd does, and its keys / values from the
//   segment of drug d = kv_index[n] in one packed [K | V'] row store: rows kv_row0[d] .. kv_row0[d] + kv_keys[d] - 1, whose last
//   key_tail_rows rows stand for kv_tail_weight[d] identical keys each (druglamp_amd/screening.py, DrugLibrary).
//
//   pgca_pairs_ragged_kernel : pgca_pairs.hip's kernel with the per-workgroup quantities (Kb, Vb, Lk, tail_start, tail_bias)
//                       taken from the table at the top of the workgroup (scalar loads: the entry's index is a scalar load
//                       itself); loader and tile loop are that file's (copied: each file keeps them in its anonymous namespace).
//                       The grid is n_pairs x ceil(Lq / (64 QT)) whatever the drugs' key counts; the workgroups of a short
//                       drug run fewer tiles.  Rows >= Lk of the last tile read the zero page, never the next drug's rows.
//                       A pair whose index is out of range (DL_FLAG_PAIR_INDEX), or whose drug's table entry does not
//                       describe rows inside the store (DL_FLAG_KEY_TABLE), returns before it reads anything through the
//                       entry or writes anything; both tests are uniform for the workgroup.
#include "tiles.cuh"

namespace {
using namespace dltile;

// v_exp_f32 without libm's denormal-range fix-up (arguments here are <= 0 and results below 2^-126 may flush);
// exp2(-inf) = 0 as the online softmax needs
__device__ __forceinline__ float fast_exp2(float x) { return __builtin_amdgcn_exp2f(x); }

struct RaggedP {
  const char *Q, *K, *V, *left;
  char* out;
  const float* bias;
  const int32_t *qi, *ki;
  const int64_t* row0;             // per drug: first row of its segment of the row store
  const int32_t* keys;             //           rows of the segment (Lk_d)
  const float* tailw;              //           multiplicity of each of the segment's last tail_rows rows
  uint32_t* flags;
  int64_t q_es, q_rs, k_rs, v_rs, left_es, left_rs, out_ps, out_rs, total_rows;
  int n_q, n_kv, Lq, bps;          // bps: workgroups per pair
  int left_chunks;                 // 16-byte chunks of a row of `left` (0: no copy)
  int out_col0;
  float scale;
  int tail_rows;                   // launch-wide key_tail_rows (0: no key multiplicities)
};

__device__ __attribute__((aligned(16))) const uint32_t ragged_zero_page[4] = {0u, 0u, 0u, 0u};

// LDS-DMA of `total_rows` (a multiple of 64) rows of head_dim elements into an ATile image: source-side XOR
// swizzle, rows >= valid_rows read a zero page.  NT threads; complete for the workgroup after vm_wait<0>() + __syncthreads().
// (attention.hip's loader: that file keeps it in its anonymous namespace)
template <typename T, int HD, int NT>
__device__ __forceinline__ void dma_rows(char* lds, const T* base, int64_t row_stride, int valid_rows, int total_rows) {
  using TL = ATile<T, HD>;
  const int tid = threadIdx.x, wave = tid >> 6;
  const int nchunks = total_rows * TL::CPR;
  const char* zero = reinterpret_cast<const char*>(ragged_zero_page);
  for (int c0 = 0; c0 < nchunks; c0 += NT) {
    const int c = c0 + tid;
    const int row = c / TL::CPR, ch = (c % TL::CPR) ^ TL::swz(row);
    const char* src = (c < nchunks && row < valid_rows) ? reinterpret_cast<const char*>(base + (int64_t)row * row_stride + ch * TL::EPC) : zero;
    const uint32_t off = __builtin_amdgcn_readfirstlane((uint32_t)((c0 + wave * 64) * 16));
    if (c0 + wave * 64 < nchunks)
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                       (__attribute__((address_space(3))) void*)(lds + off), 16, 0, 0);
  }
}

constexpr int KVB = 64;            // keys per streamed tile

// LDS: two (K tile, V tile) pairs = 64 KB in bf16 (two workgroups per CU), 128 KB in fp32 (one: the parity dtype)
template <typename T, int HD, int QT>
__global__ __launch_bounds__(ATT_THREADS, 2) void pgca_pairs_ragged_kernel(const RaggedP p) {
  using TL = ATile<T, HD>;
  constexpr int KF = Mma<T>::KF, NKF = HD / KF, NDT = HD / 16, CT = KF / 16;
  constexpr int NKT = KVB / 16, NKP = KVB / KF;
  constexpr int QB = 4 * QT * 16;
  constexpr int BUF = 2 * KVB * TL::RB;                 // one (K tile, V tile) pair
  __shared__ __attribute__((aligned(16))) char smem[2 * BUF];

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, il = lane & 15, g = lane >> 4;
  const int n = blockIdx.x / p.bps, qb = blockIdx.x % p.bps;
  const int pi = p.qi[n], di = p.ki[n];
  // Both guards are uniform for the workgroup: the indices and the drug's table entry are scalar loads (the entry is read
  // only through an index in range; all of them in front of the one atomic, so that nothing the compiler must treat as a
  // store precedes them).  An entry that does not describe rows inside the store is not used.
  uint32_t bad = 0;
  int64_t row0 = 0;
  int Lk = 0;
  float tw = 1.f;
  if ((unsigned)pi >= (unsigned)p.n_q || (unsigned)di >= (unsigned)p.n_kv) {
    bad = DL_FLAG_PAIR_INDEX;
  } else {
    row0 = p.row0[di];
    Lk = p.keys[di];
    tw = p.tailw[di];
    if (row0 < 0 || Lk < max(1, p.tail_rows) || row0 > p.total_rows - (int64_t)Lk || !(tw >= 1.f && tw < INFINITY)) bad = DL_FLAG_KEY_TABLE;
  }
  if (bad) {                                            // the pair is skipped: nothing read through the entry, nothing written
    if (p.flags && qb == 0 && threadIdx.x == 0) atomicOr(p.flags, bad);
    return;
  }
  const int tail_start = Lk - p.tail_rows;              // == Lk: no key multiplicities
  const float tail_bias = logf(tw) / p.scale;           // added to the UNSCALED score of a tail key (as attention.hip)
  const T* Qb = reinterpret_cast<const T*>(p.Q) + (int64_t)pi * p.q_es;
  const T* Kb = reinterpret_cast<const T*>(p.K) + row0 * p.k_rs;
  const T* Vb = reinterpret_cast<const T*>(p.V) + row0 * p.v_rs;
  T* Ob = reinterpret_cast<T*>(p.out) + (int64_t)n * p.out_ps;

  const int qw0 = qb * QB + wave * QT * 16;
  u32x4 qf[QT][NKF];
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) {
    const int q = qw0 + qt * 16 + il;
#pragma unroll
    for (int kf = 0; kf < NKF; ++kf) qf[qt][kf] = frag_global<T>(Qb + (int64_t)q * p.q_rs, q < p.Lq, kf, g);
  }

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
    // ---- S^T = K Q^T ----
    f32x4 s[QT][NKT];
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt) {
#pragma unroll
      for (int qt = 0; qt < QT; ++qt) s[qt][kt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kf = 0; kf < NKF; ++kf) {
        const u32x4 ka = frag_kc<T, HD>(Ks, kt * 16, kf, il, g);
#pragma unroll
        for (int qt = 0; qt < QT; ++qt) s[qt][kt] = Mma<T>::mma(ka, qf[qt][kf], s[qt][kt]);
      }
    }
    // ---- key multiplicities, key masking (tiles in front of both skip this through a uniform branch) ----
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
    // ---- online softmax (per q = il; replicated over g) ----
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
        for (int r = 0; r < 4; ++r) {
          const float e = fast_exp2(s[qt][kt][r] * c - mc);
          s[qt][kt][r] = e;
          rs += e;
        }
      l_run[qt] = l_run[qt] * alpha + rs;   // per-lane partial (own keys); reduced at the end
      m_run[qt] = m_new;
#pragma unroll
      for (int d = 0; d < NDT; ++d) o[d][qt] *= alpha;
    }
    // ---- O^T += V^T P^T ----
#pragma unroll
    for (int kp = 0; kp < NKP; ++kp) {
      u32x4 pb[QT];
#pragma unroll
      for (int qt = 0; qt < QT; ++qt) pb[qt] = frag_from_acc<T>(&s[qt][kp * CT]);
#pragma unroll
      for (int d = 0; d < NDT; ++d) {
        const u32x4 va = frag_tr<T, HD>(Vs, kp * KF, d * 16, il, g);
#pragma unroll
        for (int qt = 0; qt < QT; ++qt) o[d][qt] = Mma<T>::mma(va, pb[qt], o[d][qt]);
      }
    }
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

template <typename T> constexpr int ragged_qt() { return sizeof(T) == 2 ? 2 : 1; }

template <typename T>
void launch_ragged(RaggedP& p, int n_pairs, hipStream_t s) {
  constexpr int QT = ragged_qt<T>();
  hipLaunchKernelGGL((pgca_pairs_ragged_kernel<T, 128, QT>), dim3((uint32_t)n_pairs * (uint32_t)p.bps), dim3(ATT_THREADS), 0, s, p);
}

}  // namespace

extern "C" int dl_pgca_pairs_ragged_fwd(const dl_pgca_pairs_ragged_args* a, dl_stream stream) {
  hipStream_t s = (hipStream_t)stream;
  const char* who = "dl_pgca_pairs_ragged_fwd";
  DL_CHECK_ARG(a, DL_ERR_ARG, "%s: null argument block", who);
  DL_CHECK_ARG(a->dtype == DL_F32 || a->dtype == DL_BF16, DL_ERR_ARG, "%s: bad dtype %d", who, a->dtype);
  DL_CHECK_ARG(a->head_dim == 128, DL_ERR_UNSUPPORTED, "%s: head_dim %d (one head of 128 only)", who, a->head_dim);
  DL_CHECK_ARG(a->n_pairs >= 0 && a->n_q >= 0 && a->n_kv >= 0, DL_ERR_SHAPE, "%s: negative count (n_pairs %d, n_q %d, n_kv %d)", who,
               a->n_pairs, a->n_q, a->n_kv);
  DL_CHECK_ARG(a->Lq > 0, DL_ERR_SHAPE, "%s: Lq %d must be positive", who, a->Lq);
  DL_CHECK_ARG(a->kv_total_rows >= 0, DL_ERR_SHAPE, "%s: kv_total_rows %ld is negative", who, (long)a->kv_total_rows);
  DL_CHECK_ARG(a->key_tail_rows >= 0, DL_ERR_ARG, "%s: key_tail_rows %d is negative", who, a->key_tail_rows);
  DL_CHECK_ARG(a->scale > 0.f, DL_ERR_ARG, "%s: scale must be positive", who);
  DL_CHECK_ARG(a->left_cols >= 0 && a->left_cols % 8 == 0, DL_ERR_ALIGN, "%s: left_cols %d not a non-negative multiple of 8 elements", who,
               a->left_cols);
  DL_CHECK_ARG(a->out_col0 >= 0 && a->out_col0 % 8 == 0, DL_ERR_ALIGN, "%s: out_col0 %d not a non-negative multiple of 8 elements", who,
               a->out_col0);
  DL_CHECK_ARG((a->left != nullptr) == (a->left_cols > 0), DL_ERR_ARG, "%s: left and left_cols (%d) go together", who, a->left_cols);
  DL_CHECK_ARG(a->out_col0 >= a->left_cols, DL_ERR_ARG, "%s: out_col0 %d overlaps the left_cols %d copied columns", who, a->out_col0,
               a->left_cols);
  if (a->n_pairs == 0) return DL_OK;
  DL_CHECK_ARG(a->Q && a->K && a->V && a->out && a->q_index && a->kv_index, DL_ERR_ARG, "%s: null pointer (Q, K, V, out, q_index, kv_index)", who);
  DL_CHECK_ARG(a->kv_row0 && a->kv_keys && a->kv_tail_weight, DL_ERR_ARG, "%s: null pointer (kv_row0, kv_keys, kv_tail_weight)", who);
  const int epc = 16 / (int)dl_dtype_size(a->dtype);
  const int64_t st[] = {a->q_es, a->q_rs, a->k_rs, a->v_rs, a->left_es, a->left_rs, a->out_ps, a->out_rs};
  const char* stn[] = {"q_es", "q_rs", "k_rs", "v_rs", "left_es", "left_rs", "out_ps", "out_rs"};
  for (int i = 0; i < 8; ++i) {
    if (!a->left && (i == 4 || i == 5)) continue;       // (left_es / left_rs are not read without left)
    DL_CHECK_ARG(st[i] >= 0 && st[i] % epc == 0, DL_ERR_ALIGN, "%s: stride %s (%ld) not a non-negative multiple of %d elements", who,
                 stn[i], (long)st[i], epc);
  }
  DL_CHECK_ARG((((uintptr_t)a->Q | (uintptr_t)a->K | (uintptr_t)a->V | (uintptr_t)a->out | (uintptr_t)a->left | (uintptr_t)a->bias) & 15) == 0,
               DL_ERR_ALIGN, "%s: Q / K / V / left / out / bias not 16-byte aligned", who);
  DL_CHECK_ARG((((uintptr_t)a->q_index | (uintptr_t)a->kv_index | (uintptr_t)a->flags) & 3) == 0, DL_ERR_ALIGN,
               "%s: q_index / kv_index / flags not 4-byte aligned", who);
  DL_CHECK_ARG(((uintptr_t)a->kv_row0 & 7) == 0, DL_ERR_ALIGN, "%s: kv_row0 not 8-byte aligned", who);
  DL_CHECK_ARG((((uintptr_t)a->kv_keys | (uintptr_t)a->kv_tail_weight) & 3) == 0, DL_ERR_ALIGN,
               "%s: kv_keys / kv_tail_weight not 4-byte aligned", who);
  DL_CHECK_ARG(a->out_rs >= (int64_t)a->out_col0 + a->head_dim, DL_ERR_SHAPE, "%s: out_rs %ld below out_col0 + head_dim = %d", who,
               (long)a->out_rs, a->out_col0 + a->head_dim);
  const int qt = a->dtype == DL_BF16 ? ragged_qt<bf16_t>() : ragged_qt<float>();
  const int bps = (a->Lq + 64 * qt - 1) / (64 * qt);
  DL_CHECK_ARG((int64_t)a->n_pairs * bps <= INT32_MAX, DL_ERR_SHAPE, "%s: too many workgroups (%d pairs x %d)", who, a->n_pairs, bps);
  RaggedP p = {};
  p.Q = (const char*)a->Q; p.K = (const char*)a->K; p.V = (const char*)a->V; p.left = (const char*)a->left;
  p.out = (char*)a->out; p.bias = a->bias; p.qi = a->q_index; p.ki = a->kv_index; p.flags = a->flags;
  p.row0 = a->kv_row0; p.keys = a->kv_keys; p.tailw = a->kv_tail_weight;
  p.q_es = a->q_es; p.q_rs = a->q_rs; p.k_rs = a->k_rs; p.v_rs = a->v_rs;
  p.left_es = a->left_es; p.left_rs = a->left_rs; p.out_ps = a->out_ps; p.out_rs = a->out_rs; p.total_rows = a->kv_total_rows;
  p.n_q = a->n_q; p.n_kv = a->n_kv; p.Lq = a->Lq; p.bps = bps;
  p.left_chunks = a->left ? a->left_cols / epc : 0;
  p.out_col0 = a->out_col0;
  p.scale = a->scale;
  p.tail_rows = a->key_tail_rows;
  if (a->dtype == DL_BF16) launch_ragged<bf16_t>(p, a->n_pairs, s);
  else launch_ragged<float>(p, a->n_pairs, s);
  DL_CHECK_LAUNCH("dl_pgca_pairs_ragged_fwd");
  return DL_OK;
}
