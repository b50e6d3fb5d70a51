// tiles.cuh — LDS tile image + MFMA fragment loaders shared by the attention and NT-Xent kernels, the LDS-DMA row loader
// of the attention kernels, the three tile steps of the streamed forward, and the steps of the kernels that take the softmax
// statistics first: key masking, running statistics, LSE.
// Tiles are [rows][HD] with 16-byte chunks XOR-swizzled by ATile::swz(row); the same image serves
// ds_read_b128 (K-contiguous fragments) and ds_read_b64_tr_b16 / ds_read_b32 (transposed fragments).
#pragma once
#include <math.h>
#include "common.cuh"

namespace dltile {

constexpr float LOG2E = 1.4426950408889634f;
constexpr int ATT_THREADS = 256;

template <typename T, int HD> struct ATile {
  static constexpr int ES = (int)sizeof(T);
  static constexpr int RB = HD * ES;       // bytes per row
  static constexpr int CPR = RB / 16;      // 16-byte chunks per row
  static constexpr int EPC = 16 / ES;
  // XOR swizzle of a row's 16-byte chunks.  128-byte rows (bf16, head_dim 64): row & 7 — the row parity supplies
  // the fourth bank-space bit.  256-byte rows (bf16, head_dim 128) fill the 256-byte bank space on their own: the
  // 16 lanes of a ds_read_b128 group (rows il, chunk pair g) and the 32 lanes of a ds_read_b64_tr_b16 group (rows
  // 4g + q, adjacent chunks h) need FOUR swizzle bits, and row & 7 left both 2-way conflicted (SQ_LDS_BANK_CONFLICT
  // = 42-46 % of the LDS cycles of the head_dim-128 kernels): row bits 0..1 -> chunk bits 1..2, row bit 2 -> bit 3,
  // chunk bit 0 stays with g / h.
  __device__ static __forceinline__ int swz(int row) {
    if constexpr (ES == 2 && CPR == 16) return ((row & 3) << 1) | (((row >> 2) & 1) << 3);
    else return row & 7;
  }
  __device__ static __forceinline__ int off(int row, int col) {
    const int b = col * ES;
    return row * RB + ((((b >> 4) ^ swz(row))) << 4) + (b & 15);
  }
};

// ---- cooperative global -> LDS staging of NR rows (all 256 threads) -----------------------
// rows >= row_limit are zero filled.  NCH = chunks per thread.
template <typename T, int HD, int NR> struct Stager {
  using TL = ATile<T, HD>;
  static constexpr int NCH = (NR * TL::CPR + ATT_THREADS - 1) / ATT_THREADS;
  u32x4 r[NCH];
  __device__ __forceinline__ void load(const T* base, int64_t row_stride, int row0, int row_limit) {
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int c = threadIdx.x + i * ATT_THREADS;
      const int row = c / TL::CPR, ch = c % TL::CPR;
      u32x4 v = {0u, 0u, 0u, 0u};
      if (c < NR * TL::CPR && row0 + row < row_limit)
        v = *reinterpret_cast<const u32x4*>(base + (int64_t)(row0 + row) * row_stride + ch * TL::EPC);
      r[i] = v;
    }
  }
  __device__ __forceinline__ void store(char* lds) const {
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int c = threadIdx.x + i * ATT_THREADS;
      const int row = c / TL::CPR, ch = c % TL::CPR;
      if (c < NR * TL::CPR) lds_write16(lds, row * TL::RB + ((ch ^ TL::swz(row)) << 4), r[i]);
    }
  }
};

// K-contiguous fragment: rows rowbase+il, contraction chunk (kf, g)
template <typename T, int HD>
__device__ __forceinline__ u32x4 frag_kc(const char* lds, int rowbase, int kf, int il, int g) {
  using TL = ATile<T, HD>;
  const int row = rowbase + il;
  return lds_read16(lds, row * TL::RB + (((kf * 4 + g) ^ TL::swz(row)) << 4));
}
// K-contiguous fragment straight from global memory (kept in registers for a whole kernel)
template <typename T>
__device__ __forceinline__ u32x4 frag_global(const T* rowptr, bool valid, int kf, int g) {
  constexpr int KF = Mma<T>::KF;
  u32x4 v = {0u, 0u, 0u, 0u};
  if (valid) v = *reinterpret_cast<const u32x4*>(rowptr + kf * KF + g * (KF / 4));
  return v;
}
// Transposed fragment: A[i = colbase + il][slots <-> tile rows rbase + CTILE map]
// (covers KF rows: 32 for bf16, 16 for f32)
template <typename T, int HD>
__device__ __forceinline__ u32x4 frag_tr(const char* lds, int rbase, int colbase, int il, int g) {
  using TL = ATile<T, HD>;
  if constexpr (sizeof(T) == 2) {
    const int r0 = rbase + 4 * g + (il >> 2);
    const int col = colbase + (il & 3) * 4;
    const u32x2 a = lds_read_tr16(lds, TL::off(r0, col));
    const u32x2 b = lds_read_tr16(lds, TL::off(r0 + 16, col));
    u32x4 r = {a[0], a[1], b[0], b[1]};
    return r;
  } else {
    u32x4 r;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      r[j] = __builtin_bit_cast(uint32_t, lds_read_f32(lds, TL::off(rbase + 4 * g + j, colbase + il)));
    return r;
  }
}
// accumulator tiles -> fragment (CTILE map); `t` points at CT consecutive tiles
template <typename T>
__device__ __forceinline__ u32x4 frag_from_acc(const f32x4* t) {
  if constexpr (sizeof(T) == 2) return ctile_frag_bf16(t[0], t[1]);
  else return ctile_frag_f32(t[0]);
}

// v_exp_f32 without libm's denormal-range fix-up (arguments here are <= 0 and results below 2^-126 may flush);
// exp2(-inf) = 0 as the online softmax needs
__device__ __forceinline__ float fast_exp2(float x) { return __builtin_amdgcn_exp2f(x); }

// what the LDS-DMA loaders read for a row past the end of its tensor (const: every translation unit keeps its own copy)
__device__ __attribute__((aligned(16))) const uint32_t zero_page[4] = {0u, 0u, 0u, 0u};

// LDS-DMA of `total_rows` (a multiple of 64) rows of head_dim elements into an ATile image: source-side XOR
// swizzle, rows >= valid_rows read the zero page.  NT threads; complete for the workgroup after vm_wait<0>() + __syncthreads().
template <typename T, int HD, int NT>
__device__ __forceinline__ void dma_rows(char* lds, const T* base, int64_t row_stride, int valid_rows, int total_rows) {
  using TL = ATile<T, HD>;
  const int tid = threadIdx.x, wave = tid >> 6;
  const int nchunks = total_rows * TL::CPR;
  const char* zero = reinterpret_cast<const char*>(zero_page);
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

// ---- the three steps of the streamed forward on one tile of 16 * NKT keys, transposed layout: lane (il, g) holds keys
//      kt * 16 + 4 g + r of query il for each of the wave's QT 16-query tiles.  Raw-logit stores, key masking and the tail
//      bias go between the first and the second at the call site. ----
// S^T = K Q^T: K fragments from the LDS tile, Q fragments from registers
template <typename T, int HD, int QT, int NKT>
__device__ __forceinline__ void fwd_scores(const char* Ks, const u32x4 (&qf)[QT][HD / Mma<T>::KF], f32x4 (&s)[QT][NKT], int il, int g) {
  constexpr int NKF = HD / Mma<T>::KF;
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
}
// online softmax (per q = il; replicated over g): s becomes exp2(s * c - m_new * c), the running maximum and sum move on
// and o is rescaled
template <int QT, int NKT, int NDT>
__device__ __forceinline__ void fwd_softmax(f32x4 (&s)[QT][NKT], float (&m_run)[QT], float (&l_run)[QT], f32x4 (&o)[NDT][QT], float c) {
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
}
// O^T += V^T P^T: P^T straight from the accumulators, V^T by the LDS transpose read
template <typename T, int HD, int QT, int NKT>
__device__ __forceinline__ void fwd_accumulate(const char* Vs, const f32x4 (&s)[QT][NKT], f32x4 (&o)[HD / 16][QT], int il, int g) {
  constexpr int KF = Mma<T>::KF, NDT = HD / 16, CT = KF / 16, NKP = NKT * 16 / KF;
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
}

// ---- the tile steps of the kernels that need the softmax statistics first (attn_probs.hip and the two-sweep pair-indexed
//      kernels), same layout ----
// key multiplicities and key masking on the tile at key k0: tail keys get the bias on the UNSCALED score, keys >= Lk leave the
// softmax.  Tiles in front of both skip this through a uniform branch.
template <int QT, int NKT>
__device__ __forceinline__ void mask_keys(f32x4 (&s)[QT][NKT], int k0, int Lk, int tail_start, float tail_bias, int g) {
  if (k0 + NKT * 16 > tail_start || k0 + NKT * 16 > Lk) {
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
}
// the tail bias alone, where the statistics are known and no key is masked (a second pass over the scores)
template <int QT, int NKT>
__device__ __forceinline__ void bias_tail_keys(f32x4 (&s)[QT][NKT], int k0, int tail_start, float tail_bias, int g) {
  if (k0 + NKT * 16 > tail_start) {
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (k0 + kt * 16 + 4 * g + r >= tail_start) {
#pragma unroll
          for (int qt = 0; qt < QT; ++qt) s[qt][kt][r] += tail_bias;
        }
  }
}
// running maximum and sum (fwd_softmax's, s left as it is); WITH_G: under the same rescale the running sum of e g, g from a
// second score array gs (attributions).
// l_run / d_run are per-lane partials (own keys): lse2_join() reduces them.
template <bool WITH_G = false, int QT, int NKT>
__device__ __forceinline__ void sweep_stats(const f32x4 (&s)[QT][NKT], float (&m_run)[QT], float (&l_run)[QT], float c,
                                            const f32x4 (*gs)[NKT] = nullptr, float* d_run = nullptr) {
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
        const float e = fast_exp2(s[qt][kt][r] * c - mc);       // w exp(..) on a tail key: the bias is inside
        rs += e;
        if constexpr (WITH_G) rd = fmaf(e, gs[qt][kt][r], rd);
      }
    l_run[qt] = l_run[qt] * alpha + rs;
    if constexpr (WITH_G) d_run[qt] = d_run[qt] * alpha + rd;
    m_run[qt] = m_new;
  }
}
// between the sweeps: a query's sum from its four lanes' partials (returned), lse2 = LSE_q = m scale + log l in exp2 units
__device__ __forceinline__ float lse2_join(float m_run, float l_run, float scale, float& lse2) {
  const float l = group4_sum(l_run);
  lse2 = (m_run * scale + logf(l)) * LOG2E;
  return l;
}

// ---- LDS-DMA as inline assembly (invisible to the compiler's wait-count model: counted vmcnt waits stay counted) ----
// one instruction = 64 lanes x 16 (4) bytes -> 1 KB (256 B) of LDS at lds_off + 16 (4) * lane
__device__ __forceinline__ void lds_dma16(const void* gsrc, uint32_t lds_off) {
  asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" ::"v"(gsrc), "s"(lds_off) : "memory");
}
__device__ __forceinline__ void lds_dma4(const void* gsrc, uint32_t lds_off) {
  asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dword %0, off" ::"v"(gsrc), "s"(lds_off) : "memory");
}
template <int N> __device__ __forceinline__ void vm_wait() {
  static_assert(N >= 0 && N < 64, "vmcnt immediate");
  asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(N) : "memory");
}
__device__ __forceinline__ void raw_barrier() { asm volatile("s_barrier" ::: "memory"); }

}  // namespace dltile
