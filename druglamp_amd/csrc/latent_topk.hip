// latent_topk.hip — dot-product top-M of every query row against a resident library, without a (P, D) matrix.
//
// The streamed-similarity skeleton of ntxent.hip at 256-wide rows: a workgroup keeps 64 query rows as MFMA fragments in
// registers (one 16-row tile per wave) and streams its slab of the library 64 rows at a time through an LDS ring filled by
// LDS-DMA (bf16: v_mfma_f32_16x16x32_bf16, fp32: exact v_mfma_f32_16x16x4_f32).  A score is ONE accumulator chain over the
// 256 terms in fragment order, started from zero: its bits depend on the two rows alone, not on P, D, M, the slab or the
// row's place in a tile.
//
// Selection works on 64-bit keys: (order-preserving image of the fp32 score) << 32 | (2^32 - 1 - library index).  Keys of
// one query are distinct, a larger key is a better hit (value descending, then index ascending; a NaN score maps to the
// largest image, so it ranks first as in torch.topk), so "the M largest keys, descending" IS the specified order and the
// result cannot depend on the order in which candidates were found.
//   per (slab, query row): a candidate buffer of CAP = pow2(2 M + 64) keys (128 .. 2048) in the workspace, an LDS counter and an
//   LDS threshold (the M-th best key so far, 0 until M candidates exist).  A score whose key beats the threshold is
//   appended (LDS atomic on the counter, plain vector store of the key).  A buffer that could not take another full tile
//   (count > CAP - 64) is compacted: bitonic sort in LDS, the best M written back, the threshold raised.  Several rows are
//   sorted side by side when CAP is small.  After the warm-up appends are rare.
//   latent_topk_merge_kernel: one workgroup per query merges the slabs' sorted lists (bitonic merge) and decodes.
#include "tiles.cuh"

namespace {
using namespace dltile;

constexpr int LT_HD = 256;        // latent width
constexpr int LT_SORT = 2048;     // keys of the LDS sort buffer = the largest CAP (M <= 1024)
constexpr int LT_TARGET_WGS = 256;

struct LtP {
  const char *q, *lib;
  int64_t P, D, slab;
  int32_t nslab, M, cap_log2;
  unsigned long long* ws;
};

__device__ __forceinline__ uint64_t lt_key(float v, uint32_t idx) {
  uint32_t b = __builtin_bit_cast(uint32_t, v);
  if (b == 0x80000000u) b = 0u;                                   // -0 == +0: the index decides
  uint32_t o = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
  if ((b & 0x7fffffffu) > 0x7f800000u) o = 0xffffffffu;           // NaN above every number
  return ((uint64_t)o << 32) | (uint64_t)(0xffffffffu - idx);
}
__device__ __forceinline__ float lt_value(uint64_t key) {
  const uint32_t o = (uint32_t)(key >> 32);
  const uint32_t b = (o == 0xffffffffu) ? 0x7fc00000u : (o & 0x80000000u) ? (o & 0x7fffffffu) : ~o;
  return __builtin_bit_cast(float, b);
}

// bitonic network over `total` keys of `buf` (LDS), independent segments of `seg` keys (powers of two, seg <= total), every
// segment descending.  kfirst = 2: full sort.  kfirst = seg: the last merge alone (the segment is already bitonic).
// All threads of the workgroup; ends with a barrier.
__device__ __forceinline__ void lt_bitonic(uint64_t* buf, int total, int seg, int kfirst) {
  constexpr int NC = LT_SORT / 2 / ATT_THREADS;      // comparators per thread and step: all read before any is written back
  const int tid = threadIdx.x, half = total >> 1;
  for (int k = kfirst; k <= seg; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      uint64_t a[NC], b[NC];
      int at[NC];
#pragma unroll
      for (int u = 0; u < NC; ++u) {
        const int c = tid + u * ATT_THREADS;
        at[u] = ((c & ~(j - 1)) << 1) | (c & (j - 1));
        if (c < half) { a[u] = buf[at[u]]; b[u] = buf[at[u] | j]; }
      }
#pragma unroll
      for (int u = 0; u < NC; ++u) {
        const int c = tid + u * ATT_THREADS, i = at[u];
        const bool desc = ((i & k) == 0) || (k == seg);
        if (c < half && (desc ? (a[u] < b[u]) : (a[u] > b[u]))) { buf[i] = b[u]; buf[i | j] = a[u]; }
      }
      __syncthreads();
    }
}

__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

template <typename T>
__global__ __launch_bounds__(ATT_THREADS) void latent_topk_kernel(const LtP p) {
  using TL = ATile<T, LT_HD>;
  constexpr int KF = Mma<T>::KF, NKF = LT_HD / KF, NKT = 4;
  constexpr int TILE = 64 * TL::RB;
  constexpr int NCH = 64 * TL::CPR / ATT_THREADS;   // DMA instructions per thread per tile
  static_assert(64 * TL::CPR % ATT_THREADS == 0, "whole DMA instructions per thread");
  constexpr int NST = (TILE <= 32768) ? 3 : 2, D = NST - 1, PERT = NCH;      // fp32: two 64 KB tiles are what LDS holds
  static_assert(D <= 2 && (D - 1) * PERT < 64, "vmcnt immediate");
  __shared__ __attribute__((aligned(16))) char smem[NST * TILE];
  __shared__ uint64_t sortbuf[LT_SORT];
  __shared__ uint64_t thr_s[64];
  __shared__ int cnt_s[64], list_s[64], nlist_s;
  const uint32_t smem_lds = (uint32_t)(size_t)(__attribute__((address_space(3))) char*)smem;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, il = lane & 15, g = lane >> 4;
  const int slab_i = (int)(blockIdx.x % (uint32_t)p.nslab);
  const int64_t rowtile = blockIdx.x / (uint32_t)p.nslab;
  const int cap = 1 << p.cap_log2, M = p.M;
  const int64_t c0 = (int64_t)slab_i * p.slab, c1 = min(p.D, c0 + p.slab);     // this workgroup's library rows: c0 <= j < c1
  uint64_t* buf = reinterpret_cast<uint64_t*>(p.ws) + ((rowtile * p.nslab + slab_i) * 64) * (int64_t)cap;

  if (tid < 64) { cnt_s[tid] = 0; thr_s[tid] = 0ull; }
  if (tid == 0) nlist_s = 0;

  // resident query rows (rows past P: zeros, never appended)
  const int qrow = wave * 16 + il;
  const int64_t a = rowtile * 64 + qrow;
  const bool aok = a < p.P;
  u32x4 af[NKF];
  {
    const T* src = reinterpret_cast<const T*>(p.q) + (aok ? a : 0) * LT_HD;
#pragma unroll
    for (int kf = 0; kf < NKF; ++kf) af[kf] = frag_global<T>(src, aok, kf, g);
    // the fragments have landed before the loop: a load left pending here made the compiler wait for vmcnt(0) inside it,
    // behind the next tile's DMA — every tile then waited for its successor
#pragma unroll
    for (int kf = 0; kf < NKF; ++kf) asm volatile("" ::"v"(af[kf]));
  }

  // streamed tiles (ntxent.hip): LDS slot (row, physical chunk pc) receives the row's logical chunk pc ^ swz(row); rows past
  // the slab are clamped to its last row (their scores are not appended)
  auto issue = [&](int64_t j0, int b) {
    const uint32_t dst = smem_lds + b * TILE;
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int ch = tid + i * ATT_THREADS, row = ch / TL::CPR, pc = ch % TL::CPR;
      int64_t j = j0 + row; j = j < c1 ? j : c1 - 1;
      const char* src = p.lib + j * (int64_t)TL::RB + ((pc ^ TL::swz(row)) << 4);
      lds_dma16(src, __builtin_amdgcn_readfirstlane(dst + (uint32_t)((ch - (tid & 63)) * 16)));
    }
  };

  // compaction of the rows in list_s[0 .. n): cap-key segments sorted side by side, the best M written back, the
  // threshold raised.  Uniform over the workgroup; the caller has a barrier in front of it.
  auto compact = [&](int n) {
    const int per = LT_SORT >> p.cap_log2;
    for (int b0 = 0; b0 < n; b0 += per) {
      const int nb = min(per, n - b0), total = nb << p.cap_log2;
      for (int e = tid; e < total; e += ATT_THREADS) {
        const int r = list_s[b0 + (e >> p.cap_log2)], i = e & (cap - 1);
        sortbuf[e] = (i < cnt_s[r]) ? buf[(int64_t)r * cap + i] : 0ull;
      }
      __syncthreads();
      lt_bitonic(sortbuf, total, cap, 2);
      for (int e = tid; e < total; e += ATT_THREADS) {
        const int r = list_s[b0 + (e >> p.cap_log2)], i = e & (cap - 1);
        if (i < M) buf[(int64_t)r * cap + i] = sortbuf[e];
      }
      __syncthreads();
      if (tid < nb) {
        const int r = list_s[b0 + tid], c = min(cnt_s[r], M);
        cnt_s[r] = c;
        if (c == M) thr_s[r] = sortbuf[(tid << p.cap_log2) + M - 1];
      }
      __syncthreads();
    }
  };

  const int64_t nt = (c1 - c0 + 63) / 64;
#pragma unroll
  for (int t0 = 0; t0 < D; ++t0)
    if (t0 < nt) issue(c0 + (int64_t)t0 * 64, t0);
  __syncthreads();
  int bufi = 0;
  for (int64_t t = 0; t < nt; ++t, bufi = (bufi + 1 == NST) ? 0 : bufi + 1) {
    const int64_t j0 = c0 + t * 64;
    // tile t has landed once only the younger tile's requests are outstanding; past the barrier every wave is also done
    // with tile t - 1, whose buffer takes tile t + D.  (Key stores of this loop also count in vmcnt: more outstanding
    // requests only make the counted wait wait longer, and loads return in order.)
    const int younger = (int)min((int64_t)(D - 1), nt - 1 - t);
    if (younger <= 0) vm_wait<0>();
    else vm_wait<PERT>();
    raw_barrier();
    if (t + D < nt) issue(c0 + (t + D) * 64, (bufi + D) % NST);
    const char* Bs = smem + bufi * TILE;
    f32x4 s[NKT];
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt) {
      s[kt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kf = 0; kf < NKF; ++kf) s[kt] = Mma<T>::mma(frag_kc<T, LT_HD>(Bs, kt * 16, kf, il, g), af[kf], s[kt]);
    }
    // lane (il, g) holds library rows j0 + kt * 16 + 4 g + r of query row `qrow`
    if (aok) {
      const uint64_t thr = thr_s[qrow];
      uint64_t* mine = buf + (int64_t)qrow * cap;
#pragma unroll
      for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int64_t j = j0 + kt * 16 + 4 * g + r;
          const uint64_t key = lt_key(s[kt][r], (uint32_t)j);
          if (j < c1 && key > thr) {
            const int pos = atomicAdd(&cnt_s[qrow], 1);      // < cap: count <= cap - 64 before a tile, at most 64 per tile
            mine[pos] = key;
          }
        }
    }
    // the two barriers of every tile are bare (LDS traffic alone): a fence here would also wait for the tiles in flight
    lds_barrier();
    if (tid < 64 && cnt_s[tid] > cap - 64) list_s[atomicAdd(&nlist_s, 1)] = tid;
    lds_barrier();
    const int n = nlist_s;
    if (n) {
      vm_wait<0>();            // every wave's key stores are done before any wave reads a buffer back
      __syncthreads();
      compact(n);
      if (tid == 0) nlist_s = 0;
    }
  }
  vm_wait<0>();
  // the slab's result: every row's best M, sorted, in the first M keys of its buffer (zeros where the slab has fewer)
  __syncthreads();
  if (tid < 64) list_s[tid] = tid;
  __syncthreads();
  compact(64);
}

__global__ __launch_bounds__(ATT_THREADS) void latent_topk_merge_kernel(const LtP p, float* __restrict__ values,
                                                                        int32_t* __restrict__ indices) {
  __shared__ uint64_t sortbuf[LT_SORT];
  const int tid = threadIdx.x, M = p.M, cap = 1 << p.cap_log2;
  int m2 = 1;
  while (m2 < M) m2 <<= 1;
  const int64_t row = blockIdx.x, rowtile = row >> 6;
  const int r = (int)(row & 63);
  const uint64_t* base = reinterpret_cast<const uint64_t*>(p.ws);
  auto list = [&](int s) { return base + ((rowtile * p.nslab + s) * 64 + r) * (int64_t)cap; };
  {
    const uint64_t* l0 = list(0);
    for (int i = tid; i < m2; i += ATT_THREADS) sortbuf[i] = i < M ? l0[i] : 0ull;
  }
  __syncthreads();
  for (int s = 1; s < p.nslab; ++s) {
    // descending list, then the next slab's list reversed: a bitonic sequence, one merge sorts it
    const uint64_t* ls = list(s);
    for (int i = tid; i < m2; i += ATT_THREADS) sortbuf[2 * m2 - 1 - i] = i < M ? ls[i] : 0ull;
    __syncthreads();
    lt_bitonic(sortbuf, 2 * m2, 2 * m2, 2 * m2);
  }
  for (int i = tid; i < M; i += ATT_THREADS) {
    const uint64_t key = sortbuf[i];
    values[row * M + i] = lt_value(key);
    indices[row * M + i] = (int32_t)(0xffffffffu - (uint32_t)key);
  }
}

// the launch geometry of (P, D, M, slab): slab == 0 asks for the host's choice
struct LtGeom { int64_t slab, rowtiles, nslab; int cap_log2; };
bool lt_geometry(int64_t P, int64_t D, int32_t M, int64_t slab, LtGeom& g) {
  if (P < 1 || D < 1 || D >= (1ll << 31) || M < 1 || M > 1024 || M > D) return false;
  if (slab < 0 || slab % 64 != 0) return false;
  int cl = 7;                                      // CAP = pow2(2 M + 64) in [128, 2048]: room for M kept + M new + one tile
  while (cl < 11 && (1 << cl) < 2 * M + 64) ++cl;
  g.cap_log2 = cl;
  g.rowtiles = (P + 63) / 64;
  if (slab == 0) {
    // enough workgroups to fill the chip, but slabs long enough that the warm-up (about M ln(slab / M) appends per row)
    // stays small beside the streaming
    const int64_t min_slab = std::max<int64_t>(4096, 4ll << cl);
    int64_t ns = std::min<int64_t>((LT_TARGET_WGS + g.rowtiles - 1) / g.rowtiles, (D + min_slab - 1) / min_slab);
    ns = std::max<int64_t>(ns, 1);
    slab = ((D + ns - 1) / ns + 63) / 64 * 64;
  }
  g.slab = slab;
  g.nslab = (D + slab - 1) / slab;
  return true;
}
}  // namespace

extern "C" size_t dl_latent_topk_workspace_bytes(int64_t P, int64_t D, int32_t M, int64_t slab) {
  LtGeom g;
  if (!lt_geometry(P, D, M, slab, g)) return 0;
  return (size_t)g.rowtiles * (size_t)g.nslab * 64u * ((size_t)8 << g.cap_log2);
}

extern "C" int dl_latent_topk(const void* q, const void* lib, int64_t P, int64_t D, int32_t M, int32_t dtype, int64_t slab,
                              float* values, int32_t* indices, dl_stream stream, void* workspace, size_t workspace_bytes) {
  hipStream_t s = (hipStream_t)stream;
  DL_CHECK_ARG(q && lib && values && indices, DL_ERR_ARG, "dl_latent_topk: null pointer");
  DL_CHECK_ARG(dtype == DL_F32 || dtype == DL_BF16, DL_ERR_ARG, "dl_latent_topk: bad dtype");
  DL_CHECK_ARG(P >= 1, DL_ERR_ARG, "dl_latent_topk: P must be >= 1 (got %ld)", (long)P);
  DL_CHECK_ARG(D >= 1 && D < (1ll << 31), DL_ERR_SHAPE, "dl_latent_topk: D must be in [1, 2^31) (got %ld)", (long)D);
  DL_CHECK_ARG(M >= 1 && M <= 1024 && M <= D, DL_ERR_ARG, "dl_latent_topk: M must be in [1, min(D, 1024)] (got %d, D %ld)", M, (long)D);
  DL_CHECK_ARG(slab >= 0 && slab % 64 == 0, DL_ERR_ARG, "dl_latent_topk: slab must be 0 (host's choice) or a positive multiple of 64 (got %ld)", (long)slab);
  DL_CHECK_ARG(aligned_to(q, 16) && aligned_to(lib, 16), DL_ERR_ALIGN, "dl_latent_topk: q and lib rows must be 16-byte aligned");
  DL_CHECK_ARG(aligned_to(values, 4) && aligned_to(indices, 4), DL_ERR_ALIGN, "dl_latent_topk: values and indices must be 4-byte aligned");
  LtGeom g;
  DL_CHECK_ARG(lt_geometry(P, D, M, slab, g), DL_ERR_ARG, "dl_latent_topk: bad shape");
  DL_CHECK_ARG(g.rowtiles * g.nslab < (1ll << 31) && P < (1ll << 31), DL_ERR_SHAPE,
               "dl_latent_topk: %ld row tiles x %ld slabs do not fit one grid", (long)g.rowtiles, (long)g.nslab);
  DL_CHECK_ARG(workspace && aligned_to(workspace, 8) && workspace_bytes >= dl_latent_topk_workspace_bytes(P, D, M, slab), DL_ERR_WORKSPACE,
               "dl_latent_topk: workspace too small");
  LtP p;
  p.q = (const char*)q; p.lib = (const char*)lib; p.P = P; p.D = D; p.slab = g.slab; p.nslab = (int32_t)g.nslab; p.M = M;
  p.cap_log2 = g.cap_log2; p.ws = (unsigned long long*)workspace;
  const dim3 grid((uint32_t)(g.rowtiles * g.nslab));
  if (dtype == DL_BF16) hipLaunchKernelGGL(latent_topk_kernel<bf16_t>, grid, dim3(ATT_THREADS), 0, s, p);
  else hipLaunchKernelGGL(latent_topk_kernel<float>, grid, dim3(ATT_THREADS), 0, s, p);
  DL_CHECK_LAUNCH("dl_latent_topk");
  hipLaunchKernelGGL(latent_topk_merge_kernel, dim3((uint32_t)P), dim3(ATT_THREADS), 0, s, p, values, indices);
  DL_CHECK_LAUNCH("dl_latent_topk(merge)");
  return DL_OK;
}
