// pair_keys.cuh — where a pair-indexed PGCA kernel finds the keys of one pair: the `Keys` types that pgca_pairs.hip (the
// attention core) and pgca_pairs_probs.hip (the probability maps) are instantiated with, so that both use one locate().
//     DenseKeys  : entity d of K / V, k_es / v_es elements apart; Lk, the tail rows and their weight are launch-wide.
//     RaggedKeys : rows kv_row0[d] .. kv_row0[d] + kv_keys[d] - 1 of one packed [K | V'] row store, whose last key_tail_rows
//                  rows stand for kv_tail_weight[d] identical keys each (DrugLibrary); the table entry is read at the top of
//                  the workgroup (scalar loads: the entry's index is a scalar load itself).
#pragma once
#include <math.h>
#include "common.cuh"

namespace dlpairs {

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

}  // namespace dlpairs
