// What the winner passes over a volume [D][P] share (k_wta and k_wta_agg_sub, wta.hip, on float32; k_wta_u16 and
// k_wta_u16_sub, sgm16.hip, on uint16 read as int): the four smallest (cost, level) of a pixel, the scan over the
// levels that finds them (MVS_SCAN_TOP4), and the confidence rule.
#pragma once
#include <hip/hip_runtime.h>

namespace mvs {

// Of the three (cost, level) pairs behind the winner (level i0) in lexicographic order, the cost of the first whose
// level is more than one away from i0: the smallest cost outside i0 +- 1 (at most two of the three are adjacent to
// i0).  A level below 0 is an empty slot; `none` where there is no such pair.
template <class T>
__device__ __forceinline__ T second_cost(int i0, int i1, T v1, int i2, T v2, int i3, T v3, T none) {
  if (i1 >= 0 && (i1 < i0 - 1 || i1 > i0 + 1)) return v1;
  if (i2 >= 0 && (i2 < i0 - 1 || i2 > i0 + 1)) return v2;
  if (i3 >= 0 && (i3 < i0 - 1 || i3 > i0 + 1)) return v3;
  return none;
}

// the 4 smallest (cost, level) of one pixel in lexicographic order, from `init` (above every cost that counts) at
// level -1: the first is the first index of the minimum
template <class T>
struct Top4 {
  T v0, v1, v2, v3;
  int i0, i1, i2, i3;
  __device__ __forceinline__ void clear(T init) {
    v0 = v1 = v2 = v3 = init;
    i0 = i1 = i2 = i3 = -1;
  }
  __device__ __forceinline__ void insert(T cc, int ci) {
    if (cc < v3) {
      if (cc < v2) {
        v3 = v2; i3 = i2;
        if (cc < v1) {
          v2 = v1; i2 = i1;
          if (cc < v0) { v1 = v0; i1 = i0; v0 = cc; i0 = ci; }
          else { v1 = cc; i1 = ci; }
        } else { v2 = cc; i2 = ci; }
      } else { v3 = cc; i3 = ci; }
    }
  }
  __device__ __forceinline__ T second(T none) const { return second_cost(i0, i1, v1, i2, v2, i3, v3, none); }
};

// The Top4 t[NP] (T costs) of NP consecutive pixels over the D levels at col (const M*, plane pitch P elements),
// from init: UNR levels in flight, non-temporal.  NP = 1: one element per load.  NP > 1: one NP-wide vector per
// load, which needs P a multiple of NP and col aligned to NP elements.
// A macro, so that the scan stands in the kernel's own body.  As a __forceinline__ function the optimiser works on
// it alone first, insert's conditional stores being memory behind a reference then, and merges them into selects:
// k_wta_u16<4, 8> came out at 90 VGPRs against 62; on a local copied out at the end, at 62 VGPRs, 95 instructions
// more and 0.124 against 0.119 ms at 1080p, D = 128 (profiles/sgm_unify/ab.json).
#define MVS_SCAN_TOP4(NP, UNR, M, T, col, P, D, init, t)                                                \
  do {                                                                                                  \
    _Pragma("unroll") for (int s4k = 0; s4k < NP; s4k++) t[s4k].clear(init);                            \
    int s4d = 0;                                                                                        \
    if constexpr (NP == 1) {                                                                            \
      const M* s4c = col;                                                                               \
      for (; s4d + UNR <= D; s4d += UNR) {                                                              \
        T s4v[UNR];                                                                                     \
        _Pragma("unroll") for (int u = 0; u < UNR; u++)                                                 \
            s4v[u] = (T)__builtin_nontemporal_load(s4c + (long)(s4d + u) * P);                          \
        _Pragma("unroll") for (int u = 0; u < UNR; u++) t[0].insert(s4v[u], s4d + u);                   \
      }                                                                                                 \
      for (; s4d < D; s4d++) t[0].insert((T)s4c[(long)s4d * P], s4d);                                   \
    } else {                                                                                            \
      typedef M s4vec __attribute__((ext_vector_type(NP)));                                             \
      const s4vec* s4c = (const s4vec*)(col);                                                           \
      const long s4p = P / NP;                                                                          \
      for (; s4d + UNR <= D; s4d += UNR) {                                                              \
        s4vec s4v[UNR];                                                                                 \
        _Pragma("unroll") for (int u = 0; u < UNR; u++)                                                 \
            s4v[u] = __builtin_nontemporal_load(s4c + (long)(s4d + u) * s4p);                           \
        _Pragma("unroll") for (int u = 0; u < UNR; u++)                                                 \
            _Pragma("unroll") for (int k = 0; k < NP; k++) t[k].insert((T)s4v[u][k], s4d + u);          \
      }                                                                                                 \
      for (; s4d < D; s4d++) {                                                                          \
        const s4vec s4w = s4c[(long)s4d * s4p];                                                         \
        _Pragma("unroll") for (int k = 0; k < NP; k++) t[k].insert((T)s4w[k], s4d);                     \
      }                                                                                                 \
    }                                                                                                   \
  } while (0)

}  // namespace mvs
