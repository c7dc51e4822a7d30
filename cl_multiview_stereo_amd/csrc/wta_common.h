// The confidence rule of the winner passes, for the kernels that take a winner and fit at it (k_wta_agg_sub,
// wta.hip; k_wta_u16_sub, sgm16.hip).  Top4::emit and Top4u::emit state the same rule in place and keep their code.
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

}  // namespace mvs
