// Semi-global aggregation on float32 costs (include/mvs.h at mvs_sgm_d, mvs_sgm8_d and mvs_sgm8_batch_d): the
// float32 instantiation of sgm_kernels.h, every form up to kSgmMaxD levels.
#include "sgm_kernels.h"

namespace mvs {

int launch_sgm(hipStream_t s, int W, int H, int D, int N, const float* vol, size_t vol_stride, float P1, float P2,
               int paths, float* agg, size_t agg_stride) {
  return launch_sgm_paths<SgmF32, true>(s, W, H, D, N, vol, vol_stride, P1, P2, paths, agg, agg_stride, "k_sgm");
}

}  // namespace mvs
