// The passes over a materialised NCC cost volume [D][H][W] (ncc.hip's definition) for gfx950.
//
//  k_wta             winner-take-all + confidence over the materialised volume
//                    (the HBM-streaming pass the roofline is quoted on); the fused
//                    sweeps (ncc.hip, ncc_mfma.hip) fold the same from kWtaInit
//  k_wta_sub         winner-take-all + the sub-level parabola fit (definition: ncc_sub.hip)
//  k_wta_agg_sub     k_wta over an aggregate + the fit through the raw volume's costs at the aggregate's winner
#include "ncc_common.h"
#include "wta_common.h"

namespace mvs {
namespace {
using namespace ncc;

// ---- winner-take-all + confidence ----------------------------------------
// c2 - c0 of the winner c0 and the smallest cost c2 outside its neighbour levels; 0 where either is missing
__device__ __forceinline__ float confidence(const Top4<float>& t) {
  const float c2 = t.second(kWtaInit);
  return (t.i0 < 0 || c2 == kWtaInit) ? 0.0f : c2 - t.v0;
}

// One lane per NP consecutive pixels (NP-wide non-temporal vector loads, so a
// wave streams 256 NP contiguous bytes per level), UNR levels in flight.
template <int NP, int UNR>
__global__ __launch_bounds__(256) void k_wta(const float* __restrict__ vol, const float* __restrict__ levels, long P,
                                             int D, float* __restrict__ disp, float* __restrict__ conf) {
  const long p = (blockIdx.x * (long)blockDim.x + threadIdx.x) * NP;
  if (p >= P) return;
  Top4<float> t[NP];
  MVS_SCAN_TOP4(NP, UNR, float, float, vol + p, P, D, kWtaInit, t);
#pragma unroll
  for (int k = 0; k < NP; k++) {
    disp[p + k] = t[k].i0 >= 0 ? levels[t[k].i0] : 0.0f;
    if (conf) conf[p + k] = confidence(t[k]);
  }
}

// ---- winner-take-all + sub-level fit (b and parabola: ncc_sub.hip's header) -
__global__ __launch_bounds__(256) void k_wta_sub(const float* __restrict__ vol, const float* __restrict__ levels,
                                                 long P, int D, float* __restrict__ out) {
  const long p = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (p >= P) return;
  const float* col = vol + p;
  float best = __builtin_nontemporal_load(col);
  int b = 0;
#pragma unroll 8
  for (int dl = 1; dl < D; dl++) {
    const float c = __builtin_nontemporal_load(col + (long)dl * P);
    if (c < best) {
      best = c;
      b = dl;
    }
  }
  float r = levels[b];
  if (b > 0 && b < D - 1)
    r = parabola(col[(long)(b - 1) * P], best, col[(long)(b + 1) * P], levels[b - 1], r, levels[b + 1]);
  out[p] = r;
}

// ---- winner of an aggregate + the fit through the raw costs at that winner ---------------
// (include/mvs.h at mvs_wta_agg_sub_d).  k_wta<1, UNR>'s pass over agg, read once, with its Top4, its disp and its
// conf; then three raw costs and three levels are gathered from planes b-1, b, b+1.  The three plane indices
// are clamped into [0, D) before the loads, so every address lies inside vol and levels for every lane, b at an
// end and "no winner" (i0 < 0) included, and no lane-dependent condition stands between an address and its load;
// what must not count is dropped by the one select behind all six loads.  vol is addressed on its own: nothing
// of agg's alignment is assumed for it.
template <int UNR>
__global__ __launch_bounds__(256) void k_wta_agg_sub(const float* __restrict__ agg, const float* __restrict__ vol,
                                                     const float* __restrict__ levels, long P, int D,
                                                     float* __restrict__ disp, float* __restrict__ conf,
                                                     float* __restrict__ sub) {
  const long p = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (p >= P) return;
  Top4<float> t1[1];
  MVS_SCAN_TOP4(1, UNR, float, float, agg + p, P, D, kWtaInit, t1);
  const Top4<float>& t = t1[0];
  const int b = max(t.i0, 0), bm = max(b - 1, 0), bp = min(b + 1, D - 1);
  const float* rc = vol + p;
  const float cm = rc[(long)bm * P], c0 = rc[(long)b * P], cp = rc[(long)bp * P];
  const float lm = levels[bm], lb = levels[b], lp = levels[bp];
  if (disp) disp[p] = t.i0 >= 0 ? lb : 0.0f;
  if (conf) conf[p] = confidence(t);
  // raw has its minimum at b (mvs_wta_d's tie rule): den > 0, |off| <= 0.5
  const bool ok = b > 0 && b < D - 1 && cm > c0 && cp >= c0;
  const float fit = parabola(cm, c0, cp, lm, lb, lp);
  sub[p] = t.i0 < 0 ? 0.0f : ok ? fit : lb;
}

}  // namespace

int launch_wta(hipStream_t s, int W, int H, int D, const float* vol, const float* levels, float* disp,
               float* conf) {
  long P = (long)W * H;
  // one pixel per lane, 16 levels in flight (C2: 0.185 -> 0.182 ms against 8; 32 no faster;
  // wider per-lane vectors measured no faster)
  hipLaunchKernelGGL((k_wta<1, 16>), dim3((unsigned)((P + 255) / 256)), dim3(256), 0, s, vol, levels, P, D, disp,
                     conf);
  MVS_LAUNCH_CHECK("k_wta");
  return 0;
}

int launch_wta_sub(hipStream_t s, int W, int H, int D, const float* vol, const float* levels, float* disp_sub) {
  const long P = (long)W * H;
  hipLaunchKernelGGL(k_wta_sub, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, s, vol, levels, P, D, disp_sub);
  MVS_LAUNCH_CHECK("k_wta_sub");
  return 0;
}

int launch_wta_agg_sub(hipStream_t s, int W, int H, int D, const float* agg, const float* vol, const float* levels,
                       float* disp, float* conf, float* disp_sub) {
  const long P = (long)W * H;
  // launch_wta's form: one pixel per lane, 16 levels in flight
  hipLaunchKernelGGL(k_wta_agg_sub<16>, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, s, agg, vol, levels, P, D,
                     disp, conf, disp_sub);
  MVS_LAUNCH_CHECK("k_wta_agg_sub");
  return 0;
}

}  // namespace mvs
