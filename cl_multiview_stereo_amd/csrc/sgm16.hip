// Semi-global aggregation on 16-bit integer costs (include/mvs.h at mvs_quant_u16_d, mvs_sgm8_u16_batch_d,
// mvs_wta_u16_d and mvs_wta_u16_sub_d; tests/sgm16_ref.py): the uint16 instantiation of sgm_kernels.h at
// D <= kSgm16MaxD (the lanes form with one wave and 1, 2 or 4 levels per lane for the horizontal paths, the
// columns form for the vertical ones, the sheared form for the diagonal ones), and the streaming passes before and
// behind.  k_quant_u16: float32 costs -> uint16.  k_wta_u16: the winner with its confidence from a uint16
// aggregate.  k_wta_u16_sub: that winner pass with the sub-level fit through the raw (quantised, not aggregated)
// costs at the winner.
#include "sgm_kernels.h"
#include "wta_common.h"

namespace mvs {
namespace {

// ---- float32 costs -> uint16 ------------------------------------------------------------------
// q = rint_to_even(min(max(v, 0), 2) * 2047): one rounded multiply, v_rndne
__device__ __forceinline__ unsigned quant1(float v) {
  return (unsigned)(int)rintf(fminf(fmaxf(v, 0.0f), 2.0f) * 2047.0f);
}

// Elements [0, h) bring dst to a 16-byte boundary; thread t < G then takes the eight elements from h + 8 t (one
// 16-byte store; two 16-byte loads where src + h is 16-byte aligned as well, SV, else eight 4-byte loads); the
// head and the tail behind h + 8 G, under eight elements each, go one by one on the first 16 threads.
template <bool SV>
__global__ __launch_bounds__(256) void k_quant_u16(const float* __restrict__ src, uint16_t* __restrict__ dst, size_t n,
                                                   int h, size_t G) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (t < G) {
    const float* s = src + h + 8 * t;
    float v[8];
    if (SV) {
      const f32x4 lo = __builtin_nontemporal_load((const f32x4*)s), hi = __builtin_nontemporal_load((const f32x4*)s + 1);
#pragma unroll
      for (int k = 0; k < 4; k++) {
        v[k] = lo[k];
        v[4 + k] = hi[k];
      }
    } else {
#pragma unroll
      for (int k = 0; k < 8; k++) v[k] = s[k];
    }
    u32x4 o;
#pragma unroll
    for (int k = 0; k < 4; k++) o[k] = quant1(v[2 * k]) | (quant1(v[2 * k + 1]) << 16);
    *(u32x4*)(dst + h + 8 * t) = o;
  }
  if (t < 16) {
    const size_t e = t < 8 ? t : (size_t)h + 8 * G + (t - 8);
    if (t < 8 ? (int)t < h : e < n) dst[e] = (uint16_t)quant1(src[e]);
  }
}

// ---- winner and confidence of a uint16 aggregate ------------------------------------------------
// Top4 from kInf: the smallest cost at a level more than one away from the winner's is among the other three
__device__ __forceinline__ float confidence(const Top4<int>& t) {
  const int c2 = t.second(-1);
  return c2 < 0 ? 0.0f : (float)(c2 - t.v0) / 2047.0f;
}

// One lane per NP consecutive pixels, UNR levels in flight.  NP = 4 (8-byte loads) needs the plane pitch P a
// multiple of 4 and agg 8-byte aligned; NP = 1 takes everything else.
template <int NP, int UNR>
__global__ __launch_bounds__(256) void k_wta_u16(const uint16_t* __restrict__ agg, const float* __restrict__ levels,
                                                 long P, int D, float* __restrict__ disp, float* __restrict__ conf) {
  const long p = (blockIdx.x * (long)blockDim.x + threadIdx.x) * NP;
  if (p >= P) return;
  Top4<int> t[NP];
  MVS_SCAN_TOP4(NP, UNR, uint16_t, int, agg + p, P, D, kInf, t);
  // conf first, as k_wta_u16_sub: behind disp it cost the four-pixel form 24 instructions and 0.6 us at 1080p
  if (conf) {
#pragma unroll
    for (int k = 0; k < NP; k++) conf[p + k] = confidence(t[k]);
  }
#pragma unroll
  for (int k = 0; k < NP; k++) disp[p + k] = levels[t[k].i0];  // (D >= 1 and every cost is below kInf: i0 >= 0)
}

// ---- winner of a uint16 aggregate + the fit through the raw costs at that winner ----------------
// (include/mvs.h at mvs_wta_u16_sub_d).  k_wta_u16's pass over agg, read once, in both of its forms; then every
// pixel gathers three raw costs and three levels from planes b-1, b, b+1.  The plane indices are clamped into
// [0, D) before the loads (b at an end: the index, not a branch), so every address lies inside raw and levels and
// no lane-dependent condition stands between an address and its load; the one select sits behind all of a lane's
// loads.  raw goes by 2-byte loads in the four-pixel form as well: its alignment is its own.
template <int NP, int UNR>
__global__ __launch_bounds__(256) void k_wta_u16_sub(const uint16_t* __restrict__ agg, const uint16_t* __restrict__ raw,
                                                     const float* __restrict__ levels, long P, int D,
                                                     float* __restrict__ disp, float* __restrict__ conf,
                                                     float* __restrict__ sub) {
  const long p = (blockIdx.x * (long)blockDim.x + threadIdx.x) * NP;
  if (p >= P) return;
  Top4<int> t[NP];
  MVS_SCAN_TOP4(NP, UNR, uint16_t, int, agg + p, P, D, kInf, t);
  // conf first: from here on only the winners' indices stay live beside the gathered values
  if (conf) {
#pragma unroll
    for (int k = 0; k < NP; k++) conf[p + k] = confidence(t[k]);
  }
  int b[NP], rm[NP], r0[NP], rp[NP];
  float lm[NP], lb[NP], lp[NP];
#pragma unroll
  for (int k = 0; k < NP; k++) {  // (D >= 1 and every cost is below kInf: i0 >= 0; the clamp keeps that off the address)
    b[k] = min(max(t[k].i0, 0), D - 1);
    const int bm = max(b[k] - 1, 0), bp = min(b[k] + 1, D - 1);
    const uint16_t* rc = raw + p + k;
    rm[k] = (int)rc[(long)bm * P];
    r0[k] = (int)rc[(long)b[k] * P];
    rp[k] = (int)rc[(long)bp * P];
    lm[k] = levels[bm];
    lb[k] = levels[b[k]];
    lp[k] = levels[bp];
  }
#pragma unroll
  for (int k = 0; k < NP; k++) {
    if (disp) disp[p + k] = lb[k];
    // both sides measured (4094: no valid window) and raw has its minimum at b (mvs_wta_d's tie rule): den >= 1
    const bool ok = b[k] > 0 && b[k] < D - 1 && rm[k] < 4094 && rp[k] < 4094 && rm[k] > r0[k] && rp[k] >= r0[k];
    const int den = (rm[k] - r0[k]) + (rp[k] - r0[k]);
    const float off = (float)(rm[k] - rp[k]) / (float)(2 * den);
    const float step = off < 0.0f ? lb[k] - lm[k] : lp[k] - lb[k];
    const float prod = off * step;
    sub[p + k] = ok ? lb[k] + prod : lb[k];
  }
}

}  // namespace

int launch_sgm16(hipStream_t s, int W, int H, int D, int N, const uint16_t* vol, size_t vol_stride, int P1, int P2,
                 int paths, uint16_t* agg, size_t agg_stride) {
  if (D > plan::kSgm16MaxD) return arg_fail("sgm16: more than 256 levels");
  return launch_sgm_paths<SgmU16, false>(s, W, H, D, N, vol, vol_stride, P1, P2, paths, agg, agg_stride, "k_sgm16",
                                         "sgm16: no kernel form for this plan");
}

int launch_quant_u16(hipStream_t s, size_t n, const float* src, uint16_t* dst) {
  const size_t kChunk = (size_t)1 << 33;  // elements per launch: 2^22 workgroups, one grid axis
  while (n > 0) {
    const size_t nc = n < kChunk ? n : kChunk;
    const size_t head = ((16 - ((uintptr_t)dst & 15)) & 15) / 2;
    const int h = (int)(head < nc ? head : nc);
    const size_t G = (nc - h) / 8;
    const unsigned grid = (unsigned)(G ? (G + 255) / 256 : 1);
    if (((uintptr_t)(src + h) & 15) == 0)
      hipLaunchKernelGGL(k_quant_u16<true>, dim3(grid), dim3(256), 0, s, src, dst, nc, h, G);
    else
      hipLaunchKernelGGL(k_quant_u16<false>, dim3(grid), dim3(256), 0, s, src, dst, nc, h, G);
    MVS_LAUNCH_CHECK("k_quant_u16");
    n -= nc;
    src += nc;
    dst += nc;
  }
  return 0;
}

int launch_wta_u16(hipStream_t s, int W, int H, int D, const uint16_t* agg, const float* levels, float* disp,
                   float* conf) {
  const long P = (long)W * H;
  if (P % 4 == 0 && ((uintptr_t)agg & 7) == 0)
    hipLaunchKernelGGL((k_wta_u16<4, 8>), dim3((unsigned)((P / 4 + 255) / 256)), dim3(256), 0, s, agg, levels, P, D,
                       disp, conf);
  else
    hipLaunchKernelGGL((k_wta_u16<1, 16>), dim3((unsigned)((P + 255) / 256)), dim3(256), 0, s, agg, levels, P, D, disp,
                       conf);
  MVS_LAUNCH_CHECK("k_wta_u16");
  return 0;
}

int launch_wta_u16_sub(hipStream_t s, int W, int H, int D, const uint16_t* agg, const uint16_t* raw,
                       const float* levels, float* disp, float* conf, float* disp_sub) {
  const long P = (long)W * H;
  // launch_wta_u16's choice, from agg alone
  if (P % 4 == 0 && ((uintptr_t)agg & 7) == 0)
    hipLaunchKernelGGL((k_wta_u16_sub<4, 8>), dim3((unsigned)((P / 4 + 255) / 256)), dim3(256), 0, s, agg, raw, levels,
                       P, D, disp, conf, disp_sub);
  else
    hipLaunchKernelGGL((k_wta_u16_sub<1, 16>), dim3((unsigned)((P + 255) / 256)), dim3(256), 0, s, agg, raw, levels, P,
                       D, disp, conf, disp_sub);
  MVS_LAUNCH_CHECK("k_wta_u16_sub");
  return 0;
}

}  // namespace mvs
