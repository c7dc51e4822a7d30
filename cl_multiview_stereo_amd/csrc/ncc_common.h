// Shared by the NCC kernels (ncc.hip: scalar forms and the window planes; ncc_mfma.hip: the matrix-core
// form; ncc_sub.hip and wta.hip: the sub-level fit): row-pair plane indexing, the band reads, the exact
// min / max / med3 helpers, the winner-take-all's initial cost and the fit.  Wave-level helpers: wave.h;
// the launch arguments and every host-side decision: ncc_plan.h.
#pragma once
#include <cstdint>
#include <vector>
#include "mvs_internal.h"
#include "ncc_plan.h"  // NccArgs, the parity modes, NccLaunch
#include "wave.h"

namespace mvs {
namespace ncc {

// Row-pair interleaved planes: element (y, x) of a view lives at uint2 index
// ((y >> 1) * W + x) * 2 + (y & 1), over Hp = H rounded up to even rows, so
// one 16-byte access returns rows 2m and 2m+1 of one column.
__host__ __device__ __forceinline__ long pair_index(int y, int x, int W) {
  return (((long)(y >> 1) * W + x) << 1) + (y & 1);
}

constexpr int kCPolNT = 2;  // buffer cache policy: non-temporal (CPol::NT on gfx940+)
// host-built plan (device memory, cached per context): one 128-B record per
// (chunk c, neighbour n, wave w), read with one scalar load per neighbour.
// A __restrict__ kernel parameter, so the loads are SMEM and never wait on
// the vector-memory counter the LDS-DMA prefetch runs under.
struct alignas(128) NccRec {
  int txmax, tymax;  // band origin: image column x0 - txmax; pk pair (y0-R-tymax)>>1, stats pair (y0-tymax)>>1
  int bhp, shp;      // pk pair rows to stage, stats pair rows | (64-px blocks per row) << 16
  int lv[16];        // per level j of wave w: {txmax - tx, pk start row | stats start row << 16 (band-relative)}
  int pad[12];
};
static_assert(sizeof(NccRec) == 4 * kRecWords, "the planner writes 32-word records");

// v_max_f32 (IEEE maxNum: a quiet-NaN operand is dropped).  Inline asm so the
// compiler does not re-canonicalise the loop-carried accumulators every pass.
__device__ __forceinline__ float vmax(float acc, float e) {
  float r;
  asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(acc), "v"(e));
  return r;
}
// max(-1, e) with -1.0 as an inline constant (no VGPR holding it)
__device__ __forceinline__ float vmax_m1(float e) {
  float r;
  asm("v_max_f32 %0, -1.0, %1" : "=v"(r) : "v"(e));
  return r;
}
__device__ __forceinline__ float vmin(float acc, float e) {
  float r;
  asm("v_min_f32 %0, %1, %2" : "=v"(r) : "v"(acc), "v"(e));
  return r;
}
__device__ __forceinline__ float vmin3(float a, float b, float c) {
  float r;
  asm("v_min3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
}
__device__ __forceinline__ unsigned vmin3u(unsigned a, unsigned b, unsigned c) {
  unsigned r;
  asm("v_min3_u32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
}
// the smallest of 16 as a tree of seven min3 and one min (v_min_f32's NaN rule: dropped)
__device__ __forceinline__ float vmin16(const float (&v)[16]) {
  const float a0 = vmin3(v[0], v[1], v[2]), a1 = vmin3(v[3], v[4], v[5]), a2 = vmin3(v[6], v[7], v[8]);
  const float a3 = vmin3(v[9], v[10], v[11]), a4 = vmin3(v[12], v[13], v[14]);
  return vmin(vmin3(a0, a1, a2), vmin3(a3, a4, v[15]));
}
__device__ __forceinline__ unsigned vmin16u(const unsigned (&v)[16]) {
  const unsigned a0 = vmin3u(v[0], v[1], v[2]), a1 = vmin3u(v[3], v[4], v[5]), a2 = vmin3u(v[6], v[7], v[8]);
  const unsigned a3 = vmin3u(v[9], v[10], v[11]), a4 = vmin3u(v[12], v[13], v[14]);
  return min(vmin3u(a0, a1, a2), vmin3u(a3, a4, v[15]));
}
// IEEE 754-2019 maximum of three (gfx950): NaN when any operand is NaN
__device__ __forceinline__ float vmaximum3(float a, float b, float c) {
  float r;
  asm("v_maximum3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
}
// median of three: with lo <= hi, med3(lo, hi, c) = min(hi, max(lo, c))
__device__ __forceinline__ float vmed3(float lo, float hi, float c) {
  float r;
  asm("v_med3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(lo), "v"(hi), "v"(c));
  return r;
}

// Fused winner-take-all outputs (k_ncc_volume<..., FUSE = true>): the volume
// is never written.  Same results as k_wta over the materialised volume.
struct WtaOut {
  const float* levels;  // device [D]
  float* disp;          // [H][W]
  float* conf;          // [H][W] or null
};
// the initial cost of the volume pass (k_wta's Top4, wta.hip) and of both fused folds
constexpr float kWtaInit = 1000000.0f;
// the sub-level fit (ncc_sub.hip's header); lm, lb, lp = levels[b-1], levels[b], levels[b+1]
__device__ __forceinline__ float parabola(float cm, float c0, float cp, float lm, float lb, float lp) {
  if (!(cm < 2.0f && cp < 2.0f)) return lb;
  const float den = (cm - c0) + (cp - c0);
  const float off = (0.5f * (cm - cp)) / den;
  const float step = off < 0.0f ? lb - lm : lp - lb;
  const float t = off * step;
  return lb + t;
}

// N consecutive band rows starting at band row r0 of a row-pair band (pair
// row stride BW, one column): ds_read_b128 per pair; an odd start takes the
// first and last rows as ds_read_b64 halves.  N even.
template <int N, int BW, int PAR>
__device__ __forceinline__ void read_rows(const u32x4* col, int r0, u32x2 (&v)[N]) {
  const u32x4* p = col + (r0 >> 1) * BW;
  if (PAR == kParEven || (PAR == kParMixed && (r0 & 1) == 0)) {
#pragma unroll
    for (int i = 0; i < N / 2; i++) {
      const u32x4 t = p[i * BW];
      v[2 * i] = t.xy;
      v[2 * i + 1] = t.zw;
    }
  } else {
    v[0] = ((const u32x2*)p)[1];
#pragma unroll
    for (int i = 1; i < N / 2; i++) {
      const u32x4 t = p[i * BW];
      v[2 * i - 1] = t.xy;
      v[2 * i] = t.zw;
    }
    v[N - 1] = ((const u32x2*)(p + (N / 2) * BW))[0];
  }
}

// The N/2 stats row pairs (o, o+1), o even, of a band column starting at band
// row r0: {a(o), a(o+1), b(o), b(o+1)}.  An odd start joins the second row of
// one stored pair with the first row of the next.
template <int N, int BW, int PAR>
__device__ __forceinline__ void read_stat_pairs(const u32x4* col, int r0, f32x4 (&v)[N / 2]) {
  const u32x4* p = col + (r0 >> 1) * BW;
  if (PAR != kParMixed || (r0 & 1) == 0) {
#pragma unroll
    for (int i = 0; i < N / 2; i++) v[i] = __builtin_bit_cast(f32x4, p[i * BW]);
  } else {
    // only the 16 needed dwords, as ds_read2_b32 pairs ({a, b} of one stored
    // row): no stored pair held whole, so the odd path needs no more registers
    // than the even one (the whole-pair form kept N/2 + 1 pairs live, and the
    // fused mixed-parity kernels spilled their fold accumulators for it)
    const float* f = (const float*)p;
#pragma unroll
    for (int i = 0; i < N / 2; i++) {
      const float* q0 = f + i * BW * 4;        // stored pair i: second rows (y, w)
      const float* q1 = f + (i + 1) * BW * 4;  // stored pair i + 1: first rows (x, z)
      v[i] = f32x4{q0[1], q1[0], q0[3], q1[2]};
    }
  }
}

constexpr int kMagicI = 0x4B400000;  // the bits of 12582912.0f = 1.5 * 2^23
constexpr float kMagicF = 12582912.0f;
// v_dot4_i32_i8 is the VOP3P form (separate destination): a prefix-sum chain
// keeps every partial sum without the accumulator copies the VOP2 v_dot4c
// form forces.  The Makefile builds the ncc*.hip files with the dot6 feature
// (v_dot4c) off, so the compiler selects the VOP3P form and still tracks its
// hazards.
__device__ __forceinline__ int dot4(unsigned a, unsigned b, int c) {
  return __builtin_amdgcn_sdot4((int)a, (int)b, c, false);
}

// One planned launch (ncc_plan.h) with its device pointers: ncc.hip and
// ncc_mfma.hip each map it to the kernel instantiation of its coordinates.
struct NccCall {
  mvs_ctx* ctx;
  const NccLaunch& L;
  const uint2 *stats, *pk;
  const int32_t* plan;  // L.table on the device
  float* vol;           // the cost volume, or null: the fused sweep into wo
  WtaOut wo;
};
inline int no_kernel() { return arg_fail("NCC sweep: no kernel instantiation for the planned launch"); }
int launch_ncc_mfma(const NccCall& c);  // the matrix-core family (ncc_mfma.hip)

}  // namespace ncc
}  // namespace mvs
