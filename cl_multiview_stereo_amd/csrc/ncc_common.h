// Shared by the NCC sweep kernels (ncc.hip: scalar forms and the window
// planes; ncc_mfma.hip: the matrix-core form): row-pair plane indexing, the
// LDS-DMA and the exact min / max / med3 helpers.  The launch arguments and
// every host-side decision are ncc_plan.h's.
#pragma once
#include <cstdint>
#include <vector>
#include "mvs_internal.h"
#include "ncc_plan.h"  // NccArgs, the parity modes, NccLaunch

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

typedef __attribute__((address_space(3))) void* lds_ptr_t;
typedef const __attribute__((address_space(1))) void* gptr_t;
// 16-byte LDS-DMA: lane l's 16 bytes land at dst + 16*l (dst wave-uniform)
__device__ __forceinline__ void glds_b128(const void* src, void* dst) {
  __builtin_amdgcn_global_load_lds((gptr_t)src, (lds_ptr_t)dst, 16, 0, 0);
}

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
constexpr float kWtaInit = 1000000.0f;  // k_wta's Top4 initial cost (sweep.hip)

typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

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

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

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

// v_dot4_i32_i8 is the VOP3P form (separate destination): a prefix-sum chain
// keeps every partial sum without the accumulator copies the VOP2 v_dot4c
// form forces.  The Makefile builds this file with the dot6 feature (v_dot4c)
// off, so the compiler selects the VOP3P form and still tracks its hazards.
// s_waitcnt vmcnt(min(n, 6)) (n >= 0; a count above 6 waits for 6: still
// correct for a caller that needs at most n outstanding, only earlier)
__device__ __forceinline__ void wait_vm_le(int n) {
  switch (n) {
    case 0: __builtin_amdgcn_s_waitcnt(0x0f70); break;
    case 1: __builtin_amdgcn_s_waitcnt(0x0f71); break;
    case 2: __builtin_amdgcn_s_waitcnt(0x0f72); break;
    case 3: __builtin_amdgcn_s_waitcnt(0x0f73); break;
    case 4: __builtin_amdgcn_s_waitcnt(0x0f74); break;
    case 5: __builtin_amdgcn_s_waitcnt(0x0f75); break;
    default: __builtin_amdgcn_s_waitcnt(0x0f76); break;
  }
}

// s_waitcnt vmcnt(n) for a wave-uniform n in [0, 6] (n > 6: vmcnt(6)), then
// s_barrier -- the selection inside one asm block, so the compiler sees no
// branch (a C-level switch split the step and spilled the fold's registers)
__device__ __forceinline__ void wait_vm_barrier(int n) {
  asm volatile(
      "s_cmp_eq_u32 %0, 0\n\ts_cbranch_scc1 10f\n\t"
      "s_cmp_eq_u32 %0, 1\n\ts_cbranch_scc1 11f\n\t"
      "s_cmp_eq_u32 %0, 2\n\ts_cbranch_scc1 12f\n\t"
      "s_cmp_eq_u32 %0, 3\n\ts_cbranch_scc1 13f\n\t"
      "s_cmp_eq_u32 %0, 4\n\ts_cbranch_scc1 14f\n\t"
      "s_cmp_eq_u32 %0, 5\n\ts_cbranch_scc1 15f\n\t"
      "s_waitcnt vmcnt(6)\n\ts_branch 19f\n"
      "10:\n\ts_waitcnt vmcnt(0)\n\ts_branch 19f\n"
      "11:\n\ts_waitcnt vmcnt(1)\n\ts_branch 19f\n"
      "12:\n\ts_waitcnt vmcnt(2)\n\ts_branch 19f\n"
      "13:\n\ts_waitcnt vmcnt(3)\n\ts_branch 19f\n"
      "14:\n\ts_waitcnt vmcnt(4)\n\ts_branch 19f\n"
      "15:\n\ts_waitcnt vmcnt(5)\n"
      "19:\n\ts_barrier"
      :
      : "s"(n)
      : "memory", "scc");
}

// the lane id, recomputed where it is used (volatile: never hoisted, so it is
// never a long-lived value the register allocator would spill)
__device__ __forceinline__ int lane_now() {
  int l;
  asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
  return l;
}

constexpr int kMagicI = 0x4B400000;  // the bits of 12582912.0f = 1.5 * 2^23
constexpr float kMagicF = 12582912.0f;
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
