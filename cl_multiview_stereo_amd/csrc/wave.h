// Wave-level device helpers shared by the HIP units (no stage knowledge): short vector types, LDS-DMA
// pointer types, buffer descriptors, the vector-memory wait, the lane id and the exact round-half-away.
#pragma once
#include <hip/hip_runtime.h>

namespace mvs {

typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x3 __attribute__((ext_vector_type(3)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef int i32x4 __attribute__((ext_vector_type(4)));

// the destination and the source of an LDS-DMA
typedef __attribute__((address_space(3))) void* lds_ptr_t;
typedef const __attribute__((address_space(1))) void* gptr_t;
// 16-byte LDS-DMA: lane l's 16 bytes land at dst + 16*l (dst wave-uniform)
__device__ __forceinline__ void glds_b128(const void* src, void* dst) {
  __builtin_amdgcn_global_load_lds((gptr_t)src, (lds_ptr_t)dst, 16, 0, 0);
}

// The last word of a buffer descriptor: the value of the gfx9 raw-buffer recipe (ROCm's composable-kernel
// headers give this word for every gfx9 target).  Used here as: with stride 0 an access is addressed by
// its byte offset from the base and range-checked against the size in bytes -- a load past it returns 0,
// a store past it is dropped.
constexpr int kBufRsrcFlags = 0x00020000;
// the raw buffer of `bytes` bytes at base (0x7fffffff: no bound of its own)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t buf_rsrc(const void* base, int bytes) {
  return __builtin_amdgcn_make_buffer_rsrc((void*)base, 0, bytes, kBufRsrcFlags);
}

// s_waitcnt vmcnt(min(n, 6)) (n >= 0; a count above 6 waits for 6: still
// correct for a caller that needs at most n outstanding, only earlier)
__device__ __forceinline__ void wait_vm(int n) {
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

// the lane id, recomputed where it is used (volatile: never hoisted, so it is
// never a long-lived value the register allocator would spill)
__device__ __forceinline__ int lane_now() {
  int l;
  asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
  return l;
}

// roundf(v) as truncf(v + copysignf(0.49999997f, v)): equal for every non-NaN
// float (checked exhaustively over all 2^32 encodings, tests/test_oracle_cpu.py
// test_round_half_away_identity); 3 VALU instead of ~6.  NaN stays NaN.
__device__ __forceinline__ float round_ha(float v) {
  return truncf(v + copysignf(__int_as_float(0x3effffff), v));
}

}  // namespace mvs
