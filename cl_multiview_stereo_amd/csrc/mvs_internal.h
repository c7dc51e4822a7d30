// Internal helpers shared by the HIP translation units of libmvs.so.
#pragma once

#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <cstdint>
#include <cstdio>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/mvs.h"
#include "../../include/mvs_detmath.h"
#include "launch_plan.h"  // map_dim, and what the SLIC / sweep / SAD / filter kernels share with their planners

struct mvs_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  // persistent scratch (grown on demand)
  void* scratch = nullptr;
  size_t scratch_bytes = 0;
  // device copy of the last mvs_array metadata
  float* d_levels = nullptr;
  int* d_vs = nullptr;
  int* d_sn = nullptr;
  size_t cap_levels = 0, cap_vs = 0, cap_sn = 0;
  std::vector<float> h_levels;
  std::vector<int> h_vs, h_sn;
  // small host-built launch plans (e.g. the NCC shift tables), uploaded once
  // per distinct content and kept for the life of the context
  std::map<std::vector<int32_t>, int32_t*> plans;
  // NCC sweep variant override (mvs_set_ncc_variant; 0 = automatic) and the
  // variant of the last launch {K, TH, DPW, NW, BW, PAR, FUSE, NB} (DPW 16: the matrix-core form)
  int ncc_nw = 0, ncc_dpw = 0, ncc_bw = 0, ncc_general = 0;
  int ncc_last[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  // the superpixel sweep's last launch {FORM, LPS, WPS, TMODE, RELAID}
  // (mvs_sweep_last_variant_n; FORM 0 general, 1 HZ gathers, 2 HZ ring, 3 re-laid)
  int sweep_last[5] = {0, 0, 0, 0, 0};
  // kernel timing (mvs_set_kernel_timing): the fused NCC sweep's launches carry
  // start / stop events of their own dispatch (hipExtLaunchKernel), pooled
  bool ktime = false;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> kev;
  size_t kev_used = 0;
};

namespace mvs {

// the next timed launch's event pair (null, null: timing off or no events)
inline std::pair<hipEvent_t, hipEvent_t> kernel_events(mvs_ctx* ctx) {
  if (!ctx->ktime) return {nullptr, nullptr};
  if (ctx->kev_used == ctx->kev.size()) {
    hipEvent_t a = nullptr, b = nullptr;
    if (hipEventCreate(&a) != hipSuccess) return {nullptr, nullptr};
    if (hipEventCreate(&b) != hipSuccess) {
      hipEventDestroy(a);
      return {nullptr, nullptr};
    }
    ctx->kev.push_back({a, b});
  }
  return ctx->kev[ctx->kev_used++];
}

// Raise kern's dynamic-LDS limit to lds bytes on ctx's device when above the
// 64 KB default.  HIP keeps the attribute per device, so the raise is cached
// per (kernel, device) -- a context on a second GPU raises it there too --
// under a mutex (contexts may launch from several host threads).
inline hipError_t raise_lds(mvs_ctx* ctx, const void* kern, size_t lds) {
  if (lds <= 64 * 1024) return hipSuccess;
  static std::mutex mu;
  static std::map<std::pair<const void*, int>, size_t> done;
  std::lock_guard<std::mutex> lock(mu);
  size_t& have = done[{kern, ctx->device}];
  if (lds <= have) return hipSuccess;
  const hipError_t e = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e == hipSuccess) have = lds;
  return e;
}

void set_error(const std::string& msg);
int hip_fail(hipError_t e, const char* what);
int arg_fail(const char* what);
void* scratch(mvs_ctx* ctx, size_t bytes, int* rc);
const int32_t* plan_upload(mvs_ctx* ctx, const std::vector<int32_t>& table, int* rc);

#define MVS_LAUNCH_CHECK(what)                          \
  do {                                                  \
    hipError_t _e = hipGetLastError();                  \
    if (_e != hipSuccess) return mvs::hip_fail(_e, what); \
  } while (0)

#define MVS_HIP(call, what)                              \
  do {                                                   \
    hipError_t _e = (call);                              \
    if (_e != hipSuccess) return mvs::hip_fail(_e, what); \
  } while (0)

// ---- launchers implemented in the .hip files (device pointers) ------------
int launch_cvt(hipStream_t s, const uint8_t* rgbx, long npix, float* lab, uint8_t* l8);
int launch_init_centers(hipStream_t s, const float* lab, int V, int W, int H, int S, float* spixl);
int launch_grid_labels(hipStream_t s, int V, int W, int H, int S, uint32_t* labels);

int launch_boundary(hipStream_t s, int V, int W, int H, int S, const float* spixl, const uint32_t* labels,
                    uint8_t* rep);
// launch_slic, launch_sweep_spixl, launch_sweep_pixel_sad and
// launch_remove_incons decide nothing themselves: launch_plan.cpp plans (the
// SLIC launch sequence, kernel form, grids, tables, LDS), they upload the
// tables and map the plan to a kernel instantiation
int launch_slic(mvs_ctx* ctx, const plan::SlicPlan& p, float weight, float* lab, float* spixl, uint32_t* labels,
                void* scratch);
int launch_sweep_spixl(mvs_ctx* ctx, int V, int W, int H, int S, const float* lab, float* spixl,
                       const uint8_t* rep, const float* levels, int D, const int* vs, const int* sn, int aw,
                       float bl, int z0, int z1);
int launch_sweep_pixel_sad(mvs_ctx* ctx, int V, int W, int H, const float* lab, const float* levels_host, int D,
                           const int* vs_host, const int* sn_host, int aw, float bl, int z0, int z1, float* disp);
int launch_box_stats(hipStream_t s, const uint8_t* l8, int V, int W, int H, int K, int32_t* box, int z0, int z1);
int launch_ncc_volume(mvs_ctx* ctx, int V, int W, int H, const int32_t* box, const float* levels_host, int D,
                      const int* vs_host, const int* sn_host, int aw, float bl, int K, int z, float* vol,
                      const float* levels_dev = nullptr, float* disp = nullptr, float* conf = nullptr);
int launch_ncc_refs(mvs_ctx* ctx, int V, int W, int H, const int32_t* box, const float* levels_host, int D,
                    const int* vs_host, const int* sn_host, int aw, float bl, int K, int z0, int z1, float* vol,
                    const float* levels_dev, float* disp, float* conf);
int launch_wta(hipStream_t s, int W, int H, int D, const float* vol, const float* levels, float* disp,
               float* conf);
// sub-level disparity: over a volume (wta.hip); for reference views [z0, z1) from the window planes (ncc_sub.hip)
int launch_wta_sub(hipStream_t s, int W, int H, int D, const float* vol, const float* levels, float* disp_sub);
int launch_ncc_sub(hipStream_t s, int V, int W, int H, const int32_t* box, const float* levels_dev, int D,
                   const int* vs_dev, const int* sn_dev, int aw, float bl, int K, int z0, int z1, const float* disp,
                   float* disp_sub);
// semi-global aggregation (sgm.hip): the set paths of `paths` (bits 0..7) in bit order, the first stores agg, the
// others add; N volumes per launch, element i at vol + i * vol_stride and agg + i * agg_stride (floats; the
// strides are not read at N = 1)
int launch_sgm(hipStream_t s, int W, int H, int D, int N, const float* vol, size_t vol_stride, float P1, float P2,
               int paths, float* agg, size_t agg_stride);
// the same on 16-bit integer costs (sgm16.hip; include/mvs.h at mvs_sgm8_u16_batch_d): D <= 256, strides in
// 2-byte elements, the sum over the set paths exact; the quantiser that makes such a volume and the winner pass
// that reads such an aggregate
int launch_sgm16(hipStream_t s, int W, int H, int D, int N, const uint16_t* vol, size_t vol_stride, int P1, int P2,
                 int paths, uint16_t* agg, size_t agg_stride);
int launch_quant_u16(hipStream_t s, size_t n, const float* src, uint16_t* dst);
int launch_wta_u16(hipStream_t s, int W, int H, int D, const uint16_t* agg, const float* levels, float* disp,
                   float* conf);
// the winner of an aggregate with the sub-level fit through the raw costs at that winner (include/mvs.h at
// mvs_wta_agg_sub_d: wta.hip; at mvs_wta_u16_sub_d: sgm16.hip); disp and conf may each be null
int launch_wta_agg_sub(hipStream_t s, int W, int H, int D, const float* agg, const float* vol, const float* levels,
                       float* disp, float* conf, float* disp_sub);
int launch_wta_u16_sub(hipStream_t s, int W, int H, int D, const uint16_t* agg, const uint16_t* raw,
                       const float* levels, float* disp, float* conf, float* disp_sub);

int launch_flatness(hipStream_t s, int V, int mw, int mh, const float* spixl, float gamma, float* flat);
// labels: uint32, or uint16 when lbits == 16 (16-bit gathered maps)
int launch_init_state(hipStream_t s, int V, int W, int H, int S, int aw, float bl, const float* spixl,
                      const void* labels, int lbits, const uint8_t* rep, const float* flat, const int* vs,
                      const int* sn, float gamma, float alpha, int nks, float kss, float fuse, float* state,
                      int z0, int z1);
int launch_propagate(hipStream_t s, int V, int W, int H, int S, int aw, float bl, const float* spixl,
                     const void* labels, int lbits, const uint8_t* rep, const float* flat, const int* vs,
                     const int* sn, int iter, float alpha, float gamma, float fuse, int nks, float kss,
                     const float* st_in, float* st_out, int z0, int z1,
                     int max_nbr);  // the largest neighbour count of views [z0, z1)
int launch_spixl_to_image(hipStream_t s, int V, int W, int H, int S, const float* spixl,
                          const void* labels, int lbits, const float* state, float* disp);
int launch_filter(hipStream_t s, int V, int W, int H, int aw, float bl, float fuse, const float* full,
                  float* proj, float* out, int z0, int z1);
int launch_proj_inv(hipStream_t s, int V, int W, int H, int aw, float bl, const float* full, float* proj, int z0,
                    int z1, int ya, int yb, bool band);
int launch_remove_incons(hipStream_t s, int V, int W, int H, int aw, float bl, float fuse, const float* full,
                         const float* proj, float* out, int z0, int z1, int ya, int yb, bool band);

}  // namespace mvs
