// Photo-consistency plane-sweep kernels of the superpixel stage for gfx950 (CDNA4, wave64).
//
//  k_boundary        find_super_pixel_boundary           clcode.cl:791-855
//  k_sweep_spixl     initial_depth_estimation_v2          clcode.cl:972-1069
//                    (one wave per superpixel, lanes over hypotheses,
//                    exact first-minimum WTA by a (cost, index) wave reduction)
//  k_sweep_spixl_ring  the same sweep for horizontal arrays, from rows staged in LDS
//  k_relayout_lab    neighbour views transposed / sheared for k_sweep_spixl's gathers
//  (per-pixel SAD sweep: sad.hip; NCC cost volume: ncc.hip; its winner-take-all: wta.hip)
#include <algorithm>
#include <type_traits>

#include "mvs_internal.h"
#include "wave.h"

namespace mvs {
namespace {

// ---- find_super_pixel_boundary, clcode.cl:791-855 -------------------------
// One wave per superpixel.  The reference walks i = 1 .. S-1 along 8
// directions from the (clamped) centre and keeps, per direction, i - 1 of the
// last i whose pixel still carries the superpixel's label: a maximum over
// independent tests.  Lane 8k + j tests direction k at i = 1 + j + 8m, so the
// 8 (S - 1) label gathers issue together instead of as one thread's chain
// (C2: 30 -> see DESIGN.md), and an xor-butterfly takes each direction's
// maximum.  Integer results: identical.
__global__ __launch_bounds__(256) void k_boundary(const float* __restrict__ spixl,
                                                  const uint32_t* __restrict__ labels, int W, int H, int S, int mw,
                                                  int mh, uint8_t* __restrict__ rep) {
  const int lane = threadIdx.x & 63;
  const long s = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int z = blockIdx.y;
  const long M = (long)mw * mh, P = (long)W * H;
  if (s >= M) return;  // whole wave
  const float* sp = spixl + 8 * (z * M + s);
  int cx = (int)sp[1], cy = (int)sp[2];
  if (cx < S) cx += (S - cx);
  if (cx + S > W) cx -= S;
  if (cy < S) cy += (S - cy);
  if (cy + S > H) cy -= S;
  const uint32_t id = (uint32_t)s;
  const uint32_t* L = labels + z * P;
  const int k = lane >> 3, j = lane & 7;
  // direction k: (dx, dy) in the reference's order d0 .. d7
  const int dx = k < 3 ? -1 : (k < 5 ? 0 : 1);
  const int dy = (k == 0 || k == 3 || k == 5) ? -1 : ((k == 1 || k == 6) ? 0 : 1);
  int d = 0;
  for (int i0 = 1; i0 < S; i0 += 32) {
    uint32_t v[4];
    bool in[4];
#pragma unroll
    for (int m = 0; m < 4; m++) {  // unconditional (clamped) loads: all four in flight together
      const int i = i0 + j + 8 * m, xx = cx + dx * i, yy = cy + dy * i;
      in[m] = i < S && xx >= 0 && xx < W && yy >= 0 && yy < H;
      v[m] = L[in[m] ? (long)yy * W + xx : 0];
    }
#pragma unroll
    for (int m = 0; m < 4; m++)
      if (in[m] && v[m] == id) d = i0 + j + 8 * m - 1;  // i grows: the last hit is the largest
  }
  d = max(d, __shfl_xor(d, 1));
  d = max(d, __shfl_xor(d, 2));
  d = max(d, __shfl_xor(d, 4));
  uint32_t w = (uint32_t)(d & 0xff) << (8 * (k & 3));
  w |= __shfl_xor(w, 8);
  w |= __shfl_xor(w, 16);  // lane 0: directions 0-3, lane 32: directions 4-7
  const uint32_t hi = __shfl(w, 32);
  if (lane == 0) *(uint2*)(rep + 8 * (z * M + s)) = make_uint2(w, hi);
}

// ---- initial_depth_estimation_v2, clcode.cl:972-1069 ----------------------
// (SweepArgs and SB_INIT, the initial cost: launch_plan.h, shared with sad.hip)
// One workgroup = 4 waves; each superpixel is shared by wps waves (wps =
// ceil(D/64) up to 4), wave h taking levels lane + 64 (h + wps p), and all
// reference views of the call run in one launch (blockIdx.y), so the GPU is
// filled even at a few thousand superpixels per view.  The per-wave first
// minima are combined in (cost, index) lexicographic order -- the reference's
// strict-< scan over levels in index order -- through LDS.  LPS = 32 (D <= 32,
// e.g. the reference's default 31 levels): two superpixels per wave, one per
// 32-lane half, so no lane idles past the last level.
// Vertical and diagonal neighbours: lane = level puts 64 levels' taps on 64
// different rows -- 64 cache lines per gather instruction, 16 B used of each
// 128 (measured at C4, 8x4 array, 5 nearest neighbours, all 32 views:
// TCC_MISS 271 M per launch against 175 M hits, 4.66 ms).  labT (optional)
// holds such neighbour views re-laid so that consecutive levels' taps are
// consecutive elements: at labT + tslot[4 * view + kind] * tstride
// of kind 1 (same camera column: transposed, element (x, y) at x H + y),
// 2 (dx == dy: sheared, at (x - y + H - 1) H + y) or 3 (dx == -dy: at
// (x + y) H + y).  With bl != 1 the diagonal shifts drift apart by a row
// every 1/|bl - 1| levels: still a few lines per instruction instead of 64.
// TL = false (no re-laid views in this call, e.g. a horizontal array): the
// row-major addressing folds to yp W + xp at compile time -- the general
// form's extra multiply-add per tap cost C2 (5x1 array) 173 -> 224 us.
// HZ (every neighbour of the launch's references in the same camera row, every
// level x column offset an integer below 2^24, no re-laid views): the shift
// is an integer, so (int)((float)xr - d dx) = xr - (int)(d dx) exactly, the
// tap's row yr = (int)(r.y - 0) is the reference tap's own (inside the image
// whenever the reference tap is) and its offset yr W is stored with the tap.
// A tap then costs one integer subtract, one compare and one shift-add before
// its gather, and the gather needs no select: the view's buffer resource
// bounds every offset (a tap outside the image reads some pixel of the view,
// or 0, and is dropped as before).  The absolute differences and the
// reference's val += 30; val -= 30; val += AD are single-issue asm, as the
// compiler's SLP pairing put them in v_pk_add_f32 with the |.| as separate
// v_and_b32.  C2: see DESIGN.md section 3.
__device__ __forceinline__ float tap_ad(const float4& A, const u32x3& bv) {
  float t0, t1, t2, r;
  asm("v_sub_f32 %0, %1, %2" : "=v"(t0) : "v"(A.x), "v"(__uint_as_float(bv.x)));
  asm("v_sub_f32 %0, %1, %2" : "=v"(t1) : "v"(A.y), "v"(__uint_as_float(bv.y)));
  asm("v_add_f32 %0, |%1|, |%2|" : "=v"(r) : "v"(t0), "v"(t1));  // fabsf(dL) + fabsf(da)
  asm("v_sub_f32 %0, %1, %2" : "=v"(t2) : "v"(A.z), "v"(__uint_as_float(bv.z)));
  asm("v_add_f32 %0, %1, |%2|" : "=v"(r) : "v"(r), "v"(t2));  // + fabsf(db)
  return r;
}
// val = in ? ((val + 30) - 30) + ad : val + 30
__device__ __forceinline__ float tap_acc(float val, float ad, bool in) {
  float v30, t;
  asm("v_add_f32 %0, 0x41f00000, %1" : "=v"(v30) : "v"(val));
  asm("v_add_f32 %0, 0xc1f00000, %1" : "=v"(t) : "v"(v30));
  asm("v_add_f32 %0, %1, %2" : "=v"(t) : "v"(t), "v"(ad));
  return in ? t : v30;
}
template <int LPS, bool TL, bool HZ = false>
__global__ __launch_bounds__(256) void k_sweep_spixl(const float4* __restrict__ lab, float* __restrict__ spixl,
                                                     const uint8_t* __restrict__ rep,
                                                     const float* __restrict__ levels, const int* __restrict__ vs,
                                                     const int* __restrict__ sn, SweepArgs a, int wps,
                                                     const float4* __restrict__ labT,
                                                     const int* __restrict__ tslot, long tstride) {
  __shared__ float4 refc[8][25];
  __shared__ float2 refxy[8][25];  // (float)xr, (float)yr; xr = -1e9 for a tap outside the image
                                   // (HZ: int xr (-2^30 outside), int yr W)
  __shared__ float wbest[4];
  __shared__ int wbi[4];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int ll = lane & (LPS - 1);                              // level lane within the superpixel's lanes
  const int spb = LPS == 64 ? 4 / wps : 8, h = LPS == 64 ? w % wps : 0;
  const int slot = LPS == 64 ? w / wps : 2 * w + (lane >> 5);  // superpixel of this block
  const int z = a.z + blockIdx.y;
  const long M = (long)a.mw * a.mh, P = (long)a.W * a.H;
  // XCD-aware order: blocks are dealt round-robin over the 8 XCDs; give each
  // XCD a contiguous run of superpixels so the neighbour rows its gathers
  // touch are shared within one L2 instead of being fetched by all eight
  const long nb = (M + spb - 1) / spb, per = (nb + 7) / 8;
  const long blk = (long)(blockIdx.x & 7) * per + (blockIdx.x >> 3);
  const long s = blk * spb + slot;
  const bool active = blk < nb && s < M && slot < spb;
  const long idx = z * M + (active ? s : 0);
  const uint8_t* dr = rep + 8 * idx;
  int bl_ = max((int)dr[0], max((int)dr[1], (int)dr[2]));
  int br_ = max((int)dr[5], max((int)dr[6], (int)dr[7]));
  int bt_ = max((int)dr[0], max((int)dr[3], (int)dr[5]));
  int bb_ = max((int)dr[2], max((int)dr[4], (int)dr[7]));
  float stx = (float)fmax(1.0, 0.25 * (double)(float)(bl_ + br_));
  float sty = (float)fmax(1.0, 0.25 * (double)(float)(bt_ + bb_));
  float cx = spixl[8 * idx + 1], cy = spixl[8 * idx + 2];
  const float4* labz = lab + (long)z * P;
  if (ll < 25 && (LPS == 32 || h == 0)) {
    int i = ll / 5 - 2, j = ll % 5 - 2;  // tap order: i (x) outer, j (y) inner
    int xr = (int)(cx + (float)i * stx);
    int yr = (int)(cy + (float)j * sty);
    bool in = xr >= 0 && yr >= 0 && xr < a.W && yr < a.H;
    // (float)xr is exact; an outside reference tap projects outside too
    if (HZ)
      refxy[slot][ll] = make_float2(__int_as_float(in ? xr : -(1 << 30)), __int_as_float(in ? yr * a.W : 0));
    else
      refxy[slot][ll] = make_float2(in ? (float)xr : -1.0e9f, (float)yr);
    refc[slot][ll] = in ? labz[(long)yr * a.W + xr] : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  __syncthreads();
  int rx = z % a.aw, ry = z / a.aw;
  int nn = sn[z];
  float best = SB_INIT;
  int bi = 0x7fffffff;
  for (int dl = ll + LPS * h; dl < a.D; dl += LPS * wps) {
    float d = levels[dl];
    float mn = SB_INIT;
    for (int n = 0; n < nn; n++) {
      int view = vs[a.V * z + n];
      int vx = view % a.aw, vy = view / a.aw;
      float fdx = d * (float)(vx - rx);
      float fdy = (a.bl * d) * (float)(vy - ry);
      const int ddx = vx - rx, ddy = vy - ry;
      if (HZ) {
        const int sh = (int)fdx;  // exact (the launcher checked the levels)
        const __amdgpu_buffer_rsrc_t rs = buf_rsrc(lab + (long)view * P, (int)(P * 16));
        float val = 0.0f;
#pragma unroll 5
        for (int t = 0; t < 25; t++) {
          const float2 rf = refxy[slot][t];
          const int xp = __float_as_int(rf.x) - sh;
          const bool in = (unsigned)xp < (unsigned)a.W;
          const unsigned bo = (unsigned)(__float_as_int(rf.y) + xp) << 4;
          const u32x3 bv = __builtin_amdgcn_raw_buffer_load_b96(rs, (int)bo, 0, 0);
          val = tap_acc(val, tap_ad(refc[slot][t], bv), in);
        }
        if (val < mn) mn = val;
        continue;
      }
      const int kind = !TL ? 0 : ddx == 0 ? 1 : ddx == ddy ? 2 : ddx == -ddy ? 3 : 0;
      const int ts = TL && kind ? tslot[4 * view + kind] : -1;
      const float4* labv = TL && ts >= 0 ? labT + (long)ts * tstride : lab + (long)view * P;
      // 32-bit byte offsets into the view's layout (the launcher checks the
      // size): one address add per tap instead of 64-bit index arithmetic
      const __amdgpu_buffer_rsrc_t rs = buf_rsrc(labv, 0x7fffffff);
      // element index = off + x sxs + y sys in the view's layout
      const int sxs = !TL || ts < 0 ? 1 : a.H;
      const int sys = !TL || ts < 0 ? a.W : kind == 1 ? 1 : kind == 2 ? 1 - a.H : a.H + 1;
      const int off = TL && ts >= 0 && kind == 2 ? (a.H - 1) * a.H : 0;
      float val = 0.0f;
      // branch-free taps: every load is issued (out-of-image taps read pixel 0
      // and are dropped by the select), so the 25 gathers of a neighbour are
      // independent and in flight together instead of one per branch
#pragma unroll 5
      for (int t = 0; t < 25; t++) {
        const float2 r = refxy[slot][t];
        const int xp = (int)(r.x - fdx);
        const int yp = (int)(r.y - fdy);
        const bool in = (unsigned)xp < (unsigned)a.W && (unsigned)yp < (unsigned)a.H;
        const int bo = in ? (off + yp * sys + xp * sxs) * 16 : 0;  // an outside tap reads pixel 0, dropped below
        const u32x3 bv = __builtin_amdgcn_raw_buffer_load_b96(rs, bo, 0, 0);
        const float3 B = make_float3(__uint_as_float(bv.x), __uint_as_float(bv.y), __uint_as_float(bv.z));
        const float4 A = refc[slot][t];
        float ad = fabsf(A.x - B.x) + fabsf(A.y - B.y);
        ad = ad + fabsf(A.z - B.z);
        const float v30 = val + 30.0f;  // the reference's val += 30; val -= 30; val += AD
        val = in ? (v30 - 30.0f) + ad : v30;
      }
      if (val < mn) mn = val;
    }
    if (mn < best) {
      best = mn;
      bi = dl;
    }
  }
  // first minimum across the superpixel's lanes: (cost, index) lexicographic
#pragma unroll
  for (int o = LPS / 2; o >= 1; o >>= 1) {
    float ob = __shfl_xor(best, o, 64);
    int oi = __shfl_xor(bi, o, 64);
    if (ob < best || (ob == best && oi < bi)) {
      best = ob;
      bi = oi;
    }
  }
  if (LPS == 32) {
    if (active && ll == 0) spixl[8 * idx + 7] = (bi != 0x7fffffff && best < SB_INIT) ? levels[bi] : 0.0f;
    return;
  }
  if (lane == 0) {
    wbest[w] = best;
    wbi[w] = bi;
  }
  __syncthreads();
  if (active && h == 0 && lane == 0) {
    for (int k = 1; k < wps; k++) {
      const float ob = wbest[w + k];
      const int oi = wbi[w + k];
      if (ob < best || (ob == best && oi < bi)) {
        best = ob;
        bi = oi;
      }
    }
    spixl[8 * idx + 7] = (bi != 0x7fffffff && best < SB_INIT) ? levels[bi] : 0.0f;
  }
}

// ---- the HZ sweep from LDS-staged rows (k_sweep_spixl_ring) ---------------
// The HZ gather form is texture-address-bound, not VALU-bound (C2, PMC: TA
// busy 74 % of the kernel, ~15 L2 requests per 64-lane gather: the 64 levels
// of one tap hit 64 pixels dx apart, a partial line each, and the 5 taps of a
// row re-read the same pixels at other levels).  Here a wave (64 levels of
// one superpixel) stages, per neighbour and tap row, the union of the columns
// its 5 taps reach at its 64 levels -- [min xr - max sh, max xr - min sh],
// clamped to the image, at most kSwU columns -- into LDS by whole-line
// LDS-DMA (one 1 KiB piece per 64 columns), and reads every tap from there.
// Rows go through a two-slot ring per wave: row k+2 is staged while row k+1
// lands and row k is computed (s_waitcnt vmcnt(pieces of row k+1) before
// row k); no barrier, the ring is the wave's own.  A tap's absolute
// differences are k_sweep_spixl's; its out-of-image flag rides as ad = -1
// (ad >= 0 otherwise), and the reference's val += 30; val -= 30; val += AD
// chain runs in tap order (i outer, j inner) once the neighbour's 25 taps
// are in.  The launcher takes this form only when every window fits kSwU
// columns: 2 (S - 1) + 2 + |dx| x the levels' range over any 64 consecutive
// levels (stx <= (S - 1) / 2), else the HZ gathers.
// (kSwU: launch_plan.h, shared with the planner)
// What a (pass, neighbour) fixes is set up once for its five rows: the
// window, the lane's shift and the staging source -- the neighbour view's
// plane as a buffer, so a row's piece is a scalar offset beside one lane
// offset.  Where all 25 reference taps are inside and the window is whole
// (no lane's tap column leaves the image: a scalar test on the window's
// ends), the whole-window path runs: five tap addresses per lane for the
// neighbour, no clamp, no outside marker, three adds per tap in the chain.
// Every other (pass, neighbour) takes the general row-steps, and fast = 0
// (MVS_SWEEP_RING_FAST=0) sends all of them there.
__device__ __forceinline__ float wave_min_f(float v) {
  v = fminf(v, __shfl_xor(v, 32));
  v = fminf(v, __shfl_xor(v, 16));
  v = fminf(v, __shfl_xor(v, 8));
  v = fminf(v, __shfl_xor(v, 4));
  v = fminf(v, __shfl_xor(v, 2));
  v = fminf(v, __shfl_xor(v, 1));
  return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v)));
}
// tap_acc for a tap known to be inside: val = ((val + 30) - 30) + ad
__device__ __forceinline__ float tap_acc_in(float val, float ad) {
  float t;
  asm("v_add_f32 %0, 0x41f00000, %1" : "=v"(t) : "v"(val));
  asm("v_add_f32 %0, 0xc1f00000, %1" : "=v"(t) : "v"(t));
  asm("v_add_f32 %0, %1, %2" : "=v"(t) : "v"(t), "v"(ad));
  return t;
}
// a row's 5 taps from the ring slot at byte OFF past the lane's addresses and
// the row's 5 reference colours, closed by lgkmcnt(0) (see the general path's reads)
template <int OFF>
__device__ __forceinline__ void ring_taps5(const unsigned (&ra)[5], unsigned rb, u32x3 (&Bv)[5], f32x4 (&Av)[5]) {
  asm volatile(
      "ds_read_b96 %0, %10 offset:%16\n\t"
      "ds_read_b96 %1, %11 offset:%16\n\t"
      "ds_read_b96 %2, %12 offset:%16\n\t"
      "ds_read_b96 %3, %13 offset:%16\n\t"
      "ds_read_b96 %4, %14 offset:%16\n\t"
      "ds_read_b128 %5, %15\n\t"
      "ds_read_b128 %6, %15 offset:80\n\t"
      "ds_read_b128 %7, %15 offset:160\n\t"
      "ds_read_b128 %8, %15 offset:240\n\t"
      "ds_read_b128 %9, %15 offset:320\n\t"
      "s_waitcnt lgkmcnt(0)"
      : "=&v"(Bv[0]), "=&v"(Bv[1]), "=&v"(Bv[2]), "=&v"(Bv[3]), "=&v"(Bv[4]), "=&v"(Av[0]), "=&v"(Av[1]),
        "=&v"(Av[2]), "=&v"(Av[3]), "=&v"(Av[4])
      : "v"(ra[0]), "v"(ra[1]), "v"(ra[2]), "v"(ra[3]), "v"(ra[4]), "v"(rb), "i"(OFF)
      : "memory");
}
template <int WPS>
__global__ __launch_bounds__(256) void k_sweep_spixl_ring(const float4* __restrict__ lab, float* __restrict__ spixl,
                                                          const uint8_t* __restrict__ rep,
                                                          const float* __restrict__ levels, const int* __restrict__ vs,
                                                          const int* __restrict__ sn, SweepArgs a, int fast) {
  constexpr int SPB = 4 / WPS;
  constexpr unsigned kSlotB = kSwU * 16u;            // bytes of a ring slot
  __shared__ __align__(16) float4 ring[4][2][kSwU];  // per wave: two row slots
  __shared__ float4 refc[SPB][25];
  __shared__ int rxr[SPB][5], ryr[SPB][5];           // tap columns (i) and rows (j), possibly outside
  __shared__ unsigned rvm[SPB];                       // bit 5 i + j: tap (i, j) inside the image
  __shared__ float wbest[4];
  __shared__ int wbi[4];
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int h = w % WPS, slot = w / WPS;
  const int z = a.z + blockIdx.y;
  const long M = (long)a.mw * a.mh, P = (long)a.W * a.H;
  const long nbk = (M + SPB - 1) / SPB, per = (nbk + 7) / 8;  // XCD-aware order, as k_sweep_spixl
  const long blk = (long)(blockIdx.x & 7) * per + (blockIdx.x >> 3);
  const long s = blk * SPB + slot;
  const bool active = blk < nbk && s < M;
  const long idx = z * M + (active ? s : 0);
  if (h == 0) {
    const uint8_t* dr = rep + 8 * idx;
    const int bl_ = max((int)dr[0], max((int)dr[1], (int)dr[2]));
    const int br_ = max((int)dr[5], max((int)dr[6], (int)dr[7]));
    const int bt_ = max((int)dr[0], max((int)dr[3], (int)dr[5]));
    const int bb_ = max((int)dr[2], max((int)dr[4], (int)dr[7]));
    const float stx = (float)fmax(1.0, 0.25 * (double)(float)(bl_ + br_));
    const float sty = (float)fmax(1.0, 0.25 * (double)(float)(bt_ + bb_));
    const float cx = spixl[8 * idx + 1], cy = spixl[8 * idx + 2];
    const int i = lane / 5 - 2, j = lane % 5 - 2;  // tap t = lane: i (x) outer, j (y) inner
    const int xr = (int)(cx + (float)i * stx);
    const int yr = (int)(cy + (float)j * sty);
    const bool in = lane < 25 && xr >= 0 && yr >= 0 && xr < a.W && yr < a.H;
    if (lane < 25) {
      // .w: the tap's column, or -2^30 for a tap outside the image (its projection is outside too)
      float4 rc = in ? lab[(long)z * P + (long)yr * a.W + xr] : make_float4(0.f, 0.f, 0.f, 0.f);
      rc.w = __int_as_float(in ? xr : -(1 << 30));
      refc[slot][lane] = rc;
      if (j == -2) rxr[slot][i + 2] = xr;
      if (i == -2) ryr[slot][j + 2] = yr;
    }
    const unsigned long long bal = __ballot(in);
    if (lane == 0) rvm[slot] = (unsigned)bal;
  }
  __syncthreads();
  const unsigned vm = __builtin_amdgcn_readfirstlane(rvm[slot]);
  int xr[5], yr[5];
#pragma unroll
  for (int q = 0; q < 5; q++) {  // (scalars: the window, the row offsets and the tap columns are scalar arithmetic)
    xr[q] = __builtin_amdgcn_readfirstlane(rxr[slot][q]);
    yr[q] = __builtin_amdgcn_readfirstlane(ryr[slot][q]);
  }
  // the union of the inside taps' columns (any row), and the rows holding one
  int xlo = 1 << 30, xhi = -(1 << 30);
#pragma unroll
  for (int q = 0; q < 5; q++)
    if ((vm >> (5 * q)) & 0x1fu) {
      xlo = min(xlo, xr[q]);
      xhi = max(xhi, xr[q]);
    }
  const int rx = z % a.aw;  // (every neighbour in the reference's camera row)
  // the LDS byte addresses of this wave's ring and this superpixel's reference colours
  const unsigned ring_base = (unsigned)(uintptr_t)(lds_ptr_t)&ring[w][0][0];
  const unsigned refc_base = (unsigned)(uintptr_t)(lds_ptr_t)&refc[slot][0];
  const int nn = sn[z];
  float best = SB_INIT;
  int bi = 0x7fffffff;
  for (int p0 = 64 * h; p0 < a.D; p0 += 64 * WPS) {
    const int dl = p0 + lane;
    const bool act = dl < a.D;
    const float d = levels[act ? dl : a.D - 1];
    // the pass's level range: (int)(d dx) is monotone in d, so a neighbour's
    // shift range comes from its ends
    const float dlo = wave_min_f(d), dhi = -wave_min_f(-d);
    // The neighbour being staged (rows k + 2), set up once per (pass,
    // neighbour): its view's plane, this lane's shift, the staging window --
    // columns [ulo, ulo + U) of the view -- the lane's byte offset within a
    // piece, and whether the window is whole: no lane's tap column leaves the
    // image (the window's ends are the extreme lanes' extreme columns, so one
    // scalar test speaks for all 64 lanes) and the slot holds it.
    const float4* pl_s = lab;
    int ulo_s = 0, U_s = 0, sh_s = 0, vo_s = 0;
    bool whole_s = false;
    auto open_nb = [&](int n) {
      const int view = vs[a.V * z + n];
      const float fdx = (float)(view % a.aw - rx);
      sh_s = (int)(d * fdx);  // exact (the launcher checked the levels)
      const int s0 = (int)(dlo * fdx), s1 = (int)(dhi * fdx);
      const int shmin = min(s0, s1), shmax = max(s0, s1);
      const int lo = xlo - shmax, hi = xhi - shmin;
      ulo_s = max(lo, 0);
      const int U = min(hi, a.W - 1) - ulo_s + 1;
      whole_s = lo >= 0 && hi < a.W && U <= kSwU;
      U_s = min(U, kSwU);  // (the launcher's bound makes this a no-op; never past the slot)
      vo_s = 16 * min(lane, max(U_s, 1) - 1);  // U < 64: lanes past U re-read column U - 1
      pl_s = lab + (long)view * P;
    };
    // stage row j of that neighbour into slot sl; returns its LDS-DMA pieces
    // (0: nothing staged -- no inside tap on the row, or an empty window).
    // The view's plane is the buffer, the row and the piece a scalar offset.
    auto stage = [&](int j, int sl) -> int {
      if (U_s <= 0 || !((vm >> j) & 0x108421u)) return 0;
      const __amdgpu_buffer_rsrc_t rs = buf_rsrc(pl_s, (int)(P * 16));
      const int ro = (yr[j] * a.W + ulo_s) * 16;
      const int np = (U_s + 63) >> 6;
      for (int q = 0; q < np; q++) {
        const int c0 = U_s >= 64 ? min(q * 64, U_s - 64) : 0;  // the last piece ends at U
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_ptr_t)&ring[w][sl][c0], 16, vo_s, ro + 16 * c0, 0, 0);
      }
      return np;
    };
    float mn = SB_INIT;
    if (nn > 0) {
      open_nb(0);
      int pcn = stage(0, 0);  // pieces of the row after the one computed next
      pcn = stage(1, 1);
      int ulo_c = ulo_s, sh_c = sh_s;  // the neighbour being computed
      bool whole_c = whole_s;
      for (int n = 0; n < nn; n++) {
        const int par = n & 1;  // row k = 5 n + j sits in slot (n + j) & 1
        // after row j's reads: stage row k + 2 into the slot they left (the
        // next neighbour's rows 0 and 1 from j = 3 on)
        auto stage_ahead = [&](int j) {
          int pc2 = 0;
          if (j < 3 || n + 1 < nn) {
            if (j == 3) open_nb(n + 1);
            pc2 = stage(j < 3 ? j + 2 : j - 3, (par + j) & 1);
          }
          pcn = pc2;
        };
        // The whole-window path, chosen per (pass, neighbour) by scalar
        // tests: all 25 reference taps inside and the window whole, so every
        // tap of every lane is inside.  A lane's five tap addresses are set
        // once (the slot is the read's immediate offset, hence the two
        // parities), a row-step is its 10 LDS reads and 25 VALU, and the chain
        // runs without the outside marker's compare and select.
        auto whole_rows = [&](auto PAR) -> float {
          unsigned ra[5];
#pragma unroll
          for (int i = 0; i < 5; i++) ra[i] = ring_base + (unsigned)(xr[i] - sh_c - ulo_c) * 16u;
          float ad[25];
#pragma unroll
          for (int j = 0; j < 5; j++) {
            wait_vm(5 * n + j + 1 < 5 * nn ? pcn : 0);  // row k landed (row k + 1 may still be in flight)
            u32x3 Bv[5];
            f32x4 Av[5];
            const unsigned rb = refc_base + (unsigned)j * 16u;
            if ((decltype(PAR)::value + j) & 1)
              ring_taps5<(int)kSlotB>(ra, rb, Bv, Av);
            else
              ring_taps5<0>(ra, rb, Bv, Av);
            stage_ahead(j);
#pragma unroll
            for (int i = 0; i < 5; i++) {
              const int t = 5 * i + j;
              ad[t] = tap_ad(make_float4(Av[i].x, Av[i].y, Av[i].z, 0.f), Bv[i]);
            }
          }
          float val = 0.0f;
#pragma unroll
          for (int t = 0; t < 25; t++) val = tap_acc_in(val, ad[t]);
          return val;
        };
        if (fast && vm == 0x1ffffffu && whole_c) {
          const float val = par ? whole_rows(std::integral_constant<int, 1>()) : whole_rows(std::integral_constant<int, 0>());
          mn = val < mn ? val : mn;
          if (n + 1 < nn) ulo_c = ulo_s, sh_c = sh_s, whole_c = whole_s;
          continue;
        }
        float ad[25];
#pragma unroll
        for (int j = 0; j < 5; j++) {
          const int k = 5 * n + j;
          wait_vm(k + 1 < 5 * nn ? pcn : 0);  // row k landed (row k + 1 may still be in flight)
          // the row's 5 taps: their columns (-2^30 for a reference tap
          // outside), then the 5 ring reads and the 5 reference colours in
          // one asm block closed by lgkmcnt(0) -- the compiler would put
          // vmcnt(0) (every LDS-DMA in flight, row k + 1's included) before
          // plain LDS reads here
          int xp[5];
          unsigned ra[5];
#pragma unroll
          for (int i = 0; i < 5; i++) {
            xp[i] = ((vm >> (5 * i + j)) & 1u ? xr[i] : -(1 << 30)) - sh_c;
            const bool in = (unsigned)xp[i] < (unsigned)a.W;
            ra[i] = ring_base + (unsigned)(k & 1) * kSlotB + (in ? (unsigned)(xp[i] - ulo_c) * 16u : 0u);
          }
          const unsigned rb = refc_base + (unsigned)j * 16u;
          u32x3 Bv[5];
          f32x4 Av[5];
          asm volatile(
              "ds_read_b96 %0, %10\n\t"
              "ds_read_b96 %1, %11\n\t"
              "ds_read_b96 %2, %12\n\t"
              "ds_read_b96 %3, %13\n\t"
              "ds_read_b96 %4, %14\n\t"
              "ds_read_b128 %5, %15\n\t"
              "ds_read_b128 %6, %15 offset:80\n\t"
              "ds_read_b128 %7, %15 offset:160\n\t"
              "ds_read_b128 %8, %15 offset:240\n\t"
              "ds_read_b128 %9, %15 offset:320\n\t"
              "s_waitcnt lgkmcnt(0)"
              : "=&v"(Bv[0]), "=&v"(Bv[1]), "=&v"(Bv[2]), "=&v"(Bv[3]), "=&v"(Bv[4]), "=&v"(Av[0]), "=&v"(Av[1]),
                "=&v"(Av[2]), "=&v"(Av[3]), "=&v"(Av[4])
              : "v"(ra[0]), "v"(ra[1]), "v"(ra[2]), "v"(ra[3]), "v"(ra[4]), "v"(rb)
              : "memory");
#pragma unroll
          for (int i = 0; i < 5; i++) {
            const bool in = (unsigned)xp[i] < (unsigned)a.W;
            const float v = tap_ad(make_float4(Av[i].x, Av[i].y, Av[i].z, 0.f), Bv[i]);
            ad[5 * i + j] = in ? v : -1.0f;
          }
          stage_ahead(j);
        }
        float val = 0.0f;
#pragma unroll
        for (int t = 0; t < 25; t++) val = tap_acc(val, ad[t], ad[t] >= 0.0f);
        mn = val < mn ? val : mn;
        // the next neighbour's window (staged from j = 3 of this one)
        if (n + 1 < nn) ulo_c = ulo_s, sh_c = sh_s, whole_c = whole_s;
      }
    }
    if (act && mn < best) {
      best = mn;
      bi = dl;
    }
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const float ob = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (ob < best || (ob == best && oi < bi)) {
      best = ob;
      bi = oi;
    }
  }
  if (lane == 0) {
    wbest[w] = best;
    wbi[w] = bi;
  }
  __syncthreads();
  if (active && h == 0 && lane == 0) {
    for (int k = 1; k < WPS; k++) {
      const float ob = wbest[w + k];
      const int oi = wbi[w + k];
      if (ob < best || (ob == best && oi < bi)) {
        best = ob;
        bi = oi;
      }
    }
    spixl[8 * idx + 7] = (bi != 0x7fffffff && best < SB_INIT) ? levels[bi] : 0.0f;
  }
}

// lab view `view` re-laid for the superpixel sweep (see k_sweep_spixl): KIND 1
// transposed, 2 / 3 sheared along x - y / x + y; 32 x 32 tiles through LDS,
// written along the output's contiguous direction (columns, or diagonals)
template <int KIND>
__global__ __launch_bounds__(256) void k_relayout_lab(const float4* __restrict__ lab, int W, int H, int view,
                                                      float4* __restrict__ out) {
  __shared__ float4 t[32][33];
  const int x0 = blockIdx.x * 32, y0 = blockIdx.y * 32, tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const float4* src = lab + (long)view * W * H;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const int y = y0 + ty + 8 * k, x = x0 + tx;
    if (x < W && y < H) t[ty + 8 * k][tx] = src[(long)y * W + x];
  }
  __syncthreads();
  if (KIND == 1) {
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const int x = x0 + ty + 8 * k, y = y0 + tx;
      if (x < W && y < H) out[(long)x * H + y] = t[tx][ty + 8 * k];
    }
    return;
  }
  // the tile's 63 diagonals, 8 per pass; lane tx = the row within the tile
  for (int d0 = 0; d0 < 63; d0 += 8) {
    const int dd = d0 + ty, yl = tx;
    const int xl = KIND == 2 ? yl + dd - 31 : dd - yl;
    const int x = x0 + xl, y = y0 + yl;
    if (dd < 63 && xl >= 0 && xl < 32 && x < W && y < H)
      out[KIND == 2 ? (long)(x - y + H - 1) * H + y : (long)(x + y) * H + y] = t[yl][xl];
  }
}

}  // namespace

int launch_boundary(hipStream_t s, int V, int W, int H, int S, const float* spixl, const uint32_t* labels,
                    uint8_t* rep) {
  int mw = map_dim(W, S), mh = map_dim(H, S);
  hipLaunchKernelGGL(k_boundary, dim3((mw * mh + 3) / 4, V), dim3(256), 0, s, spixl, labels, W, H, S, mw, mh, rep);
  MVS_LAUNCH_CHECK("k_boundary");
  return 0;
}

// The superpixel sweep of reference views [z0, z1) as plan_sweep_spixl
// (launch_plan.cpp) lays it out.  If the re-layout scratch cannot be had, the
// call is planned again without it (same results, slower gathers).
int launch_sweep_spixl(mvs_ctx* ctx, int V, int W, int H, int S, const float* lab, float* spixl,
                       const uint8_t* rep, const float* levels, int D, const int* vs, const int* sn, int aw,
                       float bl, int z0, int z1) {
  const plan::Tuning t = plan::plan_tuning();
  const auto planned = [&](bool relayout) {
    return plan::plan_sweep_spixl(t, V, W, H, S, D, ctx->h_levels.data(), ctx->h_vs.data(), ctx->h_sn.data(), aw, z0,
                                  z1, relayout);
  };
  plan::SpixlSweepPlan p = planned(true);
  if (p.err) return arg_fail(p.err);
  if (!p.launch) return 0;
  hipStream_t s = ctx->stream;
  const float4* labT = nullptr;
  const int* tslot = nullptr;
  if (p.units > 0) {
    int rc = 0;
    float4* buf = (float4*)scratch(ctx, (size_t)p.units * p.tstride * sizeof(float4), &rc);
    if (rc == MVS_E_NOMEM) {
      (void)hipGetLastError();  // the failed hipMalloc must not fail the next launch check
      p = planned(false);
    } else if (rc) {
      return rc;
    } else {
      tslot = plan_upload(ctx, p.slot, &rc);
      if (rc) return rc;
      labT = buf;
      const dim3 tg((W + 31) / 32, (H + 31) / 32);
      static constexpr void (*relayout[3])(const float4*, int, int, int, float4*) = {k_relayout_lab<1>, k_relayout_lab<2>,
                                                                                     k_relayout_lab<3>};
      for (const plan::SpixlRelayout& r : p.relayouts)
        hipLaunchKernelGGL(relayout[r.kind - 1], tg, dim3(256), 0, s, (const float4*)lab, W, H, r.view,
                           buf + (long)r.slot * p.tstride);
      MVS_LAUNCH_CHECK("k_relayout_lab");
    }
  }
  SweepArgs a{V, W, H, p.mw, p.mh, D, aw, z0, bl};
  const dim3 g(p.grid_x, p.grid_y);
  if (p.form == plan::kSweepHzRing) {
    static constexpr void (*ring[3])(const float4*, float*, const uint8_t*, const float*, const int*, const int*,
                                     SweepArgs, int) = {k_sweep_spixl_ring<1>, k_sweep_spixl_ring<2>, k_sweep_spixl_ring<4>};
    hipLaunchKernelGGL(ring[p.wps == 1 ? 0 : p.wps == 2 ? 1 : 2], g, dim3(256), 0, s, (const float4*)lab, spixl, rep,
                       levels, vs, sn, a, (int)t.sweep_ring_fast);
    MVS_LAUNCH_CHECK("k_sweep_spixl_ring");
  } else {
    const bool half = p.lps == 32;
    const auto kern = p.form == plan::kSweepRelaid     ? (half ? k_sweep_spixl<32, true> : k_sweep_spixl<64, true>)
                      : p.form == plan::kSweepHzGather ? (half ? k_sweep_spixl<32, false, true> : k_sweep_spixl<64, false, true>)
                                                       : (half ? k_sweep_spixl<32, false> : k_sweep_spixl<64, false>);
    hipLaunchKernelGGL(kern, g, dim3(256), 0, s, (const float4*)lab, spixl, rep, levels, vs, sn, a, p.wps, labT, tslot,
                       p.tstride);
    MVS_LAUNCH_CHECK("k_sweep_spixl");
  }
  std::copy(p.last, p.last + 5, ctx->sweep_last);
  return 0;
}

}  // namespace mvs
