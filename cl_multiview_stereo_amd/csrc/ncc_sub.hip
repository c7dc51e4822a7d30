// Sub-level disparity of the per-pixel NCC sweep: a three-point parabola fit
// through the costs of the winning level and its two neighbours in level order.
//
// Definition (tests/subpixel_ref.py; float32, every operation rounded, no
// fused multiply-add).  For a pixel with costs vol[0..D-1] (ncc.hip's
// definition) and levels[0..D-1]:
//   b    = first index of the minimum in level order, strict <  (k_wta's rule)
//   cm, c0, cp = vol[b-1], vol[b], vol[b+1]
//   ok   = 0 < b < D-1 and cm < 2 and cp < 2     (a cost of 2: no valid window)
//   den  = (cm - c0) + (cp - c0)                 (> 0 whenever ok)
//   off  = (0.5 * (cm - cp)) / den               (|off| <= 0.5)
//   step = off < 0 ? levels[b] - levels[b-1] : levels[b+1] - levels[b]
//   disp_sub = ok ? levels[b] + off * step : levels[b]
//
// k_wta_sub (wta.hip) streams a materialised volume (the two-pass path); the
// fit itself is ncc_common.h's parabola, shared by both.  k_ncc_sub is
// the post-pass of the fused sweep, which keeps no volume: it recovers b from
// the integer-level disparity the sweep wrote (levels strictly increasing: a
// binary search by value) and recomputes the three costs from the window
// planes of mvs_box_stats_d, bit for bit k_ncc_volume's:
//   * the reference window's Sr' and var as exact integers from its own packed
//     rows (v_dot4_i32_i8 with ones / with itself), s_r = 1/sqrtf(var);
//   * per (level, neighbour) the K packed rows of the shifted window, read as
//     the (K+1)/2 16-byte row pairs that hold them, give Srp' by v_dot4_i32_i8
//     under the K-tap mask (the three levels of a neighbour share packed
//     entries where their windows overlap: see the loop); a, b of the shifted
//     window from the stats plane (NaN where that window leaves the image:
//     v_max_f32 drops it);
//   * x = fma(-Sr', b, Srp' * a), m = max, cost = 1 - max(-1, m * s_r).
// One lane per pixel, a wave on 64 consecutive columns of one row, four rows
// per workgroup: neighbouring pixels have neighbouring winners, so the gathers
// at x - tx stay close to coalesced.  Every plane address is kept inside the
// view's plane: a window that leaves the image is invalid (NaN in the stats
// plane, dropped by the maximum), so its packed rows are read from a window
// moved into the image and its a, b from the clamped pixel (an edge pixel's
// window is invalid too); a pixel whose winner is the first or last level, or
// whose disparity matches no level, reads nothing further.
#include <algorithm>

#include "ncc_common.h"

namespace mvs {
namespace {
using namespace ncc;

constexpr int kSubLdsLevels = 1024;  // levels kept in LDS by k_ncc_sub (4 KB); more are searched in global memory

// Image rows r0 .. r0 + K - 1 (all inside the image) of column xc of one
// view's packed plane: the (K+1)/2 row pairs holding them as 16-byte reads at
// 32-bit byte offsets from the wave-uniform plane base (a view's plane is
// under 2 GB), then the rows picked by r0's parity.
template <int K>
__device__ __forceinline__ void load_rows(const uint2* __restrict__ plane, unsigned W, int xc, int r0,
                                          u32x2 (&v)[K]) {
  constexpr int NP = (K + 1) / 2;
  const bool odd = r0 & 1;
  const unsigned off = ((unsigned)(r0 >> 1) * W + (unsigned)xc) * 16u;
  u32x4 t[NP];
#pragma unroll
  for (int i = 0; i < NP; i++) t[i] = *(const u32x4*)((const char*)plane + (off + (unsigned)i * 16u * W));
#pragma unroll
  for (int k = 0; k < K; k++) {
    // even start: row k is half k & 1 of pair k / 2; odd start: half (k + 1) & 1 of pair (k + 1) / 2
    const u32x2 e = (k & 1) ? t[k / 2].zw : t[k / 2].xy;
    const u32x2 o = ((k + 1) & 1) ? t[(k + 1) / 2].zw : t[(k + 1) / 2].xy;
    v[k] = odd ? o : e;
  }
}

template <int K>
__global__ __launch_bounds__(256) void k_ncc_sub(const uint2* __restrict__ stats, const uint2* __restrict__ pk,
                                                 const float* __restrict__ levels, int D,
                                                 const int* __restrict__ vs, const int* __restrict__ sn, int V,
                                                 int aw, float bl, int W, int H, int tiles_x, int z0,
                                                 const float* disp, float* disp_sub) {
  constexpr int R = K / 2, NK = K * K;
  constexpr unsigned HI_MASK = (K - 4) >= 4 ? 0xffffffffu : ((1u << (8 * (K - 4))) - 1u);
  // the levels in LDS when they fit: the search below is a chain of dependent
  // reads, ~log2(D) global-memory latencies per pixel otherwise
  __shared__ float lds_levels[kSubLdsLevels];
  const bool in_lds = D <= kSubLdsLevels;
  if (in_lds)
    for (int i = threadIdx.x; i < D; i += 256) lds_levels[i] = levels[i];
  __syncthreads();
  const int tile_y = blockIdx.x / tiles_x, tile_x = blockIdx.x - tile_y * tiles_x;
  const int x = tile_x * 64 + (threadIdx.x & 63), y = tile_y * 4 + (threadIdx.x >> 6);
  if (x >= W || y >= H) return;
  const int z = z0 + blockIdx.z;
  const long p = (long)blockIdx.z * W * H + (long)y * W + x;
  const float d0 = disp[p];
  // the winner's index, by value (levels strictly increasing)
  int lo = 0, hi = D - 1;
  if (in_lds) {
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (lds_levels[mid] < d0)
        lo = mid + 1;
      else
        hi = mid;
    }
  } else {
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (levels[mid] < d0)
        lo = mid + 1;
      else
        hi = mid;
    }
  }
  const int b = lo;
  // the reference window leaves the image: every cost is 2 and the fit is off
  const bool rin = x - R >= 0 && x + R < W && y - R >= 0 && y + R < H;
  if (!(b > 0 && b < D - 1 && rin && (in_lds ? lds_levels[b] : levels[b]) == d0)) {
    disp_sub[p] = d0;
    return;
  }
  const long Pv = (long)W * ((H + 1) >> 1) * 2;  // uint2 per view plane
  // reference: Sr', var and s_r from its packed rows (exact integers)
  u32x2 q[K];
  load_rows<K>(pk + z * Pv, W, x, y - R, q);
  int s1 = 0, s2 = 0;
#pragma unroll
  for (int k = 0; k < K; k++) {
    q[k].y &= HI_MASK;
    s1 = dot4(q[k].x, 0x01010101u, dot4(q[k].y, 0x01010101u, s1));
    s2 = dot4(q[k].x, q[k].x, dot4(q[k].y, q[k].y, s2));
  }
  const int var = NK * s2 - s1 * s1;
  const float sr = var != 0 ? 1.0f / sqrtf((float)var) : 0.0f;
  const float rsn = -(float)s1;
  const int rx = z % aw, ry = z / aw, nn = sn[z];
  float lv[3], m[3];
#pragma unroll
  for (int j = 0; j < 3; j++) {
    lv[j] = in_lds ? lds_levels[b - 1 + j] : levels[b - 1 + j];
    m[j] = -INFINITY;
  }
  // One packed entry holds the 8 columns from its window's left edge on, so it
  // serves the windows centred up to SPAN columns to its right.  The three
  // levels' windows in a neighbour are |dx| level steps apart: when they share
  // their rows and their centres lie in the image, the entry at the leftmost
  // centre and the one SPAN columns left of the rightmost hold every tap
  // (K = 5: column shifts up to 3 per level, K = 7: 1) -- (K+1)/2 or K+1 pair
  // reads instead of 3 (K+1)/2.  Otherwise each level reads its own entry.
  constexpr int SPAN = 8 - K;
  for (int n = 0; n < nn; n++) {
    const int view = vs[V * z + n];
    const float fdx = (float)(view % aw - rx), fdy = (float)(view / aw - ry);
    int px[3], py[3];
#pragma unroll
    for (int j = 0; j < 3; j++) {
      // the shift, held to +-2^30 so x - tx cannot wrap (such a window is far outside the image)
      px[j] = x - (int)fminf(fmaxf(round_ha(lv[j] * fdx), -1073741824.0f), 1073741824.0f);
      py[j] = y - (int)fminf(fmaxf(round_ha((bl * lv[j]) * fdy), -1073741824.0f), 1073741824.0f);
    }
    const int cmin = min(px[0], min(px[1], px[2])), cmax = max(px[0], max(px[1], px[2]));
    const int c1 = max(cmax - SPAN, cmin);  // the second entry's column
    bool shared = py[0] == py[1] && py[1] == py[2] && cmin >= 0 && cmax <= W - 1;
#pragma unroll
    for (int j = 0; j < 3; j++) shared = shared && (px[j] - cmin <= SPAN || px[j] >= c1);
    const uint2* pkv = pk + view * Pv;
    const float* stv = (const float*)(stats + view * Pv);
    int srp[3];
    if (shared) {
      u32x2 e0[K], e1[K];
      const int r0 = min(max(py[0], R), H - 1 - R) - R;  // (a window off the image is invalid: any rows do)
      load_rows<K>(pkv, W, cmin, r0, e0);
      if (cmax - cmin > SPAN) {
        load_rows<K>(pkv, W, c1, r0, e1);
      } else {
#pragma unroll
        for (int k = 0; k < K; k++) e1[k] = e0[k];
      }
#pragma unroll
      for (int j = 0; j < 3; j++) {
        const bool first = px[j] - cmin <= SPAN;
        const int sh = first ? px[j] - cmin : px[j] - c1;  // 0 .. SPAN bytes
        int acc = 0;
#pragma unroll
        for (int k = 0; k < K; k++) {
          const unsigned lo = first ? e0[k].x : e1[k].x, hi = first ? e0[k].y : e1[k].y;
          acc = dot4(q[k].x, __builtin_amdgcn_alignbyte(hi, lo, sh), dot4(q[k].y, hi >> (8 * sh), acc));
        }
        srp[j] = acc;
      }
    } else {
#pragma unroll
      for (int j = 0; j < 3; j++) {
        u32x2 w[K];
        load_rows<K>(pkv, W, min(max(px[j], 0), W - 1), min(max(py[j], R), H - 1 - R) - R, w);
        int acc = 0;
#pragma unroll
        for (int k = 0; k < K; k++) acc = dot4(q[k].x, w[k].x, dot4(q[k].y, w[k].y, acc));
        srp[j] = acc;
      }
    }
#pragma unroll
    for (int j = 0; j < 3; j++) {
      // a, b of the shifted window: floats (py & 1) and 2 + (py & 1) of its row pair's 16 bytes
      // (clamped into the plane: an edge pixel's window is invalid, NaN)
      const int ys = min(max(py[j], 0), H - 1), xs = min(max(px[j], 0), W - 1);
      const float* sp = (const float*)((const char*)stv + (((unsigned)(ys >> 1) * W + xs) * 4u + (ys & 1)) * 4u);
      m[j] = vmax(m[j], fmaf(rsn, sp[2], (float)srp[j] * sp[0]));
    }
  }
  float c[3];
#pragma unroll
  for (int j = 0; j < 3; j++) c[j] = 1.0f - vmax_m1(m[j] * sr);
  disp_sub[p] = parabola(c[0], c[1], c[2], lv[0], lv[1], lv[2]);
}

}  // namespace

int launch_ncc_sub(hipStream_t s, int V, int W, int H, const int32_t* box, const float* levels_dev, int D,
                   const int* vs_dev, const int* sn_dev, int aw, float bl, int K, int z0, int z1, const float* disp,
                   float* disp_sub) {
  const uint2* stats = (const uint2*)box;
  const uint2* pk = stats + (long)V * W * (H + (H & 1));
  const long P = (long)W * H;
  for (int za = z0; za < z1; za += 65535) {  // grid.z holds at most 65535 reference views
    const int n = std::min(z1 - za, 65535);
    const int tiles_x = (W + 63) / 64;
    const dim3 g((unsigned)((long)tiles_x * ((H + 3) / 4)), 1, n);  // tiles of 64 columns x 4 rows
    const float* di = disp + P * (za - z0);
    float* ds = disp_sub + P * (za - z0);
    if (K == 5)
      hipLaunchKernelGGL(k_ncc_sub<5>, g, dim3(256), 0, s, stats, pk, levels_dev, D, vs_dev, sn_dev, V, aw, bl, W, H,
                         tiles_x, za, di, ds);
    else
      hipLaunchKernelGGL(k_ncc_sub<7>, g, dim3(256), 0, s, stats, pk, levels_dev, D, vs_dev, sn_dev, V, aw, bl, W, H,
                         tiles_x, za, di, ds);
    MVS_LAUNCH_CHECK("k_ncc_sub");
  }
  return 0;
}

}  // namespace mvs
