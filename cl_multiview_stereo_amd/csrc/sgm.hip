// Semi-global aggregation of a cost volume vol [D][H][W] along the four
// axis-aligned paths (include/mvs.h at mvs_sgm_d; tests/sgm_ref.py) and the
// four diagonal ones (mvs_sgm8_d).
//
// Definition, float32, every operation rounded (there is no multiply, so
// nothing can fuse).  q is the pixel before p on the path:
//   first pixel:  L(p, d) = vol[d][p]
//   else:  m = min_k L(q, k)
//          t = min(L(q, d), L(q, d-1) + P1 (d > 0), L(q, d+1) + P1 (d < D-1), m + P2)
//          L(p, d) = (vol[d][p] + t) - m
//   agg = ((L_b0 + L_b1) + L_b2) + L_b3 over the set bits of `paths`, in bit
//   order: one launch per path, the first stores L, the others add to agg.
// A level that does not exist (d-1 at 0, d+1 at D-1, the padding up to a lane's
// or a wave's level count) is a state of +inf: inf + P1 drops out of the
// minimum, and a padded level's own L stays +inf (m is finite, no NaN arises)
// and is never stored.
//
// The layout decides the two forms (launch_plan.h at plan_sgm):
//  * k_sgm_lanes: lanes over levels, one workgroup per line.  A lane keeps LPL
//    consecutive levels of L(q, .) in registers, so d-1 and d+1 cross a lane
//    boundary once per side (one shuffle each) and m is an in-wave reduction
//    (DPP within the rows of 16 lanes, then four lane reads): no LDS and no
//    barrier up to 1024 levels.  Above, the workgroup's waves leave {minimum,
//    first, last} in LDS, double-buffered: one barrier per step.
//    Along x a level's consecutive pixels are contiguous: VEC reads vol and
//    reads-modifies-writes agg in aligned 16-byte pieces.  Which pixels share
//    a piece depends on the level (the plane pitch H W need not be a multiple
//    of 4) and on the row, so every (lane, level) has its own phase
//    ph = (address of the line's first element / 4) mod 4: pixel x is element
//    j = (x + ph) mod 4 of the piece of pixels x - j .. x - j + 3.  A piece
//    inside the line is loaded when the walk enters it; when the walk leaves
//    it, it is complete and is stored one step later, behind that step's
//    loads (memory operations retire in order: a load issued behind a store
//    waits for the store as well).  The pixels of a piece that crosses an end
//    of the line are read and written one by one (the scalar head and tail).
//  * k_sgm_columns: vertical paths at D <= 256.  Lanes over levels would read
//    4 bytes per plane there, so the lanes lie over 64 consecutive columns (a
//    level's row piece is one coalesced 256 bytes) and the levels are split
//    over the waves, 16 per wave, unrolled in registers.  Per row the waves
//    exchange {chunk minimum, first, last} per column through LDS,
//    double-buffered: one barrier per row.  The next row's costs and agg
//    are loaded before the waves meet and before this row's stores.
//  * k_sgm_diag: the four diagonal paths of mvs_sgm8_d (bits 4..7: steps
//    (+1, +1), (-1, -1), (-1, +1), (+1, -1) per pixel; tests/sgm8_ref.py) at
//    D <= 256: k_sgm_columns with its band of 64 columns moving by one column
//    per row, so that a lane follows one diagonal line and its state never
//    leaves the lane.  A level's row piece is still one coalesced 256 bytes;
//    its start moves by one float per row and is not aligned.  Above 256 levels
//    a diagonal line is a strided line of k_sgm_lanes (DIAG), one workgroup per
//    line, elements W + 1 or W - 1 apart.
// Plane bases are 64-bit, offsets within a plane 32-bit (W H <= 2^27).
//
// Every form takes N volumes of one shape per launch (mvs_sgm8_batch_d): the
// batch index is blockIdx.y, and a kernel first moves its two bases to its
// element (blockIdx.y * stride, 64-bit); nothing else knows of the batch.  The
// single-volume entry points launch with N = 1.
#include "mvs_internal.h"

namespace mvs {
namespace {

#define SGM_INF __builtin_inff()

template <int CTRL>
__device__ __forceinline__ float dpp_min(float v) {
  const int o = __builtin_amdgcn_update_dpp(__float_as_int(v), __float_as_int(v), CTRL, 0xf, 0xf, false);
  return fminf(v, __int_as_float(o));
}

// the minimum over the 64 lanes, in every lane (all lanes active)
__device__ __forceinline__ float wave_min(float v) {
  v = dpp_min<0xB1>(v);   // quad_perm [1,0,3,2]
  v = dpp_min<0x4E>(v);   // quad_perm [2,3,0,1]
  v = dpp_min<0x141>(v);  // row_half_mirror: the other quad of the 8
  v = dpp_min<0x140>(v);  // row_mirror: the other half of the row of 16
  const int b = __float_as_int(v);
  const float r0 = __int_as_float(__builtin_amdgcn_readlane(b, 0)), r1 = __int_as_float(__builtin_amdgcn_readlane(b, 16));
  const float r2 = __int_as_float(__builtin_amdgcn_readlane(b, 32)), r3 = __int_as_float(__builtin_amdgcn_readlane(b, 48));
  return fminf(fminf(r0, r1), fminf(r2, r3));
}

__device__ __forceinline__ float pick(const float4& v, int j) { return j == 0 ? v.x : j == 1 ? v.y : j == 2 ? v.z : v.w; }
__device__ __forceinline__ void put(float4& v, int j, float s) {
  v.x = j == 0 ? s : v.x;
  v.y = j == 1 ? s : v.y;
  v.z = j == 2 ? s : v.z;
  v.w = j == 3 ? s : v.w;
}

// One step of NL consecutive levels: L(q, .) in L -> L(p, .); up, dn = L(q, .)
// of the level below the first and above the last (+inf: none).
template <int NL>
__device__ __forceinline__ void sgm_step(float (&L)[NL], const float (&c)[NL], float up, float dn, float m, float P1,
                                         float P2) {
  const float mp2 = m + P2;
  float prev = up;
#pragma unroll
  for (int k = 0; k < NL; k++) {
    const float cur = L[k], nxt = k + 1 < NL ? L[k + 1] : dn;
    const float t = fminf(fminf(cur, prev + P1), fminf(nxt + P1, mp2));
    L[k] = (c[k] + t) - m;
    prev = cur;
  }
}

// DIAG (not VEC): line blockIdx.x of the W + H - 1 diagonal lines with elements sstride = W +- 1 apart; its first
// element and its length come from the line index (plan::sgm_diag_line), and the arguments n and lstride carry W
// and H instead.
template <int LPL, bool VEC, bool MW, bool DIAG = false>
__global__ __launch_bounds__(MW ? 1024 : 64) void k_sgm_lanes(const float* __restrict__ vol, float* __restrict__ agg,
                                                              size_t vstride, size_t astride, int D, long HW, int n,
                                                              int sstride, int lstride, int rev, int acc, float P1,
                                                              float P2) {
  static_assert(!(DIAG && VEC), "a diagonal line is not contiguous");
  vol += (size_t)blockIdx.y * vstride;  // the batch element: 64-bit, before anything is derived from the bases
  agg += (size_t)blockIdx.y * astride;
  const int lane = threadIdx.x & 63;
  const int d0 = (int)threadIdx.x * LPL;  // the lane's first level; levels >= D are padding and touch no memory
  long first = (long)((unsigned)blockIdx.x * (unsigned)lstride);
  if constexpr (DIAG) {
    const plan::SgmDiagLine ln = plan::sgm_diag_line(n, lstride, sstride - n, (int)blockIdx.x);
    first = ln.first;
    n = ln.n;  // (uniform over the workgroup: every wave meets every barrier)
  }
  const long base = (long)d0 * HW + first;
  const float* vp = vol + base;
  float* ap = agg + base;
  const int jl = rev ? 3 : 0, js = rev ? 0 : 3;  // the element at which the walk enters / leaves a piece
  float L[LPL];
  float4 cv[LPL], av[LPL], pv[LPL];  // the piece of vol, of agg, and the completed piece of agg waiting to be stored
  int ph[LPL], pxs[LPL];             // pxs: where pv goes (-1: nothing waits)
#pragma unroll
  for (int k = 0; k < LPL; k++) {
    L[k] = SGM_INF;
    cv[k] = av[k] = pv[k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    pxs[k] = -1;
    ph[k] = VEC ? (int)(((uintptr_t)(vp + (long)k * HW) >> 2) & 3) : 0;  // (vol and agg: equal mod 16 bytes)
  }
  for (int i = 0; i < n; i++) {
    const int x = rev ? n - 1 - i : i;
    float c[LPL];
    if (VEC) {
      // the pieces this step enters, every level's before anything waits for one
#pragma unroll
      for (int k = 0; k < LPL; k++) {
        const int j = (x + ph[k]) & 3, xs = x - j;
        if (d0 + k < D && j == jl && xs >= 0 && xs + 3 < n) {
          cv[k] = *(const float4*)(vp + (long)k * HW + xs);
          if (acc) av[k] = *(const float4*)(ap + (long)k * HW + xs);
        }
      }
      // then the pieces the last step completed, behind the loads: issued in front of them, the loads' data would
      // wait for these stores as well
#pragma unroll
      for (int k = 0; k < LPL; k++) {
        if (pxs[k] >= 0) {
          *(float4*)(ap + (long)k * HW + pxs[k]) = pv[k];
          pxs[k] = -1;
        }
      }
    }
#pragma unroll
    for (int k = 0; k < LPL; k++) {
      c[k] = SGM_INF;
      if (d0 + k < D) {
        const float* r = vp + (long)k * HW;
        if (VEC) {
          const int j = (x + ph[k]) & 3, xs = x - j;
          c[k] = (xs >= 0 && xs + 3 < n) ? pick(cv[k], j) : r[x];
        } else {
          c[k] = r[x * sstride];
        }
      }
    }
    if (i == 0) {
#pragma unroll
      for (int k = 0; k < LPL; k++) L[k] = c[k];
    } else {
      float m = L[0];
#pragma unroll
      for (int k = 1; k < LPL; k++) m = fminf(m, L[k]);
      m = wave_min(m);
      float up = __shfl_up(L[LPL - 1], 1), dn = __shfl_down(L[0], 1);
      if (lane == 0) up = SGM_INF;
      if (lane == 63) dn = SGM_INF;
      if constexpr (MW) {
        __shared__ float ex[2][16][3];  // {minimum, first level, last level} of each wave
        const int par = i & 1, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
        if (lane == 0) {
          ex[par][w][0] = m;
          ex[par][w][1] = L[0];
        }
        if (lane == 63) ex[par][w][2] = L[LPL - 1];
        // a wave writes buffer par again two steps on, past the next barrier: every wave has read this one by then
        __syncthreads();
        m = ex[par][0][0];
        for (int v = 1; v < nw; v++) m = fminf(m, ex[par][v][0]);
        if (lane == 0 && w > 0) up = ex[par][w - 1][2];
        if (lane == 63 && w + 1 < nw) dn = ex[par][w + 1][1];
      }
      sgm_step<LPL>(L, c, up, dn, m, P1, P2);
    }
#pragma unroll
    for (int k = 0; k < LPL; k++) {
      if (d0 + k < D) {
        float* r = ap + (long)k * HW;
        if (VEC) {
          const int j = (x + ph[k]) & 3, xs = x - j;
          if (xs >= 0 && xs + 3 < n) {
            put(av[k], j, acc ? pick(av[k], j) + L[k] : L[k]);
            if (j == js) {  // the piece is complete: stored at the next step, after that step's loads
              pv[k] = av[k];
              pxs[k] = xs;
            }
          } else {
            r[x] = acc ? r[x] + L[k] : L[k];
          }
        } else {
          const int o = x * sstride;
          r[o] = acc ? r[o] + L[k] : L[k];
        }
      }
    }
  }
  if (VEC) {
#pragma unroll
    for (int k = 0; k < LPL; k++)
      if (pxs[k] >= 0) *(float4*)(ap + (long)k * HW + pxs[k]) = pv[k];
  }
}

constexpr int LPW = plan::kSgmColumnsLpw;

// NT: the workgroup's thread limit (512 up to 8 waves: 128 levels)
template <int NT>
__global__ __launch_bounds__(NT) void k_sgm_columns(const float* __restrict__ vol, float* __restrict__ agg,
                                                    size_t vstride, size_t astride, int D, int W, int H, int rev,
                                                    int acc, float P1, float P2) {
  vol += (size_t)blockIdx.y * vstride;  // the batch element
  agg += (size_t)blockIdx.y * astride;
  __shared__ float ex[2][NT / 64][3][64];  // per wave and column: {chunk minimum, first level, last level}
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const int x = blockIdx.x * 64 + lane;
  const bool in = x < W;  // a column past the image: +inf (NaN from the second row on), read and stored nowhere
  const long HW = (long)W * H;
  const int dw = w * LPW;
  const float* vw = vol + (long)dw * HW;
  float* aw = agg + (long)dw * HW;
  float L[LPW], c[LPW], a[LPW];
  const auto load = [&](const float* pl, int y, float(&cc)[LPW], float pad) {
    const int off = y * W + x;
#pragma unroll
    for (int k = 0; k < LPW; k++) {
      cc[k] = pad;
      if (in && dw + k < D) cc[k] = pl[(long)k * HW + off];
    }
  };
  const int dy = rev ? -1 : 1;
  int y = rev ? H - 1 : 0;
  load(vw, y, c, SGM_INF);
  if (acc) load(aw, y, a, 0.0f);
  for (int i = 0; i < H; i++, y += dy) {
    // the next row's costs and agg are on their way while the waves meet, and are issued before this row's
    // stores: memory operations retire in order, so a load issued behind a store waits for the store as well
    float cn[LPW], an[LPW];
    if (i + 1 < H) {
      load(vw, y + dy, cn, SGM_INF);
      if (acc) load(aw, y + dy, an, 0.0f);
    }
    if (i == 0) {
#pragma unroll
      for (int k = 0; k < LPW; k++) L[k] = c[k];
    } else {
      const int par = i & 1;
      float m = L[0];
#pragma unroll
      for (int k = 1; k < LPW; k++) m = fminf(m, L[k]);
      ex[par][w][0][lane] = m;
      ex[par][w][1][lane] = L[0];
      ex[par][w][2][lane] = L[LPW - 1];
      // a wave writes buffer par again two rows on, past the next barrier: every wave has read this one by then
      __syncthreads();
      m = ex[par][0][0][lane];
      for (int v = 1; v < nw; v++) m = fminf(m, ex[par][v][0][lane]);
      const float up = w > 0 ? ex[par][w - 1][2][lane] : SGM_INF;
      const float dn = w + 1 < nw ? ex[par][w + 1][1][lane] : SGM_INF;
      sgm_step<LPW>(L, c, up, dn, m, P1, P2);
    }
    const int off = y * W + x;
#pragma unroll
    for (int k = 0; k < LPW; k++)
      if (in && dw + k < D) aw[(long)k * HW + off] = acc ? a[k] + L[k] : L[k];
    if (i + 1 < H) {
#pragma unroll
      for (int k = 0; k < LPW; k++) {
        c[k] = cn[k];
        if (acc) a[k] = an[k];
      }
    }
  }
}

// Diagonal paths at D <= 256: k_sgm_columns, sheared.  Lane `lane` of workgroup g follows one diagonal line: at
// image row y it stands on column x0 + sx y (launch_plan.h at plan_sgm_diag) and is live there iff that lies in
// [0, W).  Along the walk a lane is live on one run of rows: its first live row is the first pixel of its path
// (L = cost, never a step from what it held outside), and once it has left the image it stays out; it stores
// on its live rows only.  The rows [ylo, yhi] at which some lane is live are uniform over the workgroup, so
// every wave meets every barrier.
template <int NT>
__global__ __launch_bounds__(NT) void k_sgm_diag(const float* __restrict__ vol, float* __restrict__ agg,
                                                 size_t vstride, size_t astride, int D, int W, int H, int sx, int rev,
                                                 int acc, float P1, float P2) {
  vol += (size_t)blockIdx.y * vstride;  // the batch element
  agg += (size_t)blockIdx.y * astride;
  __shared__ float ex[2][NT / 64][3][64];  // per wave and line: {chunk minimum, first level, last level}
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const int g = blockIdx.x;
  const int x0 = plan::sgm_diag_x0(g, lane, H, sx);
  const int ylo = plan::sgm_diag_ylo(g, W, H, sx), n = plan::sgm_diag_yhi(g, W, H, sx) - ylo + 1;
  const long HW = (long)W * H;
  const int dw = w * LPW;
  const float* vw = vol + (long)dw * HW;
  float* aw = agg + (long)dw * HW;
  float L[LPW], c[LPW], a[LPW];
  // Row y's own column.  A lane outside the image reads the row's nearest pixel instead of nothing: what it
  // holds is never stored and never reaches a live state (`was` below), and with no lane-dependent condition
  // around or behind a load nothing waits for one before the row after uses it (a select on `in` behind each
  // load made every load wait for itself: 9.2 ms per path at 1080p, D = 128, against 2.4 ms)
  const auto load = [&](const float* pl, int y, float(&cc)[LPW], float pad) {
    const int off = y * W + min(max(x0 + sx * y, 0), W - 1);
#pragma unroll
    for (int k = 0; k < LPW; k++) {
      cc[k] = pad;
      if (dw + k < D) cc[k] = pl[(long)k * HW + off];
    }
  };
  const int dy = rev ? -1 : 1;
  int y = rev ? ylo + n - 1 : ylo;
  bool was = false;  // the lane was live on the row before: this row steps from it
  load(vw, y, c, SGM_INF);
  if (acc) load(aw, y, a, 0.0f);
  for (int i = 0; i < n; i++, y += dy) {
    // as in k_sgm_columns: the next row's loads before the waves meet and before this row's stores
    float cn[LPW], an[LPW];
    if (i + 1 < n) {
      load(vw, y + dy, cn, SGM_INF);
      if (acc) load(aw, y + dy, an, 0.0f);
    }
    const int x = x0 + sx * y;
    const bool in = x >= 0 && x < W;
    if (i > 0) {  // (on the first row no lane has a pixel before it)
      const int par = i & 1;
      float m = L[0];
#pragma unroll
      for (int k = 1; k < LPW; k++) m = fminf(m, L[k]);
      ex[par][w][0][lane] = m;
      ex[par][w][1][lane] = L[0];
      ex[par][w][2][lane] = L[LPW - 1];
      // a wave writes buffer par again two rows on, past the next barrier: every wave has read this one by then
      __syncthreads();
      m = ex[par][0][0][lane];
      for (int v = 1; v < nw; v++) m = fminf(m, ex[par][v][0][lane]);
      const float up = w > 0 ? ex[par][w - 1][2][lane] : SGM_INF;
      const float dn = w + 1 < nw ? ex[par][w + 1][1][lane] : SGM_INF;
      sgm_step<LPW>(L, c, up, dn, m, P1, P2);
    }
#pragma unroll
    for (int k = 0; k < LPW; k++) L[k] = was ? L[k] : c[k];
    was = in;
    const int off = y * W + x;
#pragma unroll
    for (int k = 0; k < LPW; k++)
      if (in && dw + k < D) aw[(long)k * HW + off] = acc ? a[k] + L[k] : L[k];
    if (i + 1 < n) {
#pragma unroll
      for (int k = 0; k < LPW; k++) {
        c[k] = cn[k];
        if (acc) a[k] = an[k];
      }
    }
  }
}

// The batch of a launch: N elements on the grid's second axis, element i at vol + i vstride, agg + i astride.
struct SgmBatch {
  unsigned N;
  const float* vol;
  size_t vstride;
  float* agg;
  size_t astride;
};

template <bool VEC, bool MW>
void launch_lanes(hipStream_t s, const plan::SgmPlan& p, const SgmBatch& b, int D, long HW, int acc, float P1,
                  float P2) {
#define SGM_LANES(LPL)                                                                                          \
  hipLaunchKernelGGL((k_sgm_lanes<LPL, VEC, MW>), dim3(p.grid, b.N), dim3(p.block), 0, s, b.vol, b.agg, b.vstride, \
                     b.astride, D, HW, p.n, p.sstride, p.lstride, (int)p.rev, acc, P1, P2)
  if constexpr (MW) {
    SGM_LANES(16);
  } else {
    switch (p.lpl) {
      case 1: SGM_LANES(1); break;
      case 2: SGM_LANES(2); break;
      case 4: SGM_LANES(4); break;
      case 8: SGM_LANES(8); break;
      default: SGM_LANES(16); break;
    }
  }
#undef SGM_LANES
}

// one diagonal path (4..7)
int launch_diag(hipStream_t s, int W, int H, int D, const SgmBatch& b, float P1, float P2, int path, int acc) {
  const plan::SgmDiagPlan p = plan::plan_sgm_diag(W, H, D, path);
  if (p.err) return arg_fail(p.err);
  const long HW = (long)W * H;
  const dim3 grid(p.grid, b.N);
#define SGM_DIAG_LANES(LPL, MW)                                                                                 \
  hipLaunchKernelGGL((k_sgm_lanes<LPL, false, MW, true>), grid, dim3(p.block), 0, s, b.vol, b.agg, b.vstride,   \
                     b.astride, D, HW, W, p.sstride, H, (int)p.rev, acc, P1, P2)
  if (p.form == plan::kSgmSheared) {
    if (p.block <= 512)
      hipLaunchKernelGGL(k_sgm_diag<512>, grid, dim3(p.block), 0, s, b.vol, b.agg, b.vstride, b.astride, D, W, H, p.sx,
                         (int)p.rev, acc, P1, P2);
    else
      hipLaunchKernelGGL(k_sgm_diag<1024>, grid, dim3(p.block), 0, s, b.vol, b.agg, b.vstride, b.astride, D, W, H, p.sx,
                         (int)p.rev, acc, P1, P2);
  } else if (p.waves > 1) {
    SGM_DIAG_LANES(16, true);
  } else if (p.lpl == 8) {
    SGM_DIAG_LANES(8, false);
  } else {
    SGM_DIAG_LANES(16, false);
  }
#undef SGM_DIAG_LANES
  MVS_LAUNCH_CHECK("k_sgm");
  return 0;
}

}  // namespace

int launch_sgm(hipStream_t s, int W, int H, int D, int N, const float* vol, size_t vol_stride, float P1, float P2,
               int paths, float* agg, size_t agg_stride) {
  const long HW = (long)W * H;
  const SgmBatch b{(unsigned)N, vol, vol_stride, agg, agg_stride};
  // 16-byte pieces: vol and agg equal mod 16 bytes in every element of the batch, else the scalar form for all
  const bool vec_ok = plan::sgm_batch_vec_ok(N, (uintptr_t)vol, vol_stride, (uintptr_t)agg, agg_stride);
  int acc = 0;  // the first set path stores, the later ones add
  for (int path = 0; path < 4; path++) {
    if (!((paths >> path) & 1)) continue;
    const plan::SgmPlan p = plan::plan_sgm(W, H, D, path);
    if (p.err) return arg_fail(p.err);
    if (p.form == plan::kSgmColumns) {
      if (p.block <= 512)
        hipLaunchKernelGGL(k_sgm_columns<512>, dim3(p.grid, b.N), dim3(p.block), 0, s, vol, agg, vol_stride, agg_stride,
                           D, W, H, (int)p.rev, acc, P1, P2);
      else
        hipLaunchKernelGGL(k_sgm_columns<1024>, dim3(p.grid, b.N), dim3(p.block), 0, s, vol, agg, vol_stride,
                           agg_stride, D, W, H, (int)p.rev, acc, P1, P2);
    } else if (p.waves > 1) {
      launch_lanes<false, true>(s, p, b, D, HW, acc, P1, P2);
    } else if (p.vec && vec_ok) {
      launch_lanes<true, false>(s, p, b, D, HW, acc, P1, P2);
    } else {
      launch_lanes<false, false>(s, p, b, D, HW, acc, P1, P2);
    }
    MVS_LAUNCH_CHECK("k_sgm");
    acc = 1;
  }
  for (int path = 4; path < 8; path++) {
    if (!((paths >> path) & 1)) continue;
    if (const int rc = launch_diag(s, W, H, D, b, P1, P2, path, acc)) return rc;
    acc = 1;
  }
  return 0;
}

}  // namespace mvs
