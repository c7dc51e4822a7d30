// Semi-global aggregation on 16-bit integer costs (include/mvs.h at mvs_quant_u16_d, mvs_sgm8_u16_batch_d and
// mvs_wta_u16_d; tests/sgm16_ref.py): the recurrence, the eight paths and the kernel forms of sgm.hip with
// uint16 in memory and exact integer arithmetic.
//
// Definition, integers.  q is the pixel before p on the path:
//   first pixel:  L(p, d) = vol[d][p]
//   else:  m = min_k L(q, k)
//          t = min(L(q, d), L(q, d-1) + P1 (d > 0), L(q, d+1) + P1 (d < D-1), m + P2)
//          L(p, d) = vol[d][p] + t - m
//   agg = the sum of L over the set bits of `paths`: exact, so the order plays no part.  One launch per path all
//   the same, the first stores L, the others add to agg (fusing paths is what the exact sum leaves open).
// With vol <= 4094 and 0 <= P1 <= P2 <= 4095: t <= m + P2, so L <= vol + P2 <= 8189, and eight paths sum to at
// most 65512: nothing wraps 16 bits.  In registers everything is int32.  A level that does not exist (d-1 at 0,
// d+1 at D-1, the padding up to a lane's or a wave's level count, a column past the image) is a state of
// kInf = 2^28: kInf + P1 drops out of every minimum that has a real member, kInf + kInf - kInf and kInf + P2 stay
// far below 2^31, and such a state is never stored.  With costs above 4094 (a broken precondition) the values
// are unspecified; every address comes from the dimensions alone, and a stored value is cut to 16 bits.
//
// The forms (launch_plan.h at plan_sgm, plan_sgm_diag and plan_sgm16_batch; D <= 256):
//  * k_sgm16_lanes, horizontal paths: lanes over levels, one wave per row, 1, 2 or 4 levels per lane, the minimum
//    by DPP and four lane reads, one shuffle per side.  VEC reads vol and reads-modifies-writes agg in aligned
//    16-byte pieces of EIGHT pixels; every (lane, level) has its own phase ph = (address of the line's first
//    element / 2) mod 8: pixel x is element j = (x + ph) mod 8 of the piece of pixels x - j .. x - j + 7.  A piece
//    inside the line is loaded when the walk enters it and, complete, stored one step later behind that step's
//    loads; the pixels of a piece that crosses an end of the line go one by one (2-byte accesses).  Without VEC
//    (vol and agg not equally aligned mod 16 bytes somewhere in the batch) every access is 2 bytes.
//  * k_sgm16_columns, vertical paths: lanes over 64 consecutive columns, levels 16 per wave, {chunk minimum,
//    first, last} through double-buffered LDS, one barrier per row, the next row's loads issued before the barrier
//    and before this row's stores.  One column per lane: a wave's row piece is 128 bytes.  Two adjacent columns
//    per lane (one dword, 256 bytes) were not taken: a row's first element is 2-byte aligned only (W and the
//    plane pitch may be odd), so the pairs would need a phase per (row, level) with single pixels at both ends,
//    and two columns of 16 levels with the row in flight behind them are 160 values per lane, above the 128
//    registers of the 1,024-thread instantiation.  Not measured against each other.
//  * k_sgm16_diag, diagonal paths: the columns form with its band moving one column per row; clamped in-bounds
//    loads with no lane-dependent select around or behind a load, the `was` flag for a lane's first live row, row
//    ranges uniform over the workgroup (sgm.hip at k_sgm_diag).
// Every form takes the batch on blockIdx.y.  Plane bases are 64-bit, offsets within a plane 32-bit.
//
// k_quant_u16 and k_wta_u16 are the streaming passes before and behind: float32 costs -> uint16, and the winner
// with its confidence from a uint16 aggregate.  k_wta_u16_sub is that winner pass with the sub-level fit through the
// raw (quantised, not aggregated) costs at the winner.
#include "mvs_internal.h"
#include "wave.h"
#include "wta_common.h"

namespace mvs {
namespace {

constexpr int kInf = 1 << 28;

template <int CTRL>
__device__ __forceinline__ int dpp_min_i(int v) {
  return min(v, __builtin_amdgcn_update_dpp(v, v, CTRL, 0xf, 0xf, false));
}

// the minimum over the 64 lanes, in every lane (all lanes active)
__device__ __forceinline__ int wave_min_i(int v) {
  v = dpp_min_i<0xB1>(v);   // quad_perm [1,0,3,2]
  v = dpp_min_i<0x4E>(v);   // quad_perm [2,3,0,1]
  v = dpp_min_i<0x141>(v);  // row_half_mirror: the other quad of the 8
  v = dpp_min_i<0x140>(v);  // row_mirror: the other half of the row of 16
  const int r0 = __builtin_amdgcn_readlane(v, 0), r1 = __builtin_amdgcn_readlane(v, 16);
  const int r2 = __builtin_amdgcn_readlane(v, 32), r3 = __builtin_amdgcn_readlane(v, 48);
  return min(min(r0, r1), min(r2, r3));
}

// element j (0..7) of a piece of eight uint16
__device__ __forceinline__ int pick16(const u32x4& v, int j) {
  const int w = j >> 1;
  const unsigned d = w == 0 ? v.x : w == 1 ? v.y : w == 2 ? v.z : v.w;
  return (int)((d >> ((j & 1) * 16)) & 0xffffu);
}
__device__ __forceinline__ void put16(u32x4& v, int j, int s) {
  const int w = j >> 1, sh = (j & 1) * 16;
  const unsigned keep = ~(0xffffu << sh), val = ((unsigned)s & 0xffffu) << sh;
  v.x = w == 0 ? (v.x & keep) | val : v.x;
  v.y = w == 1 ? (v.y & keep) | val : v.y;
  v.z = w == 2 ? (v.z & keep) | val : v.z;
  v.w = w == 3 ? (v.w & keep) | val : v.w;
}

// One step of NL consecutive levels: L(q, .) in L -> L(p, .); up, dn = L(q, .) of the level below the first and
// above the last (kInf: none).
template <int NL>
__device__ __forceinline__ void sgm16_step(int (&L)[NL], const int (&c)[NL], int up, int dn, int m, int P1, int P2) {
  const int mp2 = m + P2;
  int prev = up;
#pragma unroll
  for (int k = 0; k < NL; k++) {
    const int cur = L[k], nxt = k + 1 < NL ? L[k + 1] : dn;
    const int t = min(min(cur, prev + P1), min(nxt + P1, mp2));
    L[k] = c[k] + t - m;
    prev = cur;
  }
}

// Row blockIdx.x of every level's plane, n = W pixels; the lane's levels are d0 .. d0 + LPL - 1.
template <int LPL, bool VEC>
__global__ __launch_bounds__(64) void k_sgm16_lanes(const uint16_t* __restrict__ vol, uint16_t* __restrict__ agg,
                                                    size_t vstride, size_t astride, int D, long HW, int n,
                                                    int lstride, int rev, int acc, int P1, int P2) {
  vol += (size_t)blockIdx.y * vstride;  // the batch element: 64-bit, before anything is derived from the bases
  agg += (size_t)blockIdx.y * astride;
  const int lane = threadIdx.x & 63;
  const int d0 = (int)threadIdx.x * LPL;  // levels >= D are padding and touch no memory
  const long base = (long)d0 * HW + (long)((unsigned)blockIdx.x * (unsigned)lstride);
  const uint16_t* vp = vol + base;
  uint16_t* ap = agg + base;
  const int jl = rev ? 7 : 0, js = rev ? 0 : 7;  // the element at which the walk enters / leaves a piece
  int L[LPL];
  u32x4 cv[LPL], av[LPL], pv[LPL];  // the piece of vol, of agg, and the completed piece of agg waiting to be stored
  int ph[LPL], pxs[LPL];            // pxs: where pv goes (-1: nothing waits)
#pragma unroll
  for (int k = 0; k < LPL; k++) {
    L[k] = kInf;
    cv[k] = av[k] = pv[k] = u32x4{0u, 0u, 0u, 0u};
    pxs[k] = -1;
    ph[k] = VEC ? plan::sgm16_phase((uintptr_t)(vp + (long)k * HW)) : 0;  // (vol and agg: equal mod 16 bytes)
  }
  for (int i = 0; i < n; i++) {
    const int x = rev ? n - 1 - i : i;
    int c[LPL];
    if (VEC) {
      // the pieces this step enters, every level's before anything waits for one
#pragma unroll
      for (int k = 0; k < LPL; k++) {
        const int j = plan::sgm16_piece_elem(ph[k], x), xs = x - j;
        if (d0 + k < D && j == jl && plan::sgm16_piece_inside(ph[k], x, n)) {
          cv[k] = *(const u32x4*)(vp + (long)k * HW + xs);
          if (acc) av[k] = *(const u32x4*)(ap + (long)k * HW + xs);
        }
      }
      // then the pieces the last step completed, behind the loads
#pragma unroll
      for (int k = 0; k < LPL; k++) {
        if (pxs[k] >= 0) {
          *(u32x4*)(ap + (long)k * HW + pxs[k]) = pv[k];
          pxs[k] = -1;
        }
      }
    }
#pragma unroll
    for (int k = 0; k < LPL; k++) {
      c[k] = kInf;
      if (d0 + k < D) {
        const uint16_t* r = vp + (long)k * HW;
        if (VEC) {
          const int j = plan::sgm16_piece_elem(ph[k], x);
          c[k] = plan::sgm16_piece_inside(ph[k], x, n) ? pick16(cv[k], j) : (int)r[x];
        } else {
          c[k] = (int)r[x];
        }
      }
    }
    if (i == 0) {
#pragma unroll
      for (int k = 0; k < LPL; k++) L[k] = c[k];
    } else {
      int m = L[0];
#pragma unroll
      for (int k = 1; k < LPL; k++) m = min(m, L[k]);
      m = wave_min_i(m);
      int up = __shfl_up(L[LPL - 1], 1), dn = __shfl_down(L[0], 1);
      if (lane == 0) up = kInf;
      if (lane == 63) dn = kInf;
      sgm16_step<LPL>(L, c, up, dn, m, P1, P2);
    }
#pragma unroll
    for (int k = 0; k < LPL; k++) {
      if (d0 + k < D) {
        uint16_t* r = ap + (long)k * HW;
        if (VEC) {
          const int j = plan::sgm16_piece_elem(ph[k], x), xs = x - j;
          if (plan::sgm16_piece_inside(ph[k], x, n)) {
            put16(av[k], j, acc ? pick16(av[k], j) + L[k] : L[k]);
            if (j == js) {  // the piece is complete: stored at the next step, after that step's loads
              pv[k] = av[k];
              pxs[k] = xs;
            }
          } else {
            r[x] = (uint16_t)(acc ? (int)r[x] + L[k] : L[k]);
          }
        } else {
          r[x] = (uint16_t)(acc ? (int)r[x] + L[k] : L[k]);
        }
      }
    }
  }
  if (VEC) {
#pragma unroll
    for (int k = 0; k < LPL; k++)
      if (pxs[k] >= 0) *(u32x4*)(ap + (long)k * HW + pxs[k]) = pv[k];
  }
}

constexpr int LPW = plan::kSgmColumnsLpw;

// NT: the workgroup's thread limit (512 up to 8 waves: 128 levels)
template <int NT>
__global__ __launch_bounds__(NT) void k_sgm16_columns(const uint16_t* __restrict__ vol, uint16_t* __restrict__ agg,
                                                      size_t vstride, size_t astride, int D, int W, int H, int rev,
                                                      int acc, int P1, int P2) {
  vol += (size_t)blockIdx.y * vstride;  // the batch element
  agg += (size_t)blockIdx.y * astride;
  __shared__ int ex[2][NT / 64][3][64];  // per wave and column: {chunk minimum, first level, last level}
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const int x = blockIdx.x * 64 + lane;
  const bool in = x < W;  // a column past the image: kInf throughout, read and stored nowhere
  const long HW = (long)W * H;
  const int dw = w * LPW;
  const uint16_t* vw = vol + (long)dw * HW;
  uint16_t* aw = agg + (long)dw * HW;
  int L[LPW], c[LPW], a[LPW];
  const auto load = [&](const uint16_t* pl, int y, int(&cc)[LPW], int pad) {
    const int off = y * W + x;
#pragma unroll
    for (int k = 0; k < LPW; k++) {
      cc[k] = pad;
      if (in && dw + k < D) cc[k] = (int)pl[(long)k * HW + off];
    }
  };
  const int dy = rev ? -1 : 1;
  int y = rev ? H - 1 : 0;
  load(vw, y, c, kInf);
  if (acc) load(aw, y, a, 0);
  for (int i = 0; i < H; i++, y += dy) {
    // the next row's costs and agg are on their way while the waves meet, and are issued before this row's stores
    int cn[LPW], an[LPW];
    if (i + 1 < H) {
      load(vw, y + dy, cn, kInf);
      if (acc) load(aw, y + dy, an, 0);
    }
    if (i == 0) {
#pragma unroll
      for (int k = 0; k < LPW; k++) L[k] = c[k];
    } else {
      const int par = i & 1;
      int m = L[0];
#pragma unroll
      for (int k = 1; k < LPW; k++) m = min(m, L[k]);
      ex[par][w][0][lane] = m;
      ex[par][w][1][lane] = L[0];
      ex[par][w][2][lane] = L[LPW - 1];
      // a wave writes buffer par again two rows on, past the next barrier: every wave has read this one by then
      __syncthreads();
      m = ex[par][0][0][lane];
      for (int v = 1; v < nw; v++) m = min(m, ex[par][v][0][lane]);
      const int up = w > 0 ? ex[par][w - 1][2][lane] : kInf;
      const int dn = w + 1 < nw ? ex[par][w + 1][1][lane] : kInf;
      sgm16_step<LPW>(L, c, up, dn, m, P1, P2);
    }
    const int off = y * W + x;
#pragma unroll
    for (int k = 0; k < LPW; k++)
      if (in && dw + k < D) aw[(long)k * HW + off] = (uint16_t)(acc ? a[k] + L[k] : L[k]);
    if (i + 1 < H) {
#pragma unroll
      for (int k = 0; k < LPW; k++) {
        c[k] = cn[k];
        if (acc) a[k] = an[k];
      }
    }
  }
}

// k_sgm16_columns, sheared: lane `lane` of workgroup g follows one diagonal line, at image row y on column
// x0 + sx y, live there iff that lies in [0, W) (sgm.hip at k_sgm_diag).
template <int NT>
__global__ __launch_bounds__(NT) void k_sgm16_diag(const uint16_t* __restrict__ vol, uint16_t* __restrict__ agg,
                                                   size_t vstride, size_t astride, int D, int W, int H, int sx, int rev,
                                                   int acc, int P1, int P2) {
  vol += (size_t)blockIdx.y * vstride;  // the batch element
  agg += (size_t)blockIdx.y * astride;
  __shared__ int ex[2][NT / 64][3][64];  // per wave and line: {chunk minimum, first level, last level}
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const int g = blockIdx.x;
  const int x0 = plan::sgm_diag_x0(g, lane, H, sx);
  const int ylo = plan::sgm_diag_ylo(g, W, H, sx), n = plan::sgm_diag_yhi(g, W, H, sx) - ylo + 1;
  const long HW = (long)W * H;
  const int dw = w * LPW;
  const uint16_t* vw = vol + (long)dw * HW;
  uint16_t* aw = agg + (long)dw * HW;
  int L[LPW], c[LPW], a[LPW];
  // Row y's own column; a lane outside the image reads the row's nearest pixel instead of nothing: what it holds
  // is never stored and never reaches a live state (`was` below), and no lane-dependent condition stands around
  // or behind a load
  const auto load = [&](const uint16_t* pl, int y, int(&cc)[LPW], int pad) {
    const int off = y * W + min(max(x0 + sx * y, 0), W - 1);
#pragma unroll
    for (int k = 0; k < LPW; k++) {
      cc[k] = pad;
      if (dw + k < D) cc[k] = (int)pl[(long)k * HW + off];
    }
  };
  const int dy = rev ? -1 : 1;
  int y = rev ? ylo + n - 1 : ylo;
  bool was = false;  // the lane was live on the row before: this row steps from it
  load(vw, y, c, kInf);
  if (acc) load(aw, y, a, 0);
  for (int i = 0; i < n; i++, y += dy) {
    // as in k_sgm16_columns: the next row's loads before the waves meet and before this row's stores
    int cn[LPW], an[LPW];
    if (i + 1 < n) {
      load(vw, y + dy, cn, kInf);
      if (acc) load(aw, y + dy, an, 0);
    }
    const int x = x0 + sx * y;
    const bool in = x >= 0 && x < W;
    if (i > 0) {  // (on the first row no lane has a pixel before it)
      const int par = i & 1;
      int m = L[0];
#pragma unroll
      for (int k = 1; k < LPW; k++) m = min(m, L[k]);
      ex[par][w][0][lane] = m;
      ex[par][w][1][lane] = L[0];
      ex[par][w][2][lane] = L[LPW - 1];
      // a wave writes buffer par again two rows on, past the next barrier: every wave has read this one by then
      __syncthreads();
      m = ex[par][0][0][lane];
      for (int v = 1; v < nw; v++) m = min(m, ex[par][v][0][lane]);
      const int up = w > 0 ? ex[par][w - 1][2][lane] : kInf;
      const int dn = w + 1 < nw ? ex[par][w + 1][1][lane] : kInf;
      sgm16_step<LPW>(L, c, up, dn, m, P1, P2);
    }
#pragma unroll
    for (int k = 0; k < LPW; k++) L[k] = was ? L[k] : c[k];
    was = in;
    const int off = y * W + x;
#pragma unroll
    for (int k = 0; k < LPW; k++)
      if (in && dw + k < D) aw[(long)k * HW + off] = (uint16_t)(acc ? a[k] + L[k] : L[k]);
    if (i + 1 < n) {
#pragma unroll
      for (int k = 0; k < LPW; k++) {
        c[k] = cn[k];
        if (acc) a[k] = an[k];
      }
    }
  }
}

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
// the 4 smallest (cost, level) of one pixel in lexicographic order: the first is the first index of the minimum,
// and the smallest cost at a level more than one away from it is among the other three (at most two are adjacent)
struct Top4u {
  int v0 = kInf, v1 = kInf, v2 = kInf, v3 = kInf;
  int i0 = -1, i1 = -1, i2 = -1, i3 = -1;
  __device__ __forceinline__ void insert(int cc, int ci) {
    if (cc < v3) {
      if (cc < v2) {
        v3 = v2; i3 = i2;
        if (cc < v1) {
          v2 = v1; i2 = i1;
          if (cc < v0) { v1 = v0; i1 = i0; v0 = cc; i0 = ci; }
          else { v1 = cc; i1 = ci; }
        } else { v2 = cc; i2 = ci; }
      } else { v3 = cc; i3 = ci; }
    }
  }
  __device__ __forceinline__ void emit(const float* levels, float* disp, float* conf, long p) const {
    disp[p] = levels[i0];  // (D >= 1 and every cost is below kInf: i0 >= 0)
    if (conf) {
      int c2 = -1;
      if (i1 >= 0 && (i1 < i0 - 1 || i1 > i0 + 1)) c2 = v1;
      else if (i2 >= 0 && (i2 < i0 - 1 || i2 > i0 + 1)) c2 = v2;
      else if (i3 >= 0 && (i3 < i0 - 1 || i3 > i0 + 1)) c2 = v3;
      conf[p] = c2 < 0 ? 0.0f : (float)(c2 - v0) / 2047.0f;
    }
  }
};

// One lane per NP consecutive pixels, UNR levels in flight.  NP = 4 (8-byte loads) needs the plane pitch P a
// multiple of 4 and agg 8-byte aligned; NP = 1 takes everything else.
template <int NP, int UNR>
__global__ __launch_bounds__(256) void k_wta_u16(const uint16_t* __restrict__ agg, const float* __restrict__ levels,
                                                 long P, int D, float* __restrict__ disp, float* __restrict__ conf) {
  typedef unsigned short vec __attribute__((ext_vector_type(NP)));
  const long p = (blockIdx.x * (long)blockDim.x + threadIdx.x) * NP;
  if (p >= P) return;
  Top4u t[NP];
  int dl = 0;
  if constexpr (NP == 1) {
    const uint16_t* col = agg + p;
    for (; dl + UNR <= D; dl += UNR) {
      int c[UNR];
#pragma unroll
      for (int u = 0; u < UNR; u++) c[u] = (int)__builtin_nontemporal_load(col + (long)(dl + u) * P);
#pragma unroll
      for (int u = 0; u < UNR; u++) t[0].insert(c[u], dl + u);
    }
    for (; dl < D; dl++) t[0].insert((int)col[(long)dl * P], dl);
  } else {
    const vec* col = (const vec*)(agg + p);
    const long Pv = P / NP;
    for (; dl + UNR <= D; dl += UNR) {
      vec c[UNR];
#pragma unroll
      for (int u = 0; u < UNR; u++) c[u] = __builtin_nontemporal_load(col + (long)(dl + u) * Pv);
#pragma unroll
      for (int u = 0; u < UNR; u++)
#pragma unroll
        for (int k = 0; k < NP; k++) t[k].insert((int)c[u][k], dl + u);
    }
    for (; dl < D; dl++) {
      const vec c = col[(long)dl * Pv];
#pragma unroll
      for (int k = 0; k < NP; k++) t[k].insert((int)c[k], dl);
    }
  }
#pragma unroll
  for (int k = 0; k < NP; k++) t[k].emit(levels, disp, conf, p + k);
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
  typedef unsigned short vec __attribute__((ext_vector_type(NP)));
  const long p = (blockIdx.x * (long)blockDim.x + threadIdx.x) * NP;
  if (p >= P) return;
  Top4u t[NP];
  int dl = 0;
  if constexpr (NP == 1) {
    const uint16_t* col = agg + p;
    for (; dl + UNR <= D; dl += UNR) {
      int c[UNR];
#pragma unroll
      for (int u = 0; u < UNR; u++) c[u] = (int)__builtin_nontemporal_load(col + (long)(dl + u) * P);
#pragma unroll
      for (int u = 0; u < UNR; u++) t[0].insert(c[u], dl + u);
    }
    for (; dl < D; dl++) t[0].insert((int)col[(long)dl * P], dl);
  } else {
    const vec* col = (const vec*)(agg + p);
    const long Pv = P / NP;
    for (; dl + UNR <= D; dl += UNR) {
      vec c[UNR];
#pragma unroll
      for (int u = 0; u < UNR; u++) c[u] = __builtin_nontemporal_load(col + (long)(dl + u) * Pv);
#pragma unroll
      for (int u = 0; u < UNR; u++)
#pragma unroll
        for (int k = 0; k < NP; k++) t[k].insert((int)c[u][k], dl + u);
    }
    for (; dl < D; dl++) {
      const vec c = col[(long)dl * Pv];
#pragma unroll
      for (int k = 0; k < NP; k++) t[k].insert((int)c[k], dl);
    }
  }
  // conf first: from here on only the winners' indices stay live beside the gathered values
  if (conf) {
#pragma unroll
    for (int k = 0; k < NP; k++) {
      const Top4u& q = t[k];
      const int c2 = second_cost(q.i0, q.i1, q.v1, q.i2, q.v2, q.i3, q.v3, -1);
      conf[p + k] = c2 < 0 ? 0.0f : (float)(c2 - q.v0) / 2047.0f;
    }
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
  const long HW = (long)W * H;
  const dim3 gy(1, (unsigned)N);
  // 16-byte pieces: vol and agg equal mod 16 bytes in every element of the batch, else the 2-byte form for all
  const bool vec_ok = plan::sgm16_batch_vec_ok(N, (uintptr_t)vol, vol_stride, (uintptr_t)agg, agg_stride);
  int acc = 0;  // the first set path stores, the later ones add
  for (int path = 0; path < 4; path++) {
    if (!((paths >> path) & 1)) continue;
    const plan::SgmPlan p = plan::plan_sgm(W, H, D, path);
    if (p.err) return arg_fail(p.err);
    const dim3 grid(p.grid, gy.y), block(p.block);
    if (p.form == plan::kSgmColumns) {
      if (p.block <= 512)
        hipLaunchKernelGGL(k_sgm16_columns<512>, grid, block, 0, s, vol, agg, vol_stride, agg_stride, D, W, H,
                           (int)p.rev, acc, P1, P2);
      else
        hipLaunchKernelGGL(k_sgm16_columns<1024>, grid, block, 0, s, vol, agg, vol_stride, agg_stride, D, W, H,
                           (int)p.rev, acc, P1, P2);
    } else {  // D <= 256: one wave, 1, 2 or 4 levels per lane
#define SGM16_LANES(LPL, VEC)                                                                                      \
  hipLaunchKernelGGL((k_sgm16_lanes<LPL, VEC>), grid, block, 0, s, vol, agg, vol_stride, agg_stride, D, HW, p.n, \
                     p.lstride, (int)p.rev, acc, P1, P2)
      if (p.waves != 1 || p.lpl > 4 || p.sstride != 1) return arg_fail("sgm16: no kernel form for this plan");
      if (p.vec && vec_ok) {
        if (p.lpl == 1) SGM16_LANES(1, true);
        else if (p.lpl == 2) SGM16_LANES(2, true);
        else SGM16_LANES(4, true);
      } else {
        if (p.lpl == 1) SGM16_LANES(1, false);
        else if (p.lpl == 2) SGM16_LANES(2, false);
        else SGM16_LANES(4, false);
      }
#undef SGM16_LANES
    }
    MVS_LAUNCH_CHECK("k_sgm16");
    acc = 1;
  }
  for (int path = 4; path < 8; path++) {
    if (!((paths >> path) & 1)) continue;
    const plan::SgmDiagPlan p = plan::plan_sgm_diag(W, H, D, path);
    if (p.err) return arg_fail(p.err);
    if (p.form != plan::kSgmSheared) return arg_fail("sgm16: no kernel form for this plan");
    const dim3 grid(p.grid, gy.y), block(p.block);
    if (p.block <= 512)
      hipLaunchKernelGGL(k_sgm16_diag<512>, grid, block, 0, s, vol, agg, vol_stride, agg_stride, D, W, H, p.sx,
                         (int)p.rev, acc, P1, P2);
    else
      hipLaunchKernelGGL(k_sgm16_diag<1024>, grid, block, 0, s, vol, agg, vol_stride, agg_stride, D, W, H, p.sx,
                         (int)p.rev, acc, P1, P2);
    MVS_LAUNCH_CHECK("k_sgm16");
    acc = 1;
  }
  return 0;
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
