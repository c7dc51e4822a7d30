// Semi-global aggregation of a cost volume vol [D][H][W] along the four axis-aligned paths (include/mvs.h at
// mvs_sgm_d; tests/sgm_ref.py) and the four diagonal ones (mvs_sgm8_d): the kernels, once, for both cost types.
// sgm.hip instantiates them on float32 costs, sgm16.hip on 16-bit integer costs (mvs_sgm8_u16_batch_d;
// tests/sgm16_ref.py).
//
// Definition.  q is the pixel before p on the path:
//   first pixel:  L(p, d) = vol[d][p]
//   else:  m = min_k L(q, k)
//          t = min(L(q, d), L(q, d-1) + P1 (d > 0), L(q, d+1) + P1 (d < D-1), m + P2)
//          L(p, d) = (vol[d][p] + t) - m
//   agg = ((L_b0 + L_b1) + L_b2) + L_b3 ... over the set bits of `paths`, in bit order: one launch per path, the
//   first stores L, the others add to agg.
// A level that does not exist (d-1 at 0, d+1 at D-1, the padding up to a lane's or a wave's level count, a column
// past the image) is the cost type's absent state; it drops out of every minimum that has a real member and is
// never stored.
//  * float32 (SgmF32): every operation rounded (there is no multiply, so nothing can fuse), the sums in the order
//    written above.  Absent is +inf: inf + P1 drops out of the minimum, and a padded level's own L stays +inf (m
//    is finite, no NaN arises; a column past the image is NaN from the second row on).
//  * integers (SgmU16): uint16 in memory, int32 in registers, exact, so the order of the sums plays no part
//    (fusing paths is what the exact sum leaves open).  With vol <= 4094 and 0 <= P1 <= P2 <= 4095: t <= m + P2,
//    so L <= vol + P2 <= 8189, and eight paths sum to at most 65512: nothing wraps 16 bits.  Absent is
//    kInf = 2^28: kInf + P1 drops out, kInf + kInf - kInf and kInf + P2 stay far below 2^31.  With costs above
//    4094 (a broken precondition) the values are unspecified; every address comes from the dimensions alone, and
//    a stored value is cut to 16 bits.
//
// The layout decides the forms (launch_plan.h at plan_sgm and plan_sgm_diag):
//  * k_sgm_lanes: lanes over levels, one workgroup per line.  A lane keeps LPL consecutive levels of L(q, .) in
//    registers, so d-1 and d+1 cross a lane boundary once per side (one shuffle each) and m is an in-wave
//    reduction (DPP within the rows of 16 lanes, then four lane reads): no LDS and no barrier up to 1024 levels.
//    Above, the workgroup's waves leave {minimum, first, last} in LDS, double-buffered: one barrier per step.
//    Along x a level's consecutive pixels are contiguous: VEC reads vol and reads-modifies-writes agg in aligned
//    16-byte pieces of 4 floats or 8 uint16.  Which pixels share a piece depends on the level (the plane pitch
//    H W need not be a multiple of the piece) and on the row, so every (lane, level) has its own phase
//    (launch_plan.h at sgm_piece_phase).  A piece inside the line is loaded when the walk enters it; when the walk
//    leaves it, it is complete and is stored one step later, behind that step's loads (memory operations retire
//    in order: a load issued behind a store waits for the store as well).  The pixels of a piece that crosses an
//    end of the line are read and written one by one (the scalar head and tail).  Without VEC (vol and agg not
//    equally aligned mod 16 bytes somewhere in the batch, or a strided line) every access is one element.
//  * k_sgm_columns: vertical paths at D <= 256.  Lanes over levels would read one element per plane there, so the
//    lanes lie over 64 consecutive columns (a level's row piece is one coalesced 256 or 128 bytes) and the levels
//    are split over the waves, 16 per wave, unrolled in registers.  Per row the waves exchange {chunk minimum,
//    first, last} per column through LDS, double-buffered: one barrier per row.  The next row's costs and agg
//    are loaded before the waves meet and before this row's stores.
//    uint16 has one column per lane as well.  Two adjacent columns per lane (one dword, 256 bytes) were not
//    taken: a row's first element is 2-byte aligned only (W and the plane pitch may be odd), so the pairs would
//    need a phase per (row, level) with single pixels at both ends, and two columns of 16 levels with the row in
//    flight behind them are 160 values per lane, above the 128 registers of the 1,024-thread instantiation.  Not
//    measured against each other.
//  * k_sgm_diag: the four diagonal paths of mvs_sgm8_d (bits 4..7: steps (+1, +1), (-1, -1), (-1, +1), (+1, -1)
//    per pixel; tests/sgm8_ref.py) at D <= 256: k_sgm_columns with its band of 64 columns moving by one column
//    per row, so that a lane follows one diagonal line and its state never leaves the lane.  A level's row piece
//    is still coalesced; its start moves by one element per row and is not aligned.  Above 256 levels a diagonal
//    line is a strided line of k_sgm_lanes (DIAG), one workgroup per line, elements W + 1 or W - 1 apart.
// Plane bases are 64-bit, offsets within a plane 32-bit (W H <= 2^27).
// The forms above 256 levels (more than 4 levels per lane, several waves, DIAG) exist for float32 only.
//
// Every form takes N volumes of one shape per launch (mvs_sgm8_batch_d): the batch index is blockIdx.y, and a
// kernel first moves its two bases to its element (blockIdx.y * stride, 64-bit); nothing else knows of the batch.
// The single-volume entry points launch with N = 1.
#pragma once
#include <type_traits>

#include "mvs_internal.h"
#include "wave.h"

namespace mvs {
namespace {

// ---- the two cost types -------------------------------------------------------------------------
// Mem in memory, Reg in registers; a 16-byte Piece of kPiece pixels with pick / put of element j and the zero
// piece (float4{} instead sent the float32 lanes kernels' pieces to scratch); the absent state (kInf for
// integers, which the uint16 winner passes start from as well), the minimum and the bit cast to and from int
// (DPP, readlane).
struct SgmF32 {
  typedef float Mem;
  typedef float Reg;
  typedef float4 Piece;
  static constexpr int kPiece = 4;
  static __device__ __forceinline__ float4 zero() { return make_float4(0.0f, 0.0f, 0.0f, 0.0f); }
  static __device__ __forceinline__ float inf() { return __builtin_inff(); }
  static __device__ __forceinline__ float min(float a, float b) { return fminf(a, b); }
  static __device__ __forceinline__ int bits(float v) { return __float_as_int(v); }
  static __device__ __forceinline__ float from_bits(int b) { return __int_as_float(b); }
  static __device__ __forceinline__ float pick(const float4& v, int j) {
    return j == 0 ? v.x : j == 1 ? v.y : j == 2 ? v.z : v.w;
  }
  static __device__ __forceinline__ void put(float4& v, int j, float s) {
    v.x = j == 0 ? s : v.x;
    v.y = j == 1 ? s : v.y;
    v.z = j == 2 ? s : v.z;
    v.w = j == 3 ? s : v.w;
  }
};

constexpr int kInf = 1 << 28;
struct SgmU16 {
  typedef uint16_t Mem;
  typedef int Reg;
  typedef u32x4 Piece;
  static constexpr int kPiece = 8;
  static __device__ __forceinline__ u32x4 zero() { return u32x4{0u, 0u, 0u, 0u}; }
  static __device__ __forceinline__ int inf() { return kInf; }
  static __device__ __forceinline__ int min(int a, int b) { return ::min(a, b); }
  static __device__ __forceinline__ int bits(int v) { return v; }
  static __device__ __forceinline__ int from_bits(int b) { return b; }
  static __device__ __forceinline__ int pick(const u32x4& v, int j) {
    const int w = j >> 1;
    const unsigned d = w == 0 ? v.x : w == 1 ? v.y : w == 2 ? v.z : v.w;
    return (int)((d >> ((j & 1) * 16)) & 0xffffu);
  }
  static __device__ __forceinline__ void put(u32x4& v, int j, int s) {
    const int w = j >> 1, sh = (j & 1) * 16;
    const unsigned keep = ~(0xffffu << sh), val = ((unsigned)s & 0xffffu) << sh;
    v.x = w == 0 ? (v.x & keep) | val : v.x;
    v.y = w == 1 ? (v.y & keep) | val : v.y;
    v.z = w == 2 ? (v.z & keep) | val : v.z;
    v.w = w == 3 ? (v.w & keep) | val : v.w;
  }
};

template <class C, int CTRL>
__device__ __forceinline__ typename C::Reg dpp_min(typename C::Reg v) {
  const int b = C::bits(v);
  return C::min(v, C::from_bits(__builtin_amdgcn_update_dpp(b, b, CTRL, 0xf, 0xf, false)));
}

// the minimum over the 64 lanes, in every lane (all lanes active)
template <class C>
__device__ __forceinline__ typename C::Reg wave_min(typename C::Reg v) {
  typedef typename C::Reg R;
  v = dpp_min<C, 0xB1>(v);   // quad_perm [1,0,3,2]
  v = dpp_min<C, 0x4E>(v);   // quad_perm [2,3,0,1]
  v = dpp_min<C, 0x141>(v);  // row_half_mirror: the other quad of the 8
  v = dpp_min<C, 0x140>(v);  // row_mirror: the other half of the row of 16
  const int b = C::bits(v);
  const R r0 = C::from_bits(__builtin_amdgcn_readlane(b, 0)), r1 = C::from_bits(__builtin_amdgcn_readlane(b, 16));
  const R r2 = C::from_bits(__builtin_amdgcn_readlane(b, 32)), r3 = C::from_bits(__builtin_amdgcn_readlane(b, 48));
  return C::min(C::min(r0, r1), C::min(r2, r3));
}

// One step of NL consecutive levels: L(q, .) in L -> L(p, .); up, dn = L(q, .) of the level below the first and
// above the last (absent: none).
template <class C, int NL>
__device__ __forceinline__ void sgm_step(typename C::Reg (&L)[NL], const typename C::Reg (&c)[NL], typename C::Reg up,
                                         typename C::Reg dn, typename C::Reg m, typename C::Reg P1,
                                         typename C::Reg P2) {
  typedef typename C::Reg R;
  const R mp2 = m + P2;
  R prev = up;
#pragma unroll
  for (int k = 0; k < NL; k++) {
    const R cur = L[k], nxt = k + 1 < NL ? L[k + 1] : dn;
    const R t = C::min(C::min(cur, prev + P1), C::min(nxt + P1, mp2));
    L[k] = (c[k] + t) - m;
    prev = cur;
  }
}

// Line blockIdx.x of every level's plane, at blockIdx.x * lstride, n steps; the lane's levels are d0 .. d0 + LPL - 1.
// S is `int` where the launcher has strided lines (the forms above 256 levels: elements sstride apart) and empty
// where every line is contiguous: the kernel then has no such argument.
// DIAG (not VEC): line blockIdx.x of the W + H - 1 diagonal lines with elements sstride = W +- 1 apart; its first
// element and its length come from the line index (plan::sgm_diag_line), and the arguments n and lstride carry W
// and H instead.
template <class C, int LPL, bool VEC, bool MW = false, bool DIAG = false, class... S>
__global__ __launch_bounds__(MW ? 1024 : 64) void k_sgm_lanes(const typename C::Mem* __restrict__ vol,
                                                              typename C::Mem* __restrict__ agg, size_t vstride,
                                                              size_t astride, int D, long HW, int n, S... sstride_,
                                                              int lstride, int rev, int acc, typename C::Reg P1,
                                                              typename C::Reg P2) {
  typedef typename C::Mem M;
  typedef typename C::Reg R;
  typedef typename C::Piece Piece;
  constexpr int PIECE = C::kPiece;
  static_assert(!(DIAG && VEC), "a diagonal line is not contiguous");
  static_assert(!(MW || DIAG) || std::is_same<C, SgmF32>::value, "the forms above 256 levels are float32's");
  static_assert(sizeof...(S) <= 1 && (sizeof...(S) == 1 || !DIAG), "one stride, or none: contiguous lines");
  const int sstride = (1, ..., sstride_);  // the argument, or 1
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
  const M* vp = vol + base;
  M* ap = agg + base;
  const int jl = rev ? PIECE - 1 : 0, js = rev ? 0 : PIECE - 1;  // the element at which the walk enters / leaves a piece
  R L[LPL];
  Piece cv[LPL], av[LPL], pv[LPL];  // the piece of vol, of agg, and the completed piece of agg waiting to be stored
  int ph[LPL], pxs[LPL];            // pxs: where pv goes (-1: nothing waits)
#pragma unroll
  for (int k = 0; k < LPL; k++) {
    L[k] = C::inf();
    cv[k] = av[k] = pv[k] = C::zero();
    pxs[k] = -1;
    ph[k] = VEC ? plan::sgm_piece_phase(PIECE, (uintptr_t)(vp + (long)k * HW)) : 0;  // (vol and agg: equal mod 16 bytes)
  }
  for (int i = 0; i < n; i++) {
    const int x = rev ? n - 1 - i : i;
    R c[LPL];
    if (VEC) {
      // the pieces this step enters, every level's before anything waits for one
#pragma unroll
      for (int k = 0; k < LPL; k++) {
        const int j = plan::sgm_piece_elem(PIECE, ph[k], x), xs = x - j;
        if (d0 + k < D && j == jl && plan::sgm_piece_inside(PIECE, ph[k], x, n)) {
          cv[k] = *(const Piece*)(vp + (long)k * HW + xs);
          if (acc) av[k] = *(const Piece*)(ap + (long)k * HW + xs);
        }
      }
      // then the pieces the last step completed, behind the loads: issued in front of them, the loads' data would
      // wait for these stores as well
#pragma unroll
      for (int k = 0; k < LPL; k++) {
        if (pxs[k] >= 0) {
          *(Piece*)(ap + (long)k * HW + pxs[k]) = pv[k];
          pxs[k] = -1;
        }
      }
    }
#pragma unroll
    for (int k = 0; k < LPL; k++) {
      c[k] = C::inf();
      if (d0 + k < D) {
        const M* r = vp + (long)k * HW;
        if (VEC) {
          const int j = plan::sgm_piece_elem(PIECE, ph[k], x);
          c[k] = plan::sgm_piece_inside(PIECE, ph[k], x, n) ? C::pick(cv[k], j) : (R)r[x];
        } else {
          c[k] = (R)r[x * sstride];
        }
      }
    }
    if (i == 0) {
#pragma unroll
      for (int k = 0; k < LPL; k++) L[k] = c[k];
    } else {
      R m = L[0];
#pragma unroll
      for (int k = 1; k < LPL; k++) m = C::min(m, L[k]);
      m = wave_min<C>(m);
      R up = __shfl_up(L[LPL - 1], 1), dn = __shfl_down(L[0], 1);
      if (lane == 0) up = C::inf();
      if (lane == 63) dn = C::inf();
      if constexpr (MW) {
        __shared__ R ex[2][16][3];  // {minimum, first level, last level} of each wave
        const int par = i & 1, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
        if (lane == 0) {
          ex[par][w][0] = m;
          ex[par][w][1] = L[0];
        }
        if (lane == 63) ex[par][w][2] = L[LPL - 1];
        // a wave writes buffer par again two steps on, past the next barrier: every wave has read this one by then
        __syncthreads();
        m = ex[par][0][0];
        for (int v = 1; v < nw; v++) m = C::min(m, ex[par][v][0]);
        if (lane == 0 && w > 0) up = ex[par][w - 1][2];
        if (lane == 63 && w + 1 < nw) dn = ex[par][w + 1][1];
      }
      sgm_step<C, LPL>(L, c, up, dn, m, P1, P2);
    }
#pragma unroll
    for (int k = 0; k < LPL; k++) {
      if (d0 + k < D) {
        M* r = ap + (long)k * HW;
        if (VEC) {
          const int j = plan::sgm_piece_elem(PIECE, ph[k], x), xs = x - j;
          if (plan::sgm_piece_inside(PIECE, ph[k], x, n)) {
            C::put(av[k], j, acc ? C::pick(av[k], j) + L[k] : L[k]);
            if (j == js) {  // the piece is complete: stored at the next step, after that step's loads
              pv[k] = av[k];
              pxs[k] = xs;
            }
          } else {
            r[x] = (M)(acc ? (R)r[x] + L[k] : L[k]);
          }
        } else {
          const int o = x * sstride;
          r[o] = (M)(acc ? (R)r[o] + L[k] : L[k]);
        }
      }
    }
  }
  if (VEC) {
#pragma unroll
    for (int k = 0; k < LPL; k++)
      if (pxs[k] >= 0) *(Piece*)(ap + (long)k * HW + pxs[k]) = pv[k];
  }
}

constexpr int LPW = plan::kSgmColumnsLpw;

// k_sgm_columns and k_sgm_diag each spell out the per-row exchange through ex.  As one __forceinline__ function of
// both (tried with reference and with value results) it left neither kernel's instruction stream as it is: an
// instruction reordered or dropped in the <512> forms and k_sgm_diag, 32 more instructions in float32's
// k_sgm_columns<1024>.

// NT: the workgroup's thread limit (512 up to 8 waves: 128 levels)
template <class C, int NT>
__global__ __launch_bounds__(NT) void k_sgm_columns(const typename C::Mem* __restrict__ vol,
                                                    typename C::Mem* __restrict__ agg, size_t vstride, size_t astride,
                                                    int D, int W, int H, int rev, int acc, typename C::Reg P1,
                                                    typename C::Reg P2) {
  typedef typename C::Mem M;
  typedef typename C::Reg R;
  vol += (size_t)blockIdx.y * vstride;  // the batch element
  agg += (size_t)blockIdx.y * astride;
  __shared__ R ex[2][NT / 64][3][64];  // per wave and column: {chunk minimum, first level, last level}
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const int x = blockIdx.x * 64 + lane;
  const bool in = x < W;  // a column past the image: absent, read and stored nowhere
  const long HW = (long)W * H;
  const int dw = w * LPW;
  const M* vw = vol + (long)dw * HW;
  M* aw = agg + (long)dw * HW;
  R L[LPW], c[LPW], a[LPW];
  const auto load = [&](const M* pl, int y, R(&cc)[LPW], R pad) {
    const int off = y * W + x;
#pragma unroll
    for (int k = 0; k < LPW; k++) {
      cc[k] = pad;
      if (in && dw + k < D) cc[k] = (R)pl[(long)k * HW + off];
    }
  };
  const int dy = rev ? -1 : 1;
  int y = rev ? H - 1 : 0;
  load(vw, y, c, C::inf());
  if (acc) load(aw, y, a, 0);
  for (int i = 0; i < H; i++, y += dy) {
    // the next row's costs and agg are on their way while the waves meet, and are issued before this row's
    // stores: memory operations retire in order, so a load issued behind a store waits for the store as well
    R cn[LPW], an[LPW];
    if (i + 1 < H) {
      load(vw, y + dy, cn, C::inf());
      if (acc) load(aw, y + dy, an, 0);
    }
    if (i == 0) {
#pragma unroll
      for (int k = 0; k < LPW; k++) L[k] = c[k];
    } else {
      const int par = i & 1;
      R m = L[0];
#pragma unroll
      for (int k = 1; k < LPW; k++) m = C::min(m, L[k]);
      ex[par][w][0][lane] = m;
      ex[par][w][1][lane] = L[0];
      ex[par][w][2][lane] = L[LPW - 1];
      // a wave writes buffer par again two rows on, past the next barrier: every wave has read this one by then
      __syncthreads();
      m = ex[par][0][0][lane];
      for (int v = 1; v < nw; v++) m = C::min(m, ex[par][v][0][lane]);
      const R up = w > 0 ? ex[par][w - 1][2][lane] : C::inf();
      const R dn = w + 1 < nw ? ex[par][w + 1][1][lane] : C::inf();
      sgm_step<C, LPW>(L, c, up, dn, m, P1, P2);
    }
    const int off = y * W + x;
#pragma unroll
    for (int k = 0; k < LPW; k++)
      if (in && dw + k < D) aw[(long)k * HW + off] = (M)(acc ? a[k] + L[k] : L[k]);
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
template <class C, int NT>
__global__ __launch_bounds__(NT) void k_sgm_diag(const typename C::Mem* __restrict__ vol,
                                                 typename C::Mem* __restrict__ agg, size_t vstride, size_t astride,
                                                 int D, int W, int H, int sx, int rev, int acc, typename C::Reg P1,
                                                 typename C::Reg P2) {
  typedef typename C::Mem M;
  typedef typename C::Reg R;
  vol += (size_t)blockIdx.y * vstride;  // the batch element
  agg += (size_t)blockIdx.y * astride;
  __shared__ R ex[2][NT / 64][3][64];  // per wave and line: {chunk minimum, first level, last level}
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
  const int g = blockIdx.x;
  const int x0 = plan::sgm_diag_x0(g, lane, H, sx);
  const int ylo = plan::sgm_diag_ylo(g, W, H, sx), n = plan::sgm_diag_yhi(g, W, H, sx) - ylo + 1;
  const long HW = (long)W * H;
  const int dw = w * LPW;
  const M* vw = vol + (long)dw * HW;
  M* aw = agg + (long)dw * HW;
  R L[LPW], c[LPW], a[LPW];
  // Row y's own column.  A lane outside the image reads the row's nearest pixel instead of nothing: what it
  // holds is never stored and never reaches a live state (`was` below), and with no lane-dependent condition
  // around or behind a load nothing waits for one before the row after uses it (a select on `in` behind each
  // load made every load wait for itself: 9.2 ms per path at 1080p, D = 128, float32, against 2.4 ms)
  const auto load = [&](const M* pl, int y, R(&cc)[LPW], R pad) {
    const int off = y * W + min(max(x0 + sx * y, 0), W - 1);
#pragma unroll
    for (int k = 0; k < LPW; k++) {
      cc[k] = pad;
      if (dw + k < D) cc[k] = (R)pl[(long)k * HW + off];
    }
  };
  const int dy = rev ? -1 : 1;
  int y = rev ? ylo + n - 1 : ylo;
  bool was = false;  // the lane was live on the row before: this row steps from it
  load(vw, y, c, C::inf());
  if (acc) load(aw, y, a, 0);
  for (int i = 0; i < n; i++, y += dy) {
    // as in k_sgm_columns: the next row's loads before the waves meet and before this row's stores
    R cn[LPW], an[LPW];
    if (i + 1 < n) {
      load(vw, y + dy, cn, C::inf());
      if (acc) load(aw, y + dy, an, 0);
    }
    const int x = x0 + sx * y;
    const bool in = x >= 0 && x < W;
    if (i > 0) {  // (on the first row no lane has a pixel before it)
      const int par = i & 1;
      R m = L[0];
#pragma unroll
      for (int k = 1; k < LPW; k++) m = C::min(m, L[k]);
      ex[par][w][0][lane] = m;
      ex[par][w][1][lane] = L[0];
      ex[par][w][2][lane] = L[LPW - 1];
      // a wave writes buffer par again two rows on, past the next barrier: every wave has read this one by then
      __syncthreads();
      m = ex[par][0][0][lane];
      for (int v = 1; v < nw; v++) m = C::min(m, ex[par][v][0][lane]);
      const R up = w > 0 ? ex[par][w - 1][2][lane] : C::inf();
      const R dn = w + 1 < nw ? ex[par][w + 1][1][lane] : C::inf();
      sgm_step<C, LPW>(L, c, up, dn, m, P1, P2);
    }
#pragma unroll
    for (int k = 0; k < LPW; k++) L[k] = was ? L[k] : c[k];
    was = in;
    const int off = y * W + x;
#pragma unroll
    for (int k = 0; k < LPW; k++)
      if (in && dw + k < D) aw[(long)k * HW + off] = (M)(acc ? a[k] + L[k] : L[k]);
    if (i + 1 < n) {
#pragma unroll
      for (int k = 0; k < LPW; k++) {
        c[k] = cn[k];
        if (acc) a[k] = an[k];
      }
    }
  }
}

// ---- the eight paths of one call ----------------------------------------------------------------
// The set paths of `paths` in bit order, one launch each: the first stores agg, the later ones add.  N volumes on
// the grid's second axis, element i at vol + i vstride, agg + i astride.  ABOVE256: the forms above
// kSgmColumnsMaxD levels are compiled (lanes with 8 and 16 levels per lane, several waves, strided lines);
// without, a plan that asks for one is refused with `refused`.  `what` names the launches in a HIP error.
template <class C, bool ABOVE256>
int launch_sgm_paths(hipStream_t s, int W, int H, int D, int N, const typename C::Mem* vol, size_t vstride,
                     typename C::Reg P1, typename C::Reg P2, int paths, typename C::Mem* agg, size_t astride,
                     const char* what, const char* refused = nullptr) {
  const long HW = (long)W * H;
  // 16-byte pieces: vol and agg equal mod 16 bytes in every element of the batch, else the scalar form for all
  const bool vec_ok = plan::sgm_piece_vec_ok(C::kPiece, N, (uintptr_t)vol, vstride, (uintptr_t)agg, astride);
  int acc = 0;
  for (int path = 0; path < 8; path++) {
    if (!((paths >> path) & 1)) continue;
    const bool diag = path >= 4;
    const plan::SgmPlan p = diag ? plan::plan_sgm_diag(W, H, D, path) : plan::plan_sgm(W, H, D, path);
    if (p.err) return arg_fail(p.err);
    const dim3 grid(p.grid, (unsigned)N), block(p.block);
    const int rev = (int)p.rev;
// (contiguous lines only: no stride argument)
#define SGM_LANES1(LPL, VEC)                                                                                      \
  hipLaunchKernelGGL((k_sgm_lanes<C, LPL, VEC>), grid, block, 0, s, vol, agg, vstride, astride, D, HW, p.n, p.lstride, \
                     rev, acc, P1, P2)
#define SGM_LANES(LPL, VEC, ...)                                                                                  \
  hipLaunchKernelGGL((k_sgm_lanes<C, LPL, VEC, __VA_ARGS__, int>), grid, block, 0, s, vol, agg, vstride, astride, D, \
                     HW, p.n, p.sstride, p.lstride, rev, acc, P1, P2)
    if (p.form == plan::kSgmColumns) {
      if (p.block <= 512)
        hipLaunchKernelGGL((k_sgm_columns<C, 512>), grid, block, 0, s, vol, agg, vstride, astride, D, W, H, rev, acc, P1,
                           P2);
      else
        hipLaunchKernelGGL((k_sgm_columns<C, 1024>), grid, block, 0, s, vol, agg, vstride, astride, D, W, H, rev, acc,
                           P1, P2);
    } else if (p.form == plan::kSgmSheared) {
      if (p.block <= 512)
        hipLaunchKernelGGL((k_sgm_diag<C, 512>), grid, block, 0, s, vol, agg, vstride, astride, D, W, H, p.sx, rev, acc,
                           P1, P2);
      else
        hipLaunchKernelGGL((k_sgm_diag<C, 1024>), grid, block, 0, s, vol, agg, vstride, astride, D, W, H, p.sx, rev,
                           acc, P1, P2);
    } else if constexpr (!ABOVE256) {  // D <= 256: one wave, 1, 2 or 4 levels per lane, contiguous lines
      if (diag || p.waves != 1 || p.lpl > 4 || p.sstride != 1) return arg_fail(refused);
      if (p.vec && vec_ok) {
        if (p.lpl == 1) SGM_LANES1(1, true);
        else if (p.lpl == 2) SGM_LANES1(2, true);
        else SGM_LANES1(4, true);
      } else {
        if (p.lpl == 1) SGM_LANES1(1, false);
        else if (p.lpl == 2) SGM_LANES1(2, false);
        else SGM_LANES1(4, false);
      }
    } else if (diag) {  // D > 256
      if (p.waves > 1) SGM_LANES(16, false, true, true);
      else if (p.lpl == 8) SGM_LANES(8, false, false, true);
      else SGM_LANES(16, false, false, true);
    } else if (p.waves > 1) {
      SGM_LANES(16, false, true, false);
    } else if (p.vec && vec_ok) {
      switch (p.lpl) {
        case 1: SGM_LANES(1, true, false, false); break;
        case 2: SGM_LANES(2, true, false, false); break;
        case 4: SGM_LANES(4, true, false, false); break;
        case 8: SGM_LANES(8, true, false, false); break;
        default: SGM_LANES(16, true, false, false); break;
      }
    } else {
      switch (p.lpl) {
        case 1: SGM_LANES(1, false, false, false); break;
        case 2: SGM_LANES(2, false, false, false); break;
        case 4: SGM_LANES(4, false, false, false); break;
        case 8: SGM_LANES(8, false, false, false); break;
        default: SGM_LANES(16, false, false, false); break;
      }
    }
#undef SGM_LANES1
#undef SGM_LANES
    MVS_LAUNCH_CHECK(what);
    acc = 1;  // the first set path stores, the later ones add
  }
  return 0;
}

}  // namespace
}  // namespace mvs
