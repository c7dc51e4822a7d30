// The per-pixel SAD plane sweep for gfx950 (CDNA4, wave64): sweep.hip's sweep (initial_depth_estimation_v2,
// clcode.cl:972-1069) at S=1 grid semantics, the reference-parity per-pixel mode.
//
//  k_sad_band        per (chunk of levels, neighbour) the
//                    neighbour's Lab band is staged in LDS once (LDS-DMA,
//                    double-buffered) and serves every level of the chunk; per
//                    level pair a lane forms its column's absolute differences
//                    and the 25-tap sums run in the reference's order as
//                    v_pk_add_f32 over the two levels, the window columns
//                    passed lane to lane by DPP wave_shr (systolic)
//                    or through an LDS plane (the first, two-phase form).
//  k_sweep_pixel_sad the first per-pixel form (every (d, neighbour) region
//                    gathered from global memory): kept for level sets with
//                    fractional column shifts.
#include "mvs_internal.h"
#include "wave.h"

namespace mvs {
namespace {

// ---- per-pixel SAD sweep on LDS bands (S=1 grid semantics) -----------------
// Tile: 60 output columns x TH rows; its 64 x (TH+4) tap region (2-pixel
// halo) has one region column per lane.  Steps t = (chunk c of DC = 8*PPW
// levels, neighbour n): the neighbour's Lab rows and columns reachable from
// the region at any level of the chunk are staged in LDS once per step and
// serve every level of the chunk.  The next step's band is loaded into
// registers at the start of a step and written to the other LDS buffer after
// the step's compute, so its latency hides behind the compute.  Wave w takes
// the chunk's level pairs w*PPW .. w*PPW+PPW-1; per pair:
//   A. each lane forms its region column's taps a = |dL|+|da|+|db| of both
//      levels from its reference colours (registers) and the band, or 30 for
//      a tap outside the image (ref or projection), into a wave-private LDS
//      plane of float2 {level 2p, level 2p+1};
//   B. each lane sums its output pixel's 25 taps, x offset outer and y offset
//      inner as the reference does, val = ((val + 30) - 30) + a, as three
//      v_pk_add_f32 over the pair.  (An out-of-image tap with a = 30 gives
//      RN(RN(RN(val+30) - 30) + 30) = RN(val+30): RN(val+30) - 30 is exact for
//      val >= 0, so this is the reference's lone val += 30, bit for bit.)
// The per-level minimum over neighbours folds into a first-minimum WTA in
// level order; the 4 waves' (cost, level) winners are merged
// lexicographically at the end.
// (SB_TW, SB_NBLK, SadArgs and SadRec: launch_plan.h, shared with the planner;
// SB_INIT and SweepArgs: there too, shared with sweep.hip)
// row-table entry of a row outside the image: a valid entry (yp-by0)*bw - bx0
// is negative on the band's first row whenever bx0 > 0, so no -1 sentinel
constexpr int SB_NOROW = -0x40000000;

static_assert(sizeof(SadRec) == 160, "k_sad_band reads one 160-byte record per step");

// the band of step record e for the tile at (x0, y0): every neighbour pixel a
// valid tap of the region can project to at any level of the chunk
struct SadBand {
  int bx0, by0, nrows, ncols;
};
template <int TH>
__device__ __forceinline__ SadBand sad_band_of(const SadRec& e, int x0, int y0, int W, int H) {
  SadBand g;
  g.bx0 = min(max(x0 - 2 - e.sxmax, 0), W - 1);
  const int bx1 = min(max(x0 + SB_TW + 1 - e.sxmin, 0), W - 1);
  g.by0 = min(max((int)((float)(y0 - 2) - e.fdymax), 0), H - 1);
  const int by1 = min(max((int)((float)(y0 + TH + 1) - e.fdymin), 0), H - 1);
  g.nrows = by1 - g.by0 + 1;
  g.ncols = bx1 - g.bx0 + 1;
  return g;
}

// The 25-tap sums run as a systolic chain across lanes (round 2's two-phase
// form staged the AD plane in LDS per wave and re-read it per tap: 3.35 ms
// per C2 view against 2.42; it was removed in round 3 with the other A/B
// variants).  An output's 25-tap chain takes its 5 window columns in order (x offset outer),
// and window column i of output x is region column x-2+i = lane (x-x0)+i.  So
// every lane runs the 5-row inner chains of its OWN column's taps (kept in
// registers) on the partial sums it receives from the lane to its left
// (DPP wave_shr:1, folded into the first add of each column): after the 5th
// column, lane l holds the output of image column x0 + l - 4.  The AD plane,
// its LDS writes/reads and the wave barriers of the two-phase form disappear.
// AFF: every level's row shift is integral, so region row r of
// level j reads band row r + (y0 - 2 - fdy_j - by0) exactly and is valid on
// one interval of r: the rows are addressed by immediate offsets r * BWT from
// one per-level lane address, and validity is a scalar interval test -- no
// row table reads, no per-row address arithmetic or compares.  BWT = the band
// pitch (a.bw) as a compile-time constant (0: runtime, the table path).
template <int TH, int PPW, bool AFF = false, int BWT = 0>
__global__ __launch_bounds__(256) void k_sad_band(const float4* __restrict__ lab, const float* __restrict__ levels,
                                                  const SadRec* __restrict__ plan, SadArgs a,
                                                  float* __restrict__ disp) {
  constexpr int RR = TH + 4, DC = 8 * PPW;
  extern __shared__ __align__(16) uint8_t smem[];
  float4* band = (float4*)smem;                // [2][brows][bw]
  int* rtab = (int*)(band + 2 * a.brows * a.bw);  // [2][DC][RR] (the row-table form)
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  // XCD-aware tile map (as k_ncc_volume): each XCD a contiguous strip of tiles
  const int bid = blockIdx.x, grp = bid & 7;
  const int tile = grp * a.tiles_per_xcd + (bid >> 3);
  if (tile >= a.ntiles) return;
  const int W = a.W, H = a.H;
  const int x0 = (tile % a.tiles_x) * SB_TW, y0 = (tile / a.tiles_x) * TH;
  const long P = (long)W * H;
  const int gx = x0 - 2 + lane;  // this lane's region column
  const bool gxok = gx >= 0 && gx < W;
  float rL[RR], ra[RR], rb[RR];
  {
    const float4* labz = lab + (long)a.z * P;
#pragma unroll
    for (int r = 0; r < RR; r++) {
      const int gy = y0 - 2 + r;
      const bool in = gxok && gy >= 0 && gy < H;
      const float4 c = labz[in ? (long)gy * W + gx : 0];
      rL[r] = c.x;
      ra[r] = c.y;
      rb[r] = c.z;
    }
  }
  const int T = a.nch * a.nn;

  SadBand pg{0, 0, 0, 0};
  // step t's band into LDS buffer b by 16-byte LDS-DMA (lane l's pixel lands
  // at 16 l past the wave-uniform row address), wave w taking rows w, w+4, ...
  // No registers hold the band: the register-staged prefetch this replaces
  // (12 float4 per lane) spilled to scratch, and the spill store waited for
  // the prefetch loads before the step could compute.  Columns past the band
  // (pitch a.bw is a multiple of 64) get a clamped copy nothing reads.
  auto stage = [&](int t, int b) {
    const SadRec& e = plan[t];
    pg = sad_band_of<TH>(e, x0, y0, W, H);
    const float4* src = lab + (long)e.view * P + (long)pg.by0 * W + pg.bx0;
    float4* dst = band + b * a.brows * a.bw;
    const int nblk = (pg.ncols + 63) >> 6;
    for (int cb = 0; cb < nblk; cb++) {
      const int col = min(cb * 64 + lane, pg.ncols - 1);
      for (int i = wave; i < pg.nrows; i += 4)
        glds_b128(src + (long)i * W + col, dst + i * a.bw + cb * 64);
    }
  };
  // step t's row table into buffer b: per (level j, region row r) the band
  // index of row yp minus bx0 (so + xp gives the pixel), or SB_NOROW when the
  // reference row or the projected row leaves the image
  auto commit = [&](int t, int b) {
    const SadRec& e = plan[t];
    int* tb = rtab + b * DC * RR;
    const int c = t / a.nn;
    for (int k = tid; k < DC * RR; k += 256) {
      const int j = k / RR, r = k - j * RR;
      const int gy = y0 - 2 + r;
      int v = SB_NOROW;
      if (c * DC + j < a.D) {
        const int yp = (int)((float)gy - e.fdy[j]);
        if (gy >= 0 && gy < H && yp >= 0 && yp < H) v = (yp - pg.by0) * a.bw - pg.bx0;
      }
      tb[k] = v;
    }
  };

  float best[TH];
  int bidx[TH];
#pragma unroll
  for (int o = 0; o < TH; o++) {
    best[o] = SB_INIT;
    bidx[o] = -1;
  }
  f32x2 mn[PPW][TH];
  if (T > 0) {
    stage(0, 0);
    if (!AFF) commit(0, 0);
  }
  __syncthreads();
  // chunks outer, neighbours inner (step t = c * nn + n): the chunk's reset
  // and WTA fold sit outside the per-step body.  As one flat step loop the
  // compiler if-converted them into every step (exec-masked compares and
  // selects issued nn times per chunk)
  int t = 0;
  for (int c = 0; c < (a.nn > 0 ? a.nch : 0); c++) {
#pragma unroll
  for (int q = 0; q < PPW; q++)
#pragma unroll
    for (int o = 0; o < TH; o++) mn[q][o] = f32x2{SB_INIT, SB_INIT};
  for (int n = 0; n < a.nn; n++, t++) {
    // step t+1's band lands in the other buffer (last read in step t-1, before
    // the previous barrier) while this step computes
    if (t + 1 < T) stage(t + 1, (t + 1) & 1);
    const SadRec& e = plan[t];
    const float4* bnd = band + (t & 1) * a.brows * a.bw;
    const int* tb = rtab + (t & 1) * DC * RR;
#pragma unroll
    for (int q = 0; q < PPW; q++) {
      const int j0 = (wave * PPW + q) * 2;
      const int xp0 = gx - e.sx[j0], xp1 = gx - e.sx[j0 + 1];
      const bool xok0 = gxok && xp0 >= 0 && xp0 < W, xok1 = gxok && xp1 >= 0 && xp1 < W;
      const f32x2 k30 = f32x2{30.0f, 30.0f};
      // A. taps of the lane's region column, both levels
      f32x2 ad[RR];
      if constexpr (AFF) {
        const SadBand g = sad_band_of<TH>(e, x0, y0, W, H);  // this step's band (pg is step t+1's)
        const int off0 = (int)e.fdy[j0], off1 = (int)e.fdy[j0 + 1];
        const int rlo0 = max(max(0, 2 - y0), 2 - y0 + off0), rhi0 = min(min(RR - 1, H + 1 - y0), H + 1 - y0 + off0);
        const int rlo1 = max(max(0, 2 - y0), 2 - y0 + off1), rhi1 = min(min(RR - 1, H + 1 - y0), H + 1 - y0 + off1);
        const int b0 = xok0 ? (y0 - 2 - off0 - g.by0) * BWT + xp0 - g.bx0 : 0;
        const int b1 = xok1 ? (y0 - 2 - off1 - g.by0) * BWT + xp1 - g.bx0 : 0;
#pragma unroll
        for (int r = 0; r < RR; r++) {
          const bool v0 = xok0 && r >= rlo0 && r <= rhi0, v1 = xok1 && r >= rlo1 && r <= rhi1;
          const float4 n0 = bnd[b0 + r * BWT], n1 = bnd[b1 + r * BWT];
          asm volatile("" ::"v"(n0.w), "v"(n1.w));  // keep the full 16-B ds_read_b128
          float d0 = fabsf(rL[r] - n0.x) + fabsf(ra[r] - n0.y);
          d0 = d0 + fabsf(rb[r] - n0.z);
          float d1 = fabsf(rL[r] - n1.x) + fabsf(ra[r] - n1.y);
          d1 = d1 + fabsf(rb[r] - n1.z);
          ad[r] = f32x2{v0 ? d0 : 30.0f, v1 ? d1 : 30.0f};
        }
      } else {
#pragma unroll
      for (int r = 0; r < RR; r++) {
        const int t0 = tb[j0 * RR + r], t1 = tb[(j0 + 1) * RR + r];
        const bool v0 = xok0 && t0 != SB_NOROW, v1 = xok1 && t1 != SB_NOROW;
        const float4 n0 = bnd[v0 ? t0 + xp0 : 0], n1 = bnd[v1 ? t1 + xp1 : 0];
        asm volatile("" ::"v"(n0.w), "v"(n1.w));  // keep the full 16-B ds_read_b128 (b96 is 3x slower)
        float d0 = fabsf(rL[r] - n0.x) + fabsf(ra[r] - n0.y);
        d0 = d0 + fabsf(rb[r] - n0.z);
        float d1 = fabsf(rL[r] - n1.x) + fabsf(ra[r] - n1.y);
        d1 = d1 + fabsf(rb[r] - n1.z);
        ad[r] = f32x2{v0 ? d0 : 30.0f, v1 ? d1 : 30.0f};
      }
      }
      // B'. systolic: column 0 starts the chains (first tap: ((0+30)-30)+a = a
      // exactly), columns 1..4 continue the left neighbour's partials
      f32x2 p[TH];
      float c30;  // 30.0f in a VGPR: the DPP add's second source
      asm volatile("v_mov_b32 %0, 0x41f00000" : "=v"(c30));
#pragma unroll
      for (int o = 0; o < TH; o++) {
        p[o] = ad[o];
#pragma unroll
        for (int jj = 1; jj < 5; jj++) p[o] = ((p[o] + k30) - k30) + ad[o + jj];
      }
#pragma unroll
      for (int i = 1; i < 5; i++) {
        // the shift folded into the first add of the column: v_add_f32 with a
        // DPP wave_shr:1 source (lane 0 reads 0 by bound_ctrl: 0 + 30), four
        // rows per asm block.  The block's leading s_nop 1 gives the two wait
        // states a DPP read of a VALU result needs (the compiler does not see
        // inside inline asm); the pk ops below still pair the results.
        float sx[TH], sy[TH];
#pragma unroll
        for (int o = 0; o < TH; o += 4)
          asm volatile(
              "s_nop 1\n\t"
              "v_add_f32_dpp %0, %8, %16 wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:0\n\t"
              "v_add_f32_dpp %1, %9, %16 wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:0\n\t"
              "v_add_f32_dpp %2, %10, %16 wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:0\n\t"
              "v_add_f32_dpp %3, %11, %16 wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:0\n\t"
              "v_add_f32_dpp %4, %12, %16 wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:0\n\t"
              "v_add_f32_dpp %5, %13, %16 wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:0\n\t"
              "v_add_f32_dpp %6, %14, %16 wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:0\n\t"
              "v_add_f32_dpp %7, %15, %16 wave_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:0"
              : "=&v"(sx[o]), "=&v"(sy[o]), "=&v"(sx[o + 1]), "=&v"(sy[o + 1]), "=&v"(sx[o + 2]), "=&v"(sy[o + 2]),
                "=&v"(sx[o + 3]), "=&v"(sy[o + 3])
              : "v"(p[o].x), "v"(p[o].y), "v"(p[o + 1].x), "v"(p[o + 1].y), "v"(p[o + 2].x), "v"(p[o + 2].y),
                "v"(p[o + 3].x), "v"(p[o + 3].y), "v"(c30));
#pragma unroll
        for (int o = 0; o < TH; o++) {
          f32x2 v = f32x2{sx[o], sy[o]};
          v = (v - k30) + ad[o];
#pragma unroll
          for (int jj = 1; jj < 5; jj++) v = ((v + k30) - k30) + ad[o + jj];
          p[o] = v;
        }
      }
      // v_min_f32 as asm: fminf made the compiler canonicalise the
      // loop-carried minima (a v_max_f32 x, x each) every step; no NaN here
#pragma unroll
      for (int o = 0; o < TH; o++) {
        asm("v_min_f32 %0, %1, %2" : "=v"(mn[q][o].x) : "v"(mn[q][o].x), "v"(p[o].x));
        asm("v_min_f32 %0, %1, %2" : "=v"(mn[q][o].y) : "v"(mn[q][o].y), "v"(p[o].y));
      }
    }
    // step t+1's row table (its rows were last read in step t-1); the barrier
    // (vmcnt(0) first) publishes the table and the landed band
    if (t + 1 < T && !AFF) commit(t + 1, (t + 1) & 1);
    __syncthreads();
  }
  // chunk complete: first-minimum WTA in level order
#pragma unroll
  for (int q = 0; q < PPW; q++) {
    const int dl = c * DC + (wave * PPW + q) * 2;
#pragma unroll
    for (int o = 0; o < TH; o++) {
      if (dl < a.D && mn[q][o].x < best[o]) {
        best[o] = mn[q][o].x;
        bidx[o] = dl;
      }
      if (dl + 1 < a.D && mn[q][o].y < best[o]) {
        best[o] = mn[q][o].y;
        bidx[o] = dl + 1;
      }
    }
  }
  }
  // merge the 4 waves' winners: lexicographic (cost, level)
  float* mb = (float*)smem;
  int* mi = (int*)(mb + 4 * TH * 64);
#pragma unroll
  for (int o = 0; o < TH; o++) {
    mb[(wave * TH + o) * 64 + lane] = best[o];
    mi[(wave * TH + o) * 64 + lane] = bidx[o];
  }
  __syncthreads();
  for (int k = tid; k < TH * 64; k += 256) {
    const int o = k >> 6, l = k & 63;
    const int x = x0 + l - 4, y = y0 + o;  // lane l holds column x0 + l - 4
    if (l < 4 || x >= W || y >= H) continue;
    float bv = mb[k];
    int bi = mi[k];
#pragma unroll
    for (int w = 1; w < 4; w++) {
      const float v = mb[w * TH * 64 + k];
      const int i = mi[w * TH * 64 + k];
      if (i >= 0 && (v < bv || (v == bv && (bi < 0 || i < bi)))) {
        bv = v;
        bi = i;
      }
    }
    disp[(long)y * W + x] = (bi >= 0 && bv < SB_INIT) ? levels[bi] : 0.0f;
  }
}

// ---- per-pixel SAD sweep (S=1 grid semantics of initial_depth_estimation_v2)
// (PT, the output tile edge: launch_plan.h)
constexpr int PR = PT + 4;       // region edge (2-pixel halo)
constexpr int PREG = PR * PR;    // 1296 region pixels
constexpr int PPT = (PREG + 255) / 256;  // region pixels per thread (6)

__global__ __launch_bounds__(256) void k_sweep_pixel_sad(const float4* __restrict__ lab,
                                                         const float* __restrict__ levels,
                                                         const int* __restrict__ vs, const int* __restrict__ sn,
                                                         SweepArgs a, float* __restrict__ disp) {
  __shared__ float2 ca[PR][PR];  // (c, a): valid -> (30, AD), invalid -> (0, 0)
  const int tid = threadIdx.x;
  const int x0 = blockIdx.x * PT, y0 = blockIdx.y * PT;
  const long P = (long)a.W * a.H;
  const float4* labz = lab + (long)a.z * P;
  // reference colours of this thread's region pixels (constant over d, n)
  float3 rc[PPT];
  int rxy[PPT];
#pragma unroll
  for (int k = 0; k < PPT; k++) {
    int r = tid + 256 * k;
    int gx = x0 - 2 + r % PR, gy = y0 - 2 + r / PR;
    bool in = r < PREG && gx >= 0 && gy >= 0 && gx < a.W && gy < a.H;
    float4 c = in ? labz[(long)gy * a.W + gx] : make_float4(0.f, 0.f, 0.f, 0.f);
    rc[k] = make_float3(c.x, c.y, c.z);
    rxy[k] = in ? r : -1;
  }
  const int tx = tid & 31, ty0 = (tid >> 5) * 4;
  const int rx = a.z % a.aw, ry = a.z / a.aw;
  const int nn = sn[a.z];
  float cost[4], dsp[4];
#pragma unroll
  for (int o = 0; o < 4; o++) {
    cost[o] = SB_INIT;
    dsp[o] = 0.0f;
  }
  for (int dl = 0; dl < a.D; dl++) {
    const float d = levels[dl];
    float mn[4];
#pragma unroll
    for (int o = 0; o < 4; o++) mn[o] = SB_INIT;
    for (int n = 0; n < nn; n++) {
      const int view = vs[a.V * a.z + n];
      const int vx = view % a.aw, vy = view / a.aw;
      const float fdx = d * (float)(vx - rx);
      const float fdy = (a.bl * d) * (float)(vy - ry);
      const float4* labv = lab + (long)view * P;
      __syncthreads();  // previous (d, n) reads of ca done
#pragma unroll
      for (int k = 0; k < PPT; k++) {
        int r = tid + 256 * k;
        if (r < PREG) {
          float2 v = make_float2(0.0f, 0.0f);
          if (rxy[k] >= 0) {
            int gx = x0 - 2 + r % PR, gy = y0 - 2 + r / PR;
            int xp = (int)((float)gx - fdx);
            int yp = (int)((float)gy - fdy);
            if (xp >= 0 && yp >= 0 && xp < a.W && yp < a.H) {
              float4 B = labv[(long)yp * a.W + xp];
              float ad = fabsf(rc[k].x - B.x) + fabsf(rc[k].y - B.y);
              ad = ad + fabsf(rc[k].z - B.z);
              v = make_float2(30.0f, ad);
            }
          }
          ca[r / PR][r % PR] = v;
        }
      }
      __syncthreads();
      float val[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
      for (int i = 0; i < 5; i++) {  // window column (x offset) outer
        float2 col[8];
#pragma unroll
        for (int q = 0; q < 8; q++) col[q] = ca[ty0 + q][tx + i];
#pragma unroll
        for (int o = 0; o < 4; o++)
#pragma unroll
          for (int j = 0; j < 5; j++) {  // window row (y offset) inner
            float t = val[o] + 30.0f;
            t = t - col[o + j].x;
            val[o] = t + col[o + j].y;
          }
      }
#pragma unroll
      for (int o = 0; o < 4; o++)
        if (val[o] < mn[o]) mn[o] = val[o];
    }
#pragma unroll
    for (int o = 0; o < 4; o++)
      if (mn[o] < cost[o]) {
        cost[o] = mn[o];
        dsp[o] = d;
      }
  }
#pragma unroll
  for (int o = 0; o < 4; o++) {
    int x = x0 + tx, y = y0 + ty0 + o;
    if (x < a.W && y < a.H) disp[(long)y * a.W + x] = dsp[o];
  }
}

// the k_sad_band instantiation of a band plan (TH = 8; BWT: 0 with the row table, else 64 or 128)
using SadBandKernel = void (*)(const float4*, const float*, const SadRec*, SadArgs, float*);
SadBandKernel sad_band_kernel(const plan::SadPlan& p) {
  static constexpr SadBandKernel k[2][3] = {
      {k_sad_band<8, 2>, k_sad_band<8, 2, true, 64>, k_sad_band<8, 2, true, 128>},
      {k_sad_band<8, 1>, k_sad_band<8, 1, true, 64>, k_sad_band<8, 1, true, 128>}};
  return k[p.PPW == 1][!p.AFF ? 0 : p.BWT == 64 ? 1 : 2];
}

}  // namespace

// The per-pixel SAD sweep, one launch per reference view as plan_sad
// (launch_plan.cpp) chooses: a band-staged form, or the gather kernel.
int launch_sweep_pixel_sad(mvs_ctx* ctx, int V, int W, int H, const float* lab, const float* levels_host, int D,
                           const int* vs_host, const int* sn_host, int aw, float bl, int z0, int z1, float* disp) {
  const plan::Tuning t = plan::plan_tuning();
  const long P = (long)W * H;
  for (int z = z0; z < z1; z++) {
    float* out = disp + (long)(z - z0) * P;
    const plan::SadPlan p = plan::plan_sad(t, V, W, H, D, levels_host, vs_host, sn_host, aw, bl, z);
    if (!p.err.empty()) {
      set_error(p.err);
      return MVS_E_UNSUPPORTED;
    }
    const dim3 g(p.grid_x, p.grid_y);
    if (p.band) {
      int rc = 0;
      const int32_t* dev = plan_upload(ctx, p.table, &rc);
      if (rc) return rc;
      const SadBandKernel kern = sad_band_kernel(p);
      MVS_HIP(raise_lds(ctx, (const void*)kern, p.lds), "hipFuncSetAttribute(sad lds)");
      hipLaunchKernelGGL(kern, g, dim3(256), p.lds, ctx->stream, (const float4*)lab, ctx->d_levels,
                         (const SadRec*)dev, p.args, out);
      MVS_LAUNCH_CHECK("k_sad_band");
    } else {
      SweepArgs a{V, W, H, W, H, D, aw, z, bl};
      hipLaunchKernelGGL(k_sweep_pixel_sad, g, dim3(256), 0, ctx->stream, (const float4*)lab, ctx->d_levels,
                         ctx->d_vs, ctx->d_sn, a, out);
      MVS_LAUNCH_CHECK("k_sweep_pixel_sad");
    }
  }
  return 0;
}

}  // namespace mvs
