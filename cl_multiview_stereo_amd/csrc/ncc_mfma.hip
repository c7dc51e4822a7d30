// Matrix-core form of the fused NCC sweep + WTA (K = 5 and K = 7): the
// definition and the outputs are ncc.hip's (k_ncc_volume with FUSE), bit for bit;
// plan_ncc_launches (ncc_plan.cpp) picks it per reference view.  See the comment at
// NccMRec for the formulation.
#include <type_traits>

#include "ncc_common.h"

namespace mvs {
namespace ncc {
namespace {

// ---- matrix-core form of the fused sweep (written out for K = 5; K = 7: at k_ncc_mfma) ----
//
// The correlation Srp'(x, y, d) = sum_{j, i} r'(x+i, y+j) p'(x+i-tx(d), y+j)
// as a GEMM whose output lands in the SAME (pixel, level) layout for every
// neighbour, so the neighbour maximum stays in registers:
//   C[m][n] = sum_k A[m][k] B[k][n],   m = (xx, yy) of a 4 x 4 pixel block,
//   n = level d0 + n of a 16-level block, k = (row, column) of the block's
//   8 x 8 window footprint (rows y0b-2 .. y0b+5, columns x0b-2 .. x0b+5);
//   A[m][k] = r'(column, row) where the tap lies in pixel m's 5 x 5 window, else 0
//             (the REFERENCE, banded: built once per tile, reused for every
//             neighbour and level);
//   B[k][n] = p'(column - tx(d0+n), row)   (the neighbour: its row-pair pk entry
//             at column x0b - tx, i.e. one aligned 16-byte LDS read per lane).
// k = 64 = 4 row pairs x 16 bytes is exactly one v_mfma_i32_16x16x64_i8 and
// exactly the pk plane's row-pair entry, so a lane's B operand for row pair g
// is ONE ds_read_b128 from the band the LDS-DMA stages anyway.  The MFMA's
// accumulator starts at the bits of 1.5 * 2^23: read as a float the result is
// 1.5 * 2^23 + Srp' exactly (|Srp'| < 2^22), one v_sub_f32 per cell (scalar
// f32 throughout the finish and fold: v_pk_*_f32 measured slower, C2 -1.3 %,
// C5 -3.2 %, profiles/r06/ab_scalar_f32_finish.txt).
// Per lane the output is C[4 (l >> 4) + r][l & 15]: pixel column xx = l >> 4,
// rows yy = r = 0..3, level l & 15 -- a fixed pixel column and level per lane,
// so the neighbour stats (a, b of rows y0b..y0b+3 at column x - tx) are two
// ds_read_b128 per lane, and the finish x = fma(-Sr', b, Srp' a) and the
// maximum are the scalar kernel's operations in the same order (bit-identical).
// Per wave and neighbour step: 4 pixel blocks (8 columns x 8 rows) x 2 level
// blocks = 8 MFMAs for 2,048 view-cells, against 192 dot4 of the scalar form.
// Lane l holds the levels of class l & 15 (16 apart): the fold keeps the same
// (smallest, its level, second smallest) triple per cell, and the 16 classes
// of a pixel are merged through LDS as the scalar kernel merges its waves.
//
// VERT (lists with vertical / diagonal neighbours, C4): level j also shifts
// rows by ty(j), so its footprint starts o_j = tymax - ty(j) + (tymax & 1)
// rows into the band (the pk and stats bands start o_j's parity apart from
// a pair boundary alike).  At an odd o_j a lane's two footprint rows (and a
// pixel's stats rows) straddle two band pair entries: the B operand is two
// ds_read_b64 (row 2g + o_j, row 2g + o_j + 1) and the stats four (a, b)
// pairs, per-lane addresses fixed for the step -- the MFMA and the finish
// are unchanged.  The bands are staged per step (their rows depend on the
// step's tymax), 16 NDB levels per chunk.
struct alignas(128) NccMRec {
  int txmax, tymax;  // band origin, as NccRec
  int bhp, shp;      // pk pair rows to stage; stats pair rows (bits 0..7) | the stats bank shift (signed,
                     // bits 8..15) | column span << 16 | the odd pk rows' bank shift (signed) << 24
  int colo[16];      // 32 x int16: per level j of the chunk, txmax - tx(j) (band column of reference column x0)
                     // | o_j << 8 (VERT: band row of the level's footprint)
  int pad0[2];
  unsigned off_lo, off_hi;  // the neighbour's plane: byte offset from the stack's first (set by the launcher)
  int pad[8];
};
static_assert(sizeof(NccMRec) == 4 * kRecWords, "one 128-B record per (chunk, neighbour)");

// A tile is 64 columns x 8 rows: a wave owns 8 columns x 8 rows = 4 pixel
// blocks (K = 5: 4 x 4 pixels, one MFMA per level block; K = 7: 2 columns x
// 8 rows, whose 8-column x 16-row footprint is 8 row pairs = two MFMAs, the
// second accumulating onto the first).  TAIL: D % DC != 0, the last chunk carries dummy levels past the
// end.  NDB: 16-level blocks per chunk (DC = 16 NDB levels per step).  NB:
// band buffers (2: step t+1's bands land while step t computes; 1: staged at
// the start of each step, the other resident workgroup computing meanwhile;
// VERT only -- horizontal lists are always double-buffered).
// DBG (timing probe only, MVS_NCC_MFMA_DBG): 1 skips the MFMAs and the
// finish (band DMA, barriers, fold and merge stay), 2 skips the band DMA
template <int K, int BW, bool TAIL, bool VERT, int NDB, int NB, int DBG = 0>
__global__ __launch_bounds__(512) __attribute__((amdgpu_waves_per_eu(4))) void k_ncc_mfma(
    const uint2* __restrict__ stats, const uint2* __restrict__ pk, const NccMRec* __restrict__ plan, NccArgs a,
    WtaOut wo) {
  static_assert(NDB == 1 || NDB == 2, "one or two 16-level blocks per chunk");
  static_assert(K == 5 || K == 7, "5 x 5 or 7 x 7 windows");
  static_assert(K == 5 || !VERT, "K = 7: horizontal lists only");
  static_assert(VERT || NB == 2, "the horizontal form is double-buffered");
  static_assert(VERT || NDB == (K == 5 ? 2 : 1), "horizontal chunks: 32 levels (K = 5), 16 (K = 7: A takes 32 VGPRs)");
  constexpr int R = K / 2, NW = 8, TH = 8, DC = 16 * NDB, NK = K * K;
  // pixel blocks per wave: XB across (BXW columns each) x NYB down; MF MFMAs per block and level block
  constexpr int XB = K == 5 ? 2 : 4, NYB = K == 5 ? TH / 4 : 1, NBL = XB * NYB, MF = K == 5 ? 1 : 2;
  constexpr int BXW = 8 / XB;
  // band row pitch: BW + 1 columns of 16 B, so a lane group's B reads in two
  // rows (row pairs g, g + 1) fall on different banks when the shift per level
  // is even (|dx| = 2: conflict-free instead of 2-way)
  constexpr int BWP = BW + 1;
  extern __shared__ __align__(16) uint8_t smem[];
  const int nbuf = (a.pk_pairs + a.st_pairs) * BWP;  // uint4 per neighbour buffer
  u32x4* nbase = (u32x4*)smem;                      // 2 x {npk[pk_pairs][BW], nst[st_pairs][BW]}
  const int band_bytes = max(NB * nbuf * 16, 3 * 16 * kMfMergeStride * 4);
  float* rsn_l = (float*)(smem + band_bytes);  // [64][TH] -Sr' of the tile's pixels (column-major)
  float* srl = rsn_l + 64 * TH;                 // [64][TH] s_r
  short* colo_l = (short*)(srl + 64 * TH);      // [T][DC] band column (| row) offsets per step and level

  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int W = a.W, H = a.H;
  const int Hp2 = (H + 1) >> 1;
  const long Pv = (long)W * Hp2 * 2;
  const long P = (long)W * H;
  const int bid = blockIdx.x, grp = bid & 7;  // XCD-aware tile map, as k_ncc_volume
  const int tg = grp * a.tiles_per_xcd + (bid >> 3);
  if (tg >= a.ntiles * a.nref) return;
  const int ref = tg / a.ntiles, tile = tg - ref * a.ntiles;
  const int x0 = (tile % a.tiles_x) * 64;
  const int y0 = (tile / a.tiles_x) * TH;  // even
  const int nn = a.nn[ref], T = a.nch * nn;
  const NccMRec* rec = plan + a.plan[ref];

  // LDS-DMA staging of step t's bands (k_ncc_volume's stage, one record per
  // step).  Horizontal lists: every step's band rows are the same image rows,
  // so wave w stages pk pair row w (w < bhp) and stats pair row w (w < shp),
  // whose clamped row offsets are computed once per tile.  VERT: the rows
  // start at the step's tymax, the waves take the pair rows in turn
  // pk band: K = 5 rows y0 - 2 .. y0 + TH + 1 (pair (y0 - 2) / 2 on); K = 7 the
  // 8 pairs from (y0 - 4) / 2 (rows y0 - 4 .. y0 + TH + 3: every block's
  // 16-row footprint, its first and last rows masked off in A)
  const int bhp = K == 5 ? (TH + 4) / 2 : (TH + 8) / 2, shp = TH / 2;
  const long pk_row = 2L * W * min(max((y0 >> 1) - (K == 5 ? 1 : 2) + wave, 0), Hp2 - 1);
  const long st_row = 2L * W * min(max(y0 / 2 + wave, 0), Hp2 - 1);
  // Horizontal lists: a step's scalars (band origin, column span, neighbour
  // view) are loaded two steps ahead and carried, so no step waits on a
  // scalar load; its DMA goes through buffer descriptors rebased per step
  // (base = the neighbour's plane row, 32-bit lane offsets: the clamped
  // column x 16 B), no per-lane 64-bit address arithmetic.
  struct StepInfo {
    int tx, shp;      // raw record words: nothing computed on them until they are used
    unsigned lo, hi;  // the neighbour plane's byte offset
  };
  // (n, the step's neighbour, is not used: the record holds the plane's offset.  It, nmod below
  // and the !VERT branch of stage, which horizontal lists never call, are dead source that
  // the horizontal kernels' register allocation depends on all the same: without any one of
  // them the K = 5 kernels, at the 128-VGPR cap, spill 12 to 20 B.  DESIGN.md §4i)
  auto load_info = [&](int t, int n) -> StepInfo {
    const NccMRec& e = rec[t];
    return StepInfo{e.txmax, e.shp, e.off_lo, e.off_hi};
  };
  const int lane_x = x0 + lane;
  auto stage_h = [&](const StepInfo& e, int b) {
    if (DBG == 2) return;
    const int span = (e.shp >> 16) & 0xff, nblk = (span + 127) >> 6;
    const unsigned long long vo = (unsigned long long)e.hi << 32 | e.lo;
    // odd pk pair rows land sh columns along, and (K = 7) stats pair rows 2, 3
    // st columns along (the step's bank shifts, see step())
    u32x4* npk = nbase + b * nbuf + ((wave & 1) ? (e.shp >> 24) : 0);
    u32x4* nst = nbase + b * nbuf + a.pk_pairs * BWP + ((K == 7 && wave >= 2) ? ((e.shp << 16) >> 24) : 0);
    // the wave's roles (pk row w < bhp, stats row w < shp) decided once per step, not per piece
    if (wave < shp) {
      const __amdgpu_buffer_rsrc_t rp = buf_rsrc((const char*)pk + vo + 8 * pk_row, 16 * W);
      const __amdgpu_buffer_rsrc_t rs = buf_rsrc((const char*)stats + vo + 8 * st_row, 16 * W);
      for (int cb = 0; cb < nblk; cb++) {
        const int c0 = min(cb * 64, span);
        const int voff = 16 * min(max(lane_x - e.tx + c0, 0), W - 1);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rp, (lds_ptr_t)(npk + wave * BWP + c0), 16, voff, 0, 0, 0);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_ptr_t)(nst + wave * BWP + c0), 16, voff, 0, 0, 0);
      }
    } else if (wave < bhp) {
      const __amdgpu_buffer_rsrc_t rp = buf_rsrc((const char*)pk + vo + 8 * pk_row, 16 * W);
      for (int cb = 0; cb < nblk; cb++) {
        const int c0 = min(cb * 64, span);
        const int voff = 16 * min(max(lane_x - e.tx + c0, 0), W - 1);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rp, (lds_ptr_t)(npk + wave * BWP + c0), 16, voff, 0, 0, 0);
      }
    }
  };
  // VERT's staging (the prologue, the NB = 1 restage, the look-ahead); horizontal lists go through stage_h
  auto stage = [&](int t, int n, int b) {
    if (DBG == 2) return;
    const NccMRec& e = rec[t];
    const int span = (e.shp >> 16) & 0xff, nblk = (span + 127) >> 6;  // (VERT: no odd-row shift)
    const long vo = (long)a.view[ref][n] * Pv;
    u32x4* npk = nbase + b * nbuf;
    u32x4* nst = npk + a.pk_pairs * BWP;
    const int xb0 = x0 - e.txmax + lane;
    if constexpr (!VERT) {  // never called (see load_info)
      for (int cb = 0; cb < nblk; cb++) {
        const int c0 = min(cb * 64, span);
        const int xx = min(max(xb0 + c0, 0), W - 1);
        if (wave < bhp) glds_b128(pk + vo + pk_row + 2 * xx, npk + wave * BWP + c0);
        if (wave < shp) glds_b128(stats + vo + st_row + 2 * xx, nst + wave * BWP + c0);
      }
    } else {
      const int ebh = e.bhp, esh = e.shp & 0xff;
      const int pm0 = (y0 - R - e.tymax) >> 1, sm0 = (y0 - e.tymax) >> 1;  // floor: arithmetic shifts
      for (int cb = 0; cb < nblk; cb++) {
        const int c0 = min(cb * 64, span);
        const int xx = min(max(xb0 + c0, 0), W - 1);
        const uint2* gpk = pk + vo + 2 * xx;
        const uint2* gst = stats + vo + 2 * xx;
        for (int i = wave; i < ebh; i += NW) glds_b128(gpk + 2L * W * min(max(pm0 + i, 0), Hp2 - 1), npk + i * BWP + c0);
        for (int i = wave; i < esh; i += NW) glds_b128(gst + 2L * W * min(max(sm0 + i, 0), Hp2 - 1), nst + i * BWP + c0);
      }
    }
  };

  // the steps' level -> band column offsets, into LDS (before the pipeline)
  for (int i = tid; i < T * DC / 2; i += NW * 64) ((int*)colo_l)[i] = rec[i / (DC / 2)].colo[i % (DC / 2)];
  auto nmod = [&](int v) { return v >= nn ? v - nn : v; };  // (v < 2 nn) a step's neighbour: for load_info's n only
  // step t's scalars (cur) and step t+1's (nxt): horizontal lists only (VERT
  // reads rec[t] where it needs it; step() names cur in both, so they are
  // declared for both and stay empty under VERT)
  StepInfo cur{}, nxt{};
  if constexpr (!VERT) {
    cur = load_info(0, 0);
    if (T > 1) nxt = load_info(1, nmod(1));
    stage_h(cur, 0);
  } else {
    stage(0, 0, 0);
  }
  const long zo = (long)a.z[ref] * Pv;
  // The reference plane's rows this tile reads (the window rows of its pixels,
  // the blocks' footprints) lie within 8 pair rows of pair zp0, so they are
  // read through one buffer descriptor based there: a row is a scalar offset,
  // a column a 32-bit lane offset, no per-lane 64-bit address arithmetic.
  const int zp0 = min(max((y0 >> 1) - (K == 5 ? 1 : 2), 0), Hp2 - 1);
  const __amdgpu_buffer_rsrc_t rz = buf_rsrc((const char*)pk + 8 * (zo + 2L * W * zp0), 16 * W * min(Hp2 - zp0, 8));
  // -Sr' and s_r of the tile's 64 x TH pixels (lane = column), as k_ncc_volume:
  // wave w takes rows w, w + 8, ... (one correctly rounded sqrt + divide per
  // row and lane, spread over the waves instead of TH of them on wave 0)
  for (int o = wave; o < TH; o += NW) {
    const int x = x0 + lane, y = y0 + o;
    const int xoff = 16 * min(x, W - 1);
    int s1 = 0, s2 = 0;
#pragma unroll
    for (int k = 0; k < 2 * R + 1; k++) {
      const int yc = min(max(y - R + k, 0), H - 1);  // (wave-uniform: the row's offset is scalar)
      const u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(rz, xoff, 16 * W * ((yc >> 1) - zp0) + 8 * (yc & 1), 0);
      const unsigned lo = v.x, hi = v.y & (K == 5 ? 0xffu : 0xffffffu);  // the window's K bytes
      s1 = dot4(lo, 0x01010101u, dot4(hi, 0x01010101u, s1));
      s2 = dot4(lo, lo, dot4(hi, hi, s2));
    }
    const bool valid = x - R >= 0 && x + R < W && y - R >= 0 && y + R < H;
    const int var = NK * s2 - s1 * s1;
    srl[lane * TH + o] = !valid ? __int_as_float(0x7fc00000) : (var != 0 ? 1.0f / sqrtf((float)var) : 0.0f);
    rsn_l[lane * TH + o] = -(float)s1;
  }
  // the reference operands.  K = 5: pixel block (xb, yb) of this wave =
  // columns x0 + 8 wave + 4 xb .. +3, rows y0 + 4 yb .. +3; lane l supplies
  // row m = l & 15 (pixel xx = m >> 2, yy = m & 3) and row pair g = l >> 4 of
  // the footprint: the 16-byte pk entry at column x0b, masked to the pixel's
  // window (bytes xx .. xx+4 of a row; footprint rows yy .. yy+4).  K = 7:
  // block xb = columns x0 + 8 wave + 2 xb, +1, rows y0 .. y0 + 7; m = 8 xx + yy,
  // the footprint rows y0 - 4 .. y0 + 11 (pairs g and g + 4: the block's two
  // MFMAs), bytes xx .. xx+6, footprint rows yy + 1 .. yy + 7
  i32x4 A[NBL][MF];
  {
    const int mA = lane & 15, g = lane >> 4;
    const int xxA = K == 5 ? mA >> 2 : mA >> 3, yyA = K == 5 ? mA & 3 : mA & 7;
    // a row's 8 bytes masked to the window's K columns: K bytes of ones moved
    // xxA bytes up; a footprint row rr = 2 (g + 4 mf) + h outside the window's
    // rows (K = 5: yyA .. yyA + 4; K = 7: yyA + 1 .. yyA + 7) takes no tap
    const unsigned long long cm = (K == 5 ? 0xFFFFFFFFFFull : 0xFFFFFFFFFFFFFFull) << (8 * xxA);
    const unsigned cm_lo = (unsigned)cm, cm_hi = (unsigned)(cm >> 32);
    unsigned msk[MF][4];
#pragma unroll
    for (int mf = 0; mf < MF; mf++)
#pragma unroll
      for (int h = 0; h < 2; h++) {
        const int rr = 2 * (g + 4 * mf) + h;
        const bool in = (unsigned)(rr - yyA - (K == 5 ? 0 : 1)) <= (unsigned)(K - 1);
        msk[mf][2 * h] = in ? cm_lo : 0u;
        msk[mf][2 * h + 1] = in ? cm_hi : 0u;
      }
    // the entries: the lane's pair row as one 32-bit offset per (yb | mf), the
    // block's column (wave-uniform) as the load's scalar offset
    constexpr int NPR = K == 5 ? NYB : MF;
    int roff[NPR];
#pragma unroll
    for (int i = 0; i < NPR; i++) {
      const int pr = min(max((K == 5 ? (y0 >> 1) - 1 + 2 * i : (y0 >> 1) - 2 + 4 * i) + g, 0), Hp2 - 1);
      roff[i] = 16 * W * (pr - zp0);
    }
#pragma unroll
    for (int xb = 0; xb < XB; xb++) {
      const int xcol = min(x0 + 8 * wave + BXW * xb, W - 1);
#pragma unroll
      for (int yb = 0; yb < NYB; yb++)
#pragma unroll
        for (int mf = 0; mf < MF; mf++) {
          const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rz, roff[K == 5 ? yb : mf], 16 * xcol, 0);
          A[xb * NYB + yb][mf] = i32x4{(int)(v.x & msk[mf][0]), (int)(v.y & msk[mf][1]), (int)(v.z & msk[mf][2]),
                                       (int)(v.w & msk[mf][3])};
        }
    }
  }
  // this lane's output pixels of block (xb, yb): column 8 wave + pcol, rows
  // prow .. prow + 3 of the tile (the MFMA's C[4 (l >> 4) + r][l & 15])
  auto pcol = [&](int xb, int g) { return BXW * xb + (K == 5 ? g : g >> 1); };
  auto prow = [&](int yb, int g) { return K == 5 ? 4 * yb : 4 * (g & 1); };
  __syncthreads();

  float E[NBL][NDB][4];  // [block][level block][row]: max over the neighbours so far
  float wv0[NBL][4], wv1[NBL][4];
  unsigned wi0p[NBL][2];  // level of the smallest, rows (2p, 2p+1) as the halves of one register (0xffff: none)
#pragma unroll
  for (int k = 0; k < NBL; k++) {
#pragma unroll
    for (int r = 0; r < 4; r++) {
      wv0[k][r] = kWtaInit;
      wv1[k][r] = kWtaInit;
    }
    wi0p[k][0] = wi0p[k][1] = 0xffffffffu;
  }
  const i32x4 bias = i32x4{kMagicI, kMagicI, kMagicI, kMagicI};

  // fold chunk c's levels into the per-cell triples (k_ncc_volume's fold; this
  // lane's levels are c * DC + 16 db + (l & 15), in increasing order)
  auto fold = [&](int c) {
    const int ln = lane_now();
    // dummy levels past the end (TAIL kernels, last chunk): +inf costs change nothing
    float kill[NDB];
#pragma unroll
    for (int db = 0; db < NDB; db++) kill[db] = 0.0f;
    if (TAIL && c == a.nch - 1)
#pragma unroll
      for (int db = 0; db < NDB; db++) kill[db] = c * DC + 16 * db + (ln & 15) >= a.D ? INFINITY : 0.0f;
#pragma unroll
    for (int xb = 0; xb < XB; xb++)
#pragma unroll
      for (int yb = 0; yb < NYB; yb++) {
        const int kb = xb * NYB + yb;
        const f32x4 sq = *(const f32x4*)(srl + (8 * wave + pcol(xb, ln >> 4)) * TH + prow(yb, ln >> 4));
        // NDB = 2: this lane's two levels of the chunk, dl0 < dl1 = dl0 + 16,
        // folded as a pair: with lo / hi their smaller / larger cost, the
        // triple's new second smallest is min(max(v0, lo), v1, hi) (the second
        // of the multiset {v0 <= v1, c0, c1}), its smallest min(v0, lo), and its
        // level the pair's first argmin (dl1 only if c1 < c0) when lo < v0: the
        // sequential fold's results in fewer instructions per level
        const int dl0 = c * DC + (ln & 15);
        const unsigned d0 = (unsigned)dl0 * 0x10001u, d1 = (unsigned)(dl0 + 16) * 0x10001u;
#pragma unroll
        for (int r = 0; r < 4; r += 2) {
          f32x2 cst[NDB];
#pragma unroll
          for (int db = 0; db < NDB; db++) {
            f32x2 e;
            e.x = __fmul_rn(E[kb][db][r], sq[r]);
            e.y = __fmul_rn(E[kb][db][r + 1], sq[r + 1]);
            // NDB = 2: 1 - m without the clamp max(-1, m) -- a cost above 2 or
            // NaN (no valid neighbour window at the level) stands for the
            // clamped 2, restored at the merge; the pair fold below treats NaN
            // as absent.  (NDB = 1 keeps the clamp: its med3 fold would not.)
            if constexpr (NDB == 2) {
              cst[db].x = __fsub_rn(1.0f, e.x);
              cst[db].y = __fsub_rn(1.0f, e.y);
            } else {
              cst[db].x = __fsub_rn(1.0f, vmax_m1(e.x));
              cst[db].y = __fsub_rn(1.0f, vmax_m1(e.y));
            }
            if (TAIL) {  // costs are >= 0: x + 0 = x, x + inf = inf
              cst[db].x = __fadd_rn(cst[db].x, kill[db]);
              cst[db].y = __fadd_rn(cst[db].y, kill[db]);
            }
          }
#pragma unroll
          for (int h = 0; h < 2; h++) {
            const unsigned hm = h ? 0xffff0000u : 0x0000ffffu;
            unsigned& wp = wi0p[kb][r >> 1];
            float& v0 = wv0[kb][r + h];
            float& v1 = wv1[kb][r + h];
            if constexpr (NDB == 2) {
              const float c0 = cst[0][h], c1 = cst[NDB - 1][h];  // NaN: absent (the clamped 2)
              const float lo = vmin3(c0, c1, INFINITY);  // the smaller present cost (+inf: none)
              const float hi = vmaximum3(c0, c1, c1);    // the larger, NaN if either is absent
              const unsigned idx = lo == c0 ? d0 : d1;   // a tie keeps the lower level
              v1 = vmin3(vmax(v0, lo), v1, hi);          // (a NaN hi drops out of the min)
              wp = lo < v0 ? (wp & ~hm) | (idx & hm) : wp;
              v0 = vmin(v0, lo);
            } else {  // one level: the sequential fold
              const float cc = cst[0][h];
              v1 = vmed3(v0, v1, cc);
              wp = cc < v0 ? (wp & ~hm) | (d0 & hm) : wp;
              v0 = vmin(v0, cc);
            }
          }
        }
      }
  };

  // one pipeline step t = c * nn + n (chunks outer, neighbours inner; the
  // chunk's first neighbour assigns E, as k_ncc_volume's PEEL)
  auto step = [&](int t, int n, int cprev, auto first) {
    constexpr bool FIRST = decltype(first)::value;
    const int n1 = n + 1 == nn ? 0 : n + 1;
    StepInfo pf{};  // horizontal: step t+2's scalars, issued now, step t+1's nxt at the end of this step
    if constexpr (!VERT) {
      if (t + 2 < T) pf = load_info(t + 2, nmod(n1 + 1));
    }
    if (NB == 1 && t > 0) {  // this step's bands into the one buffer (step 0's: before the loop)
      stage(t, n, 0);
      __syncthreads();  // vmcnt(0): landed, for every wave
    }
    u32x4* const nbuf_t = nbase + (NB == 2 ? t & 1 : 0) * nbuf;
    // A block's B entry sits at column x0b - tx, up to 3 columns left of its
    // cells' neighbour pixels: a valid cell (neighbour column 2, xx = 3) reads
    // the entry of image column -1, which the clamped DMA filled with column
    // 0's.  Where the band holds column -1 (tiles at the left image edge),
    // that entry becomes the pk plane's definition: column 0's bytes one place
    // later (its bytes 0..2 lie outside the image and meet masked taps only).
    // (K = 7: a block's entry column is its 2-wide block's first column - tx,
    // never left of a valid cell's neighbour column - 1 >= 2: nothing to fix)
    if (K == 5 && (VERT || x0 < a.txmax_all)) {  // (tiles right of every shift: never)
      const int jf = (VERT ? rec[t].txmax : cur.tx) - x0 - 1;  // band column of image column -1 (scalar)
      const int esh = VERT ? rec[t].shp : cur.shp;
      if (jf >= 0 && jf + 1 < 64 + ((esh >> 16) & 0xff)) {  // inside the band's 64 + span columns
        if (tid < a.pk_pairs) {
          u32x4* e = nbuf_t + tid * BWP + jf + ((tid & 1) ? (esh >> 24) : 0);
          const u32x4 v = e[1];
          *e = u32x4{v.x << 8, (v.y << 8) | (v.x >> 24), v.z << 8, (v.w << 8) | (v.z >> 24)};
        }
        __syncthreads();
      }
    }
    // the look-ahead: step t+1's bands into the other buffer, landing while this step computes
    if constexpr (!VERT) {
      if (t + 1 < T) stage_h(nxt, (t + 1) & 1);
    } else {
      if (NB == 2 && t + 1 < T) stage(t + 1, n1, (t + 1) & 1);
    }
    if (FIRST && cprev >= 0) fold(cprev);
    const u32x4* npk = nbuf_t;
    const u32x4* nst = npk + a.pk_pairs * BWP;
    const int ln = lane_now();
    const int g = ln >> 4;
    // per level block: the band column of the lane's level (horizontal), or
    // (VERT) the lane's B-row and stats-row addresses for block (0, 0): uint2
    // index of footprint rows o + 2g, o + 2g + 1 and float index of the a of
    // pixel rows o, o + 1 (b two floats on; rows + 2: the next pair row)
    int cl[NDB], iB0[NDB], iB1[NDB], iS0[NDB], iS1[NDB];
#pragma unroll
    for (int db = 0; db < NDB; db++) {
      const int v = colo_l[t * DC + 16 * db + (ln & 15)];
      if constexpr (!VERT) {
        cl[db] = v;
      } else {
        const int col = 8 * wave + (v & 0xff), o = v >> 8;
        const int r0 = o + 2 * g, r1 = r0 + 1, s1 = o + 1;
        iB0[db] = 2 * ((r0 >> 1) * BWP + col) + (r0 & 1);
        iB1[db] = 2 * ((r1 >> 1) * BWP + col) + (r1 & 1);
        iS0[db] = 4 * ((o >> 1) * BWP + col + g) + (o & 1);
        iS1[db] = 4 * ((s1 >> 1) * BWP + col + g) + (s1 & 1);
      }
    }
    // The lanes reading odd pk pair rows (g odd) find them sh columns along,
    // the step's bank shift: with the pitch BW + 1, lanes of one ds_read_b128
    // group read two rows 1 + sh bank quads apart, and the host picks sh per
    // step so that the column shift per level (|dx| = 1, 3 want sh = -1; 2
    // wants 0) puts their 16-byte entries on distinct quads.  K = 7: the odd-g
    // lanes' stats pairs (2, 3) likewise, st columns along
    const int sg = (!VERT && (g & 1)) ? (cur.shp >> 24) : 0;
    const int tg = (K == 7 && (g & 1)) ? ((cur.shp << 16) >> 24) : 0;
    auto bread = [&](int xb, int yb, int db, int mf) -> i32x4 {
      if constexpr (!VERT) {  // K = 5: pair 2 yb + g of the band; K = 7: pair g + 4 mf (parity g & 1 alike)
        const int pr = K == 5 ? 2 * yb + g : g + 4 * mf;
        return __builtin_bit_cast(i32x4, npk[pr * BWP + 8 * wave + BXW * xb + cl[db] + sg]);
      } else {
        const uint2* b2 = (const uint2*)npk;
        const int off = 2 * (2 * yb * BWP + 4 * xb);
        const uint2 lo = b2[iB0[db] + off], hi = b2[iB1[db] + off];
        return i32x4{(int)lo.x, (int)lo.y, (int)hi.x, (int)hi.y};
      }
    };
    // {a, a, b, b} of pixel rows 0, 1 (s0) and rows 2, 3 (s1) of the block
    auto sread = [&](int xb, int yb, int db, f32x4& s0, f32x4& s1) {
      if constexpr (!VERT) {
        const int colS = 8 * wave + pcol(xb, g) + cl[db] + tg;  // stats band column of this lane's pixel column
        const int sp = prow(yb, g) >> 1;                    // stats band pair of its first row
        s0 = __builtin_bit_cast(f32x4, nst[sp * BWP + colS]);
        s1 = __builtin_bit_cast(f32x4, nst[(sp + 1) * BWP + colS]);
      } else {
        const float* f = (const float*)nst;
        const int off = 4 * (2 * yb * BWP + 4 * xb);
        const int q0 = iS0[db] + off, q1 = iS1[db] + off, q2 = q0 + 4 * BWP, q3 = q1 + 4 * BWP;
        s0 = f32x4{f[q0], f[q1], f[q0 + 2], f[q1 + 2]};
        s1 = f32x4{f[q2], f[q3], f[q2 + 2], f[q3 + 2]};
      }
    };
    auto finish = [&](int xb, int yb, int db, const i32x4& acc, const f32x4& nsr, const f32x4& s0,
                      const f32x4& s1) {
#pragma unroll
      for (int p = 0; p < 2; p++) {
        const f32x4 sv = p ? s1 : s0;
        f32x2 xv;
        xv.x = __fmaf_rn(nsr[2 * p], sv.z, __fmul_rn(__fsub_rn(__int_as_float(acc[2 * p]), kMagicF), sv.x));
        xv.y = __fmaf_rn(nsr[2 * p + 1], sv.w, __fmul_rn(__fsub_rn(__int_as_float(acc[2 * p + 1]), kMagicF), sv.y));
        const int kb = xb * NYB + yb;
        if (FIRST) {
          E[kb][db][2 * p] = xv.x;
          E[kb][db][2 * p + 1] = xv.y;
        } else {
          E[kb][db][2 * p] = vmax(E[kb][db][2 * p], xv.x);
          E[kb][db][2 * p + 1] = vmax(E[kb][db][2 * p + 1], xv.y);
        }
      }
    };
    // one level block at a time (at the 128-VGPR cap the paired form spilled 16-40 B)
#pragma unroll
    for (int k = 0; k < (DBG == 1 ? 0 : NBL); k++) {
      const int xb = k / NYB, yb = k % NYB;
      const f32x4 nsr = *(const f32x4*)(rsn_l + (8 * wave + pcol(xb, g)) * TH + prow(yb, g));
#pragma unroll
      for (int db = 0; db < NDB; db++) {
        // the block's operand(s) and its neighbour stats issued together, ahead
        // of the MFMA: one LDS latency per block on the wave's chain, not two
        i32x4 bv[MF];
#pragma unroll
        for (int mf = 0; mf < MF; mf++) bv[mf] = bread(xb, yb, db, mf);
        f32x4 s0, s1;
        sread(xb, yb, db, s0, s1);
        __builtin_amdgcn_sched_barrier(0);
        i32x4 acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(A[k][0], bv[0], bias, 0, 0, 0);
        if constexpr (MF == 2) acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(A[k][1], bv[1], acc, 0, 0, 0);
        finish(xb, yb, db, acc, nsr, s0, s1);
      }
    }
    __syncthreads();  // NB = 2: step t+1's bands landed, this buffer free for t+2; NB = 1: free for t+1
    if constexpr (!VERT) {
      cur = nxt;
      nxt = pf;
    }
  };
  {
    int t = 0;
    for (int c = 0; c < a.nch; c++) {
      step(t++, 0, c - 1, std::true_type{});
      for (int n = 1; n < nn; n++) step(t++, n, -1, std::false_type{});
    }
  }
  fold(a.nch - 1);

  // merge the 16 level classes of every pixel through LDS (the band buffers
  // are free: every wave passed the loop's last barrier), one half tile of
  // 64 x 4 pixels at a time; one thread per pixel, k_ncc_volume's merge
  float* m0 = (float*)smem;
  float* m1 = m0 + 16 * kMfMergeStride;
  int* mi = (int*)(m1 + 16 * kMfMergeStride);
#pragma unroll
  for (int yb = 0; yb < TH / 4; yb++) {  // tile rows 4 yb .. 4 yb + 3
    {
      const int ln = lane_now(), cls = ln & 15, g = ln >> 4;
      // K = 5: block row yb; K = 7: the lanes whose rows are these (g & 1 == yb)
      const int kyb = K == 5 ? yb : 0;
      if (K == 5 || (g & 1) == yb) {
#pragma unroll
        for (int xb = 0; xb < XB; xb++)
#pragma unroll
          for (int r = 0; r < 4; r++) {
            const int kb = xb * NYB + kyb;
            const int q = cls * kMfMergeStride + r * 64 + 8 * wave + pcol(xb, g);
            // (0xffff, no level, goes as it is: above every level, D <= 65535)
            const unsigned v = (r & 1) ? wi0p[kb][r >> 1] >> 16 : wi0p[kb][r >> 1] & 0xffffu;
            m0[q] = wv0[kb][r];
            m1[q] = wv1[kb][r];
            mi[q] = (int)v;
          }
      }
    }
    __syncthreads();
    if (tid < 256) {
      const int q = tid, xx = x0 + (q & 63), yy = y0 + 4 * yb + (q >> 6);
      // lexicographic (cost, level) minimum; "no level" (0xffff) compares as
      // the largest level (it only ever comes with the initial costs 1e6, 1e6,
      // which no real level has).  Costs can be slightly negative (NCC
      // rounding past 1), so they are compared as floats.
      // every class's entries read up front (one LDS latency, not one per
      // class).  The classes' levels are distinct, so no two entries tie in
      // both keys and the minimum splits in two: the smallest cost as a min3
      // tree, then the smallest level among the classes that hold that cost.
      // The costs are never NaN (the fold's minima drop it) nor -0 (1 - m
      // rounds an exact zero to +0), so == finds exactly the classes whose
      // cost has bv's bits.
      float v0s[16], v1s[16];
      unsigned is[16];
#pragma unroll
      for (int w = 0; w < 16; w++) {
        v0s[w] = m0[w * kMfMergeStride + q];
        is[w] = (unsigned)mi[w * kMfMergeStride + q];
        v1s[w] = m1[w * kMfMergeStride + q];
      }
      const float bv = vmin16(v0s);
      unsigned ti[16];
#pragma unroll
      for (int w = 0; w < 16; w++) ti[w] = v0s[w] == bv ? is[w] : 0xffffffffu;
      const unsigned bi = vmin16u(ti);
      // the second smallest outside bi +- 1: a class whose level lies there
      // gives its own second smallest (both are <= the initial cost kWtaInit;
      // a class with no level holds that cost twice, so its test is immaterial)
      const unsigned bl = bi - 1u;
      float sv[16];
#pragma unroll
      for (int w = 0; w < 16; w++) sv[w] = is[w] - bl <= 2u ? v1s[w] : v0s[w];
      float c2 = vmin16(sv);
      // The fold skipped the clamp (cost = 1 - max(-1, m) = min(2, 1 - m)).
      // If the smallest cost is below 2 the clamp changes neither it nor its
      // level, and the second smallest outside bi +- 1 is min(2, that) whenever
      // such a level exists; otherwise every level costs 2 and the first level
      // wins with confidence 0 (k_wta's strict <, in level order).
      const bool all2 = !(bv < 2.0f);
      const int b = (int)bi;
      if (!all2 && a.D > min(b + 1, a.D - 1) - max(b - 1, 0) + 1) c2 = vmin(c2, 2.0f);
      if (xx < W && yy < H) {
        const long p = P * ref + (long)yy * W + xx;
        wo.disp[p] = a.D <= 0 ? 0.0f : wo.levels[all2 ? 0 : b];
        if (wo.conf) wo.conf[p] = (all2 || c2 == kWtaInit) ? 0.0f : c2 - bv;
      }
    }
    __syncthreads();
  }
}


// Host side: an NccLaunch of the matrix-core family (ncc_plan.cpp decides its
// coordinates) mapped to its k_ncc_mfma instantiation.
template <int K, int BW, bool TAIL, bool VERT, int NDB, int NB, int DBG = 0>
int launch_mfma_bw(const NccCall& c) {
  auto kern = k_ncc_mfma<K, BW, TAIL, VERT, NDB, NB, DBG>;
  MVS_HIP(raise_lds(c.ctx, (const void*)kern, c.L.lds), "hipFuncSetAttribute(ncc mfma lds)");
  const auto ev = kernel_events(c.ctx);  // (timing off: plain launch)
  hipExtLaunchKernelGGL(kern, dim3(8 * c.L.args.tiles_per_xcd), dim3(512), c.L.lds, c.ctx->stream, ev.first, ev.second,
                        0, c.stats, c.pk, (const NccMRec*)c.plan, c.L.args, c.wo);
  MVS_LAUNCH_CHECK("k_ncc_mfma (fused WTA)");
  return 0;
}

// lists with vertical / diagonal neighbours (K = 5): pitch 80 | 96 | 128
template <bool TAIL, int NDB, int NB>
int launch_vert(const NccCall& c) {
  switch (c.L.BW) {
    case 80: return launch_mfma_bw<5, 80, TAIL, true, NDB, NB>(c);
    case 96: return launch_mfma_bw<5, 96, TAIL, true, NDB, NB>(c);
    case 128: return launch_mfma_bw<5, 128, TAIL, true, NDB, NB>(c);
  }
  return no_kernel();
}

// the timing probes (MVS_NCC_MFMA_DBG): C5's, C2's and C4's interior lists' forms
template <int DBG>
int launch_probe(const NccCall& c) {
  const NccLaunch& L = c.L;
  if (L.TAIL || L.NB != 2) return no_kernel();
  if (L.K == 7 && !L.VERT && L.BW == 128 && L.NDB == 1) return launch_mfma_bw<7, 128, false, false, 1, 2, DBG>(c);
  if (L.K == 5 && !L.VERT && L.BW == 192 && L.NDB == 2) return launch_mfma_bw<5, 192, false, false, 2, 2, DBG>(c);
  if (L.K == 5 && L.VERT && L.BW == 80 && L.NDB == 1) return launch_mfma_bw<5, 80, false, true, 1, 2, DBG>(c);
  return no_kernel();
}

}  // namespace

int launch_ncc_mfma(const NccCall& c) {
  const NccLaunch& L = c.L;
  if (L.DBG) return L.DBG == 1 ? launch_probe<1>(c) : launch_probe<2>(c);
  if (L.VERT) {  // K = 5: 16 NDB levels per chunk, NB band buffers
    if (L.K != 5) return no_kernel();
    const int form = 10 * L.NDB + L.NB;
    if (form == 22) return L.TAIL ? launch_vert<true, 2, 2>(c) : launch_vert<false, 2, 2>(c);
    if (form == 21) return L.TAIL ? launch_vert<true, 2, 1>(c) : launch_vert<false, 2, 1>(c);
    if (form == 12) return L.TAIL ? launch_vert<true, 1, 2>(c) : launch_vert<false, 1, 2>(c);
    if (form == 11) return L.TAIL ? launch_vert<true, 1, 1>(c) : launch_vert<false, 1, 1>(c);
    return no_kernel();
  }
  // horizontal lists: pitch 128 | 192, the tail kernels 192
  if (L.K == 7 && L.NDB == 1) {  // 16-level chunks
    if (L.TAIL) return L.BW == 192 && L.NB == 2 ? launch_mfma_bw<7, 192, true, false, 1, 2>(c) : no_kernel();
    if (L.BW == 128 && L.NB == 2) return launch_mfma_bw<7, 128, false, false, 1, 2>(c);
    return L.BW == 192 && L.NB == 2 ? launch_mfma_bw<7, 192, false, false, 1, 2>(c) : no_kernel();
  }
  if (L.K != 5 || L.NDB != 2 || L.NB != 2) return no_kernel();
  if (L.TAIL) return L.BW == 192 ? launch_mfma_bw<5, 192, true, false, 2, 2>(c) : no_kernel();
  if (L.BW == 128) return launch_mfma_bw<5, 128, false, false, 2, 2>(c);
  return L.BW == 192 ? launch_mfma_bw<5, 192, false, false, 2, 2>(c) : no_kernel();
}

}  // namespace ncc
}  // namespace mvs
