// The launch planners of the SLIC stage, the superpixel sweep, the per-pixel
// SAD sweep and the view-consistency filter: every host-side decision of
// launch_slic, launch_sweep_spixl, launch_sweep_pixel_sad and
// launch_remove_incons (the SLIC launch sequence and its shared scratch, kernel
// form, grids, the re-layout slot table, the SAD step records, LDS bytes) as
// plain C++ with no HIP header and no mvs_ctx, so it builds with g++ and runs
// without a GPU (tests/host/launch_plan_check.cpp prints its decisions).
// slic.hip, sweep.hip, sad.hip and refine.hip map a plan to a kernel
// instantiation and launch it.  The structs and constants below that a kernel
// reads too are defined here once.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

namespace mvs {

inline int map_dim(int n, int S) {
  // (int)ceil((float)n / (float)S), pipeline.cpp:18-19
  return (int)__builtin_ceilf((float)n / (float)S);
}

// ---- shared with the SLIC kernels (slic.hip) --------------------------------
constexpr int kLocal = 16;  // LOCAL_SIZE_UPDATE, header.h:37-38: the update's tile edge
constexpr int kAssignTW = 64, kAssignTH = 16;  // k_assign's pixel tile (AS_TW, AS_TH)

// ---- shared with k_sweep_spixl_ring (sweep.hip) ----------------------------
constexpr int kSwU = 336;  // C5 (S = 40, |dx| <= 4): 78 + 2 + 252 = 332

// ---- shared with k_sweep_spixl* (sweep.hip) and k_sweep_pixel_sad (sad.hip) --
struct SweepArgs {
  int V, W, H, mw, mh, D, aw, z;
  float bl;
};
constexpr float SB_INIT = 1000000.0f;  // initial_depth_estimation_v2's initial cost: every SAD sweep form's minima start here

// ---- shared with k_sad_band / k_sweep_pixel_sad (sad.hip) ------------------
constexpr int SB_TW = 60;   // output columns per tile
constexpr int SB_NBLK = 2;  // 64-column blocks per band row (band columns <= 128)
struct SadArgs {
  int W, H, D, nn, z;
  int tiles_x, ntiles, tiles_per_xcd, nch;
  int bw, brows;  // LDS band pitch (pixels) and rows per buffer
};
// host-built plan, one record per step (c, n), read by scalar loads
struct alignas(16) SadRec {
  int view, sxmin, sxmax, pad0;
  float fdymin, fdymax;
  int pad1[2];
  int sx[16];     // per level j of the chunk: column shift d*dx (integral)
  float fdy[16];  // per level j: (bl*d)*dy, the reference's float row shift
};
static_assert(sizeof(SadRec) == 160, "SadRec is uploaded as 40 int32 words");
constexpr int PT = 32;           // output tile edge

// ---- shared with k_remove_incons_q (refine.hip) ----------------------------
constexpr int kFilterRG = 4;  // reference views per workgroup of the q kernel

namespace plan {

// Every knob of the four launchers.  plan_tuning() is the one place that
// reads them, all of them per call.
struct Tuning {
  bool slic_tiles9 = false;     // MVS_SLIC_TILES9=1: the 9-cell k_assign_tiles where k_assign_tiles4 would run (A/B)
  bool slic_update_walk = true;  // MVS_SLIC_UPDATE=0: k_update where k_update_walk would run (A/B)
  int sweep_wps = 0;        // MVS_SWEEP_WPS=1|2|4: another wave count per superpixel (0: automatic; ignored at D <= 32)
  int sweep_transpose = 2;  // MVS_SWEEP_TRANSPOSE: 0 row-major gathers only, 1 vertical neighbours re-laid, 2 diagonal ones too
  bool sweep_hz = true;     // MVS_SWEEP_HZ=0: the general form where HZ would run
  bool sweep_ring = true;   // MVS_SWEEP_RING=0: the HZ gathers where the ring form would run
  // MVS_SWEEP_RING_FAST=0: the ring kernel's general row-steps where its whole-window path would run (A/B; a
  // kernel argument, no part of the plan)
  bool sweep_ring_fast = true;
  // MVS_SAD_KERNEL: "sys8x2", "sys8", "gather"; unset: 16-level chunks, else
  // 8-level chunks (taller bands: vertical neighbours), else the gather kernel.
  // A band variant named explicitly never falls back (MVS_E_UNSUPPORTED), so a
  // test of it cannot pass on another.
  std::string sad_kernel = "auto";
  bool sad_named = false;    // MVS_SAD_KERNEL is set
  bool sad_aff = true;       // MVS_SAD_AFF set (any value): the row-table path
  bool filter_px = false;    // MVS_FILTER_KERNEL=px: the per-pixel form at 16 < V <= 32
  int filter_fb_q = 2;       // MVS_FILTER_FB, views per gather block: the q kernel takes 4, else 2
  int filter_fb_px = 4;      //   the px kernel takes 4 or 2, else 8 (its default is 4, q's is 2)
  int filter_ns = 2;         // MVS_FILTER_NS: candidate slots per lane (1, else 2)
  bool filter_bound = true;  // MVS_FILTER_BOUND=0: the walk's bounds over every view
  bool filter_ref_order = false;  // MVS_FILTER_ORDER=ref: the q kernel's grid as (x tiles, rows, reference groups)
};
Tuning plan_tuning();

// ---- launch_slic --------------------------------------------------------------
enum SlicKernel {
  kSlicInitCenters, kSlicEdge, kSlicEdgeStore, kSlicApplyEdge,
  kSlicAssign,          // k_assign<S3>
  kSlicAssignTiles9,    // k_assign_tiles<S3>
  kSlicAssignTiles4,    // k_assign_tiles4<S16>
  kSlicUpdateFinalize,  // k_update_finalize<CPL>
  kSlicUpdateWalk,      // k_update_walk<UT, uintLT_t>
  kSlicUpdate,          // k_update<UT, uintLT_t>
  kSlicSuppress
};
// One launch.  A kernel's pointer arguments are the caller's lab, spixl and
// labels or the context scratch; the flags say which where there is a choice.
struct SlicStep {
  SlicKernel kernel;
  // the template coordinates (0 where the kernel has none): S3 the 3x3
  // candidate loop (search); S16 = S / 16 (2 | 4); CPL 6 | 0; UT tiles per
  // chunk 4 | 1; LT the width of the labels an update reads, 16 | 32
  int S3, S16, CPL, UT, LT;
  unsigned grid[3], block;
  bool labels;      // an assignment stores the 32-bit labels (else it gets null: an update follows that does not read them)
  bool lb16;        // k_assign stores 16-bit label copies into the scratch (else null); LT = 16 reads them there
  bool part;        // a tile assignment stores the next update's tile partials into the scratch (else null)
  bool to_scratch;  // k_suppress: labels -> scratch (else scratch -> labels)
};
// The whole stage: init centres, the edge step (edge_enable 1: k_edge,
// k_edge_store; 2: k_edge, k_apply_edge), then assign -> (update -> assign) x
// no_iter, then two k_suppress passes (enforce_connectivity).
//  * S % 16 == 0, the tile path: every assignment an update follows produces
//    that update's tile partials itself and stores no labels (one Lab read per
//    iteration); the update is k_update_finalize's sum of them.
//  * else: k_assign, and k_update_walk over the labels (k_update: when the
//    walk's 32-bit byte offsets do not cover a view, W H 16 >= 2^31, or by
//    MVS_SLIC_UPDATE=0).  With mw mh <= 65536 and no_iter > 0 the updates read
//    16-bit copies of the labels: an assignment an update follows writes only
//    them, the last one only the 32-bit labels.
// One scratch of scratch_bytes (0: none) serves four users whose lifetimes do
// not overlap, so it is the largest of them:
//  1. the edge magnitude plane (V W H floats): k_edge writes it, k_edge_store /
//     k_apply_edge read it, all before the first assignment;
//  2. the tile partials (S % 16 == 0; 6 G floats per superpixel): written by
//     an assignment, read by the k_update_finalize after it;
//  3. the 16-bit labels (never with 2: S % 16 != 0): written by an
//     assignment, read by the update after it;
//  4. the connectivity pass's second label buffer (V W H uint32): after the
//     last assignment, which writes neither 2 nor 3.
struct SlicPlan {
  int V = 0, W = 0, H = 0, S = 0;
  int mw = 0, mh = 0;
  float xy = 0, col = 0;  // clSLIC's squared distance normalisers
  // num_grid_per_center, cluster_per_line (clSLIC.cpp:20-21, 313) and the
  // image's 16 x 16 tile grid
  int G = 0, cpl = 0, ntx = 0, nty = 0;
  size_t scratch_bytes = 0;
  std::vector<SlicStep> steps;  // in launch order
};
// The caller has checked the arguments (mvs_slic_d: S in [6, 96], no_iter >= 0, ...).
SlicPlan plan_slic(const Tuning& t, int V, int W, int H, int S, int no_iter, int edge_enable, int search,
                   int enforce_connectivity);

// ---- launch_sweep_spixl -----------------------------------------------------
// the form of a launch, as mvs_sweep_last_variant_n reports it
constexpr int kSweepGeneral = 0, kSweepHzGather = 1, kSweepHzRing = 2, kSweepRelaid = 3;
struct SpixlRelayout {
  int view, kind, slot;  // k_relayout_lab<kind> of `view` to labT + slot * tstride
};
struct SpixlSweepPlan {
  const char* err = nullptr;  // the argument error, if any
  bool launch = false;        // false: nothing to do (an empty view range)
  int form = 0, lps = 64, wps = 1;  // k_sweep_spixl<lps, form == relaid, form == HZ>(wps) or k_sweep_spixl_ring<wps>
  int mw = 0, mh = 0;
  unsigned grid_x = 0, grid_y = 0;
  // re-laid neighbour views: slot[4 * view + kind] in units of tstride
  // elements, -1 none (empty without re-laid views); the copies in launch order
  std::vector<int32_t> slot;
  std::vector<SpixlRelayout> relayouts;
  long units = 0, tstride = 0;
  int last[5] = {0, 0, 0, 0, 0};  // {FORM, LPS, WPS, TMODE, RELAID}
};
// vs, sn, levels: the host lists.  allow_relayout = false: the plan of the
// same call without the re-layout scratch (it may then be HZ or ring).
SpixlSweepPlan plan_sweep_spixl(const Tuning& t, int V, int W, int H, int S, int D, const float* levels,
                                const int* vs, const int* sn, int aw, int z0, int z1, bool allow_relayout);

// ---- launch_sweep_pixel_sad -------------------------------------------------
struct SadPlan {
  bool band = false;  // k_sad_band<TH, PPW, AFF, BWT>, else k_sweep_pixel_sad
  int TH = 0, PPW = 0, AFF = 0, BWT = 0;
  std::vector<int32_t> table;  // the SadRec of every step (c, n)
  SadArgs args{};
  size_t lds = 0;
  unsigned grid_x = 0, grid_y = 1;
  std::string err;  // MVS_E_UNSUPPORTED: a named variant cannot stage this geometry
};
// The band form of DC = 8 PPW levels per step and RR = TH + 4 region rows for
// reference view z: false when the level set has fractional column shifts or
// the bands do not fit the LDS; else p's table, args (the work map included),
// lds, AFF and BWT are filled.
bool sad_band_geometry(int DC, int RR, bool aff, int V, int W, int H, int D, const float* levels, const int* vs,
                       const int* sn, int aw, float bl, int z, SadPlan& p);
SadPlan plan_sad(const Tuning& t, int V, int W, int H, int D, const float* levels, const int* vs, const int* sn,
                 int aw, float bl, int z);

// ---- launch_remove_incons ---------------------------------------------------
enum FilterKernel { kFilterNone, kFilterSel8, kFilterPx16_8, kFilterQ, kFilterPx32, kFilterSel64, kFilterPlain };
struct FilterPlan {
  FilterKernel kernel = kFilterNone;  // none: no rows or no views
  int FB = 0, NS = 0, ROWB = 0, RM = 0;  // q: k_remove_incons_q<kFilterRG, FB, NS, ROWB, RM>; px32: FB
  int inb = 0;                           // q: the walk's bounds from the array's rows
  unsigned grid[3] = {0, 1, 1}, block = 256;
  long PP = 0;        // proj's view stride in elements
  long proj_off = 0;  // added to proj: a band holds rows [ya, yb) only
};
FilterPlan plan_remove_incons(const Tuning& t, int V, int W, int H, int aw, int z0, int z1, int ya, int yb,
                              bool band);

// ---- launch_sgm (sgm.hip; the kernels: sgm_kernels.h, on cost type C) -------
// One path of the semi-global aggregation (include/mvs.h at mvs_sgm_d) over a
// volume [D][H][W].  path: 0 left->right, 1 right->left (lines = rows, n = W
// steps), 2 top->bottom, 3 bottom->top (lines = columns, n = H steps).
//  * kSgmLanes, k_sgm_lanes<C, lpl, vec, waves > 1>: one workgroup of `waves`
//    waves per line, every lane keeps lpl consecutive levels of the previous
//    pixel in registers and walks the line; element i of line l of a level's
//    plane is at l * lstride + i * sstride.  vec: the line is contiguous
//    (sstride 1) and is read and written in aligned 16-byte pieces where a
//    piece lies inside it (the launcher falls back to vec = false when vol and
//    agg are not equally aligned mod 16 bytes).  One wave up to kSgmLanesOneWave
//    levels; above, waves of 64 x 16 levels that meet in LDS once per step.
//  * kSgmColumns, k_sgm_columns: vertical paths at D <= kSgmColumnsMaxD.  A
//    workgroup takes 64 consecutive columns, lanes over x (a level's row piece
//    is one coalesced 256 bytes), wave w keeps levels [lpl w, lpl (w + 1)) and
//    the waves meet in LDS once per row (k_sgm_columns<512> up to 8 waves,
//    <1024> above: the thread limit decides the register budget).
// Vertical paths above kSgmColumnsMaxD levels take the lanes form with
// sstride = W.
constexpr int kSgmLanes = 0, kSgmColumns = 1;
constexpr int kSgmMaxLpl = 16;                         // levels per lane of the lanes form: 1, 2, 4, 8, 16
constexpr int kSgmLanesOneWave = 64 * kSgmMaxLpl;      // 1024 levels
constexpr int kSgmColumnsLpw = 16;                     // levels per wave of the columns form
constexpr int kSgmColumnsMaxD = 16 * kSgmColumnsLpw;   // 256 levels: 16 waves
constexpr int kSgmMaxD = 16 * kSgmLanesOneWave;        // 16384 levels: 16 waves of the lanes form
struct SgmPlan {
  const char* err = nullptr;  // the argument error, if any
  int form = kSgmLanes;
  int lpl = 1;         // levels per lane (lanes form) or per wave (columns form)
  int waves = 1;       // per workgroup
  bool vec = false;    // lanes form: 16-byte pieces
  int n = 0, lines = 0;  // steps of a path; rows or columns
  int sstride = 0, lstride = 0;
  int sx = 0;          // plan_sgm_diag: the column's step per image row
  bool rev = false;    // walk from the line's last element (sheared form: the last row) down
  unsigned grid = 0, block = 0;
  size_t lds = 0;      // static LDS of the kernel form, bytes
};
SgmPlan plan_sgm(int W, int H, int D, int path);

// One diagonal path (include/mvs.h at mvs_sgm8_d): path 4 steps (+1, +1) per
// pixel, 5 (-1, -1), 6 (-1, +1), 7 (+1, -1).  Paths 4 and 5 walk the W + H - 1
// lines x - y = const, 6 and 7 the lines x + y = const; along such a line the
// column moves by sx = +1 (4, 5) or -1 (6, 7) per image row.  4 and 6 walk the
// rows downwards, 5 and 7 upwards (rev).
//  * kSgmSheared, k_sgm_diag, D <= kSgmColumnsMaxD: the columns form, sheared.
//    Workgroup g takes 64 consecutive lines, one per lane; at image row y the
//    lane stands on column sgm_diag_x0(g, lane, H, sx) + sx * y and is live
//    there iff that lies in [0, W).  The workgroup walks the rows
//    [sgm_diag_ylo, sgm_diag_yhi], the rows at which some lane is live, in the
//    path's order; levels over the waves as in the columns form.
//  * kSgmLanes, k_sgm_lanes<C, lpl, false, waves > 1, true> above: one workgroup
//    per line; sgm_diag_line gives the line's topmost pixel and its length,
//    and its elements are sstride = W + sx apart.
// The plan is an SgmPlan as the launcher passes it on: lines = W + H - 1, and W and H travel in the places of n
// and lstride (k_sgm_lanes at DIAG takes them there); lpl counts levels per wave in the sheared form.
constexpr int kSgmSheared = 2;
constexpr int sgm_diag_x0(int g, int lane, int H, int sx) { return sx > 0 ? 64 * g - (H - 1) + lane : 64 * g + lane; }
constexpr int sgm_diag_ylo(int g, int W, int H, int sx) {
  const int y = sx > 0 ? H - 1 - 64 * g - 63 : 64 * g - (W - 1);
  return y > 0 ? y : 0;
}
constexpr int sgm_diag_yhi(int g, int W, int H, int sx) {
  const int y = sx > 0 ? W + H - 2 - 64 * g : 64 * g + 63;
  return y < H - 1 ? y : H - 1;
}
struct SgmDiagLine {
  int first, n;  // the topmost pixel's offset in a plane; pixels on the line
};
// line l in [0, W + H - 1): x - y = l - (H - 1) for sx = +1, x + y = l for sx = -1
constexpr SgmDiagLine sgm_diag_line(int W, int H, int sx, int l) {
  const int c = l - (H - 1);
  const int xt = sx > 0 ? (c > 0 ? c : 0) : (l < W ? l : W - 1);
  const int yt = sx > 0 ? (c < 0 ? -c : 0) : (l < W ? 0 : l - (W - 1));
  const int nx = sx > 0 ? W - xt : xt + 1, ny = H - yt;
  return {yt * W + xt, nx < ny ? nx : ny};
}
SgmPlan plan_sgm_diag(int W, int H, int D, int path);

// N volumes of one shape per launch (include/mvs.h at mvs_sgm8_batch_d and mvs_sgm8_u16_batch_d): element i is the
// volume at vol + i * vol_stride and its aggregate at agg + i * agg_stride (addresses in bytes, strides in
// elements).  The batch index is the grid's second axis, so every launch of plan_sgm / plan_sgm_diag becomes
// (grid, grid_y).  An SgmCost holds what the cost type sets: float32, or the 16-bit integer costs of sgm16.hip,
// whose paths have plan_sgm's and plan_sgm_diag's geometry as it is (D <= kSgm16MaxD: the lanes form with 1, 2 or
// 4 levels per lane and one wave for the horizontal paths, the columns form for the vertical ones, the sheared
// form for the diagonal ones).  The rules, in this order:
//  * err: bad dimensions; more than max_d levels (with `unsupported` set where the cost type says so: the forms
//    for more are left out, not impossible); N outside 1..kSgmMaxBatch; for 2-byte elements an address that is no
//    multiple of 2; a stride below D H W; the two spans
//    [addr, addr + element size * ((N - 1) stride + D H W)) overlap (abutting spans do not).
//  * vec_ok: the 16-byte-pieces form of k_sgm_lanes needs vol and agg equal mod 16 bytes in every element: the
//    bases are, and with N > 1 the strides differ by a multiple of `piece` elements.  (The strides themselves need
//    be no multiple of it: a (lane, level)'s phase comes from its real address.)  Else the whole batch takes the
//    element-wise form.
constexpr int kSgmMaxBatch = 65535;  // one grid axis
constexpr int kSgm16MaxD = kSgmColumnsMaxD;  // 256 levels: the forms for more are left out
constexpr int kSgm16MaxCost = 4094, kSgm16MaxP = 4095;
constexpr int kSgmPiece = 4, kSgm16Piece = 8;  // float32, uint16 pixels per 16-byte piece
struct SgmCost {
  int piece;         // pixels per 16-byte piece (a power of two): an element has 16 / piece bytes
  int max_d;         // the level limit
  bool unsupported;  // more levels are "unsupported", not bad dimensions
};
constexpr SgmCost kSgmF32 = {kSgmPiece, kSgmMaxD, false}, kSgmU16 = {kSgm16Piece, kSgm16MaxD, true};
struct SgmBatchPlan {
  const char* err = nullptr;  // the argument error, if any
  bool unsupported = false;   // err is "more levels than the forms built take"
  unsigned grid_y = 0;
  bool vec_ok = false;
};
SgmBatchPlan plan_sgm_batch(SgmCost cost, int W, int H, int D, int N, uintptr_t vol_addr, size_t vol_stride,
                            uintptr_t agg_addr, size_t agg_stride);
// The 16-byte pieces of k_sgm_lanes, for both cost types: a piece holds `piece` pixels of 16 / piece bytes.
//  * sgm_piece_vec_ok: vol and agg are equal mod 16 bytes in every element of the batch (strides in elements).
//  * sgm_piece_phase: for a (lane, level) whose line starts at byte address a, pixel x is element
//    j = sgm_piece_elem = (x + ph) mod piece, ph = (a / element size) mod piece, of the piece of pixels
//    x - j .. x - j + piece - 1, which starts at a multiple of 16 bytes.
//  * sgm_piece_inside: that piece lies inside the line of n pixels (it is then read and written whole; else its
//    pixels are handled one by one).
// tests/host/sgm16_plan_check.cpp checks them against brute force at both piece sizes.
constexpr bool sgm_piece_vec_ok(int piece, int N, uintptr_t vol_addr, size_t vol_stride, uintptr_t agg_addr,
                                size_t agg_stride) {
  return ((vol_addr ^ agg_addr) & 15) == 0 && (N == 1 || ((vol_stride - agg_stride) & (size_t)(piece - 1)) == 0);
}
constexpr int sgm_piece_phase(int piece, uintptr_t line_addr) {
  return (int)((line_addr / (uintptr_t)(16 / piece)) & (uintptr_t)(piece - 1));
}
constexpr int sgm_piece_elem(int piece, int ph, int x) { return (x + ph) & (piece - 1); }
constexpr bool sgm_piece_inside(int piece, int ph, int x, int n) {
  return x - sgm_piece_elem(piece, ph, x) >= 0 && x - sgm_piece_elem(piece, ph, x) + piece - 1 < n;
}

}  // namespace plan
}  // namespace mvs
