/* mvs.h -- C-ABI of the MI355X multi-view-stereo depth engine (libmvs.so).
 *
 * Drop-in boundary for the reference's hot path.  The reference has no plugin
 * API: its host stage classes enqueue OpenCL kernels by name.  Each entry point
 * below replaces one of those stage methods / kernel groups (file:line of the
 * reference interface in the comment), takes the reference's data layouts
 *  as plain pointers + sizes, and returns 0 or a negative
 * MVS_E_* status (the reference prints cl_int errors and carries on;
 * errorHandler, file_handler.cpp:97-113 -- here every failure is returned).
 *
 * Two flavours:
 *   mvs_*      host pointers; copy in, run on the context's GPU, copy out,
 *              synchronous (what the reference stage methods do).
 *   mvs_*_d    device pointers, enqueued on the context's HIP stream, async.
 *
 * Layouts (all arrays view-major, row-major):
 *   rgbx   uint8 [V][H][W][4]  s0=R, s1=G, s2=B (loadImageIn, file_handler.cpp:6-14)
 *   lab    float [V][H][W][4]  CIE-Lab + pad  (cl_float3)
 *   l8     uint8 [V][H][W]     8-bit intensity for the NCC cost (build-defined)
 *   spixl  float [V][mh][mw][8] {id, cx, cy, L, a, b, count, disparity}
 *   labels uint32 [V][H][W]    per-view superpixel index y*mw+x
 *   rep    uint8 [V][mh][mw][8] ray extents {NW,W,SW,N,S,NE,E,SE}
 *   levels float [D]           disparity hypotheses
 *   view_subset int32 [V][V] (row z = neighbour list of z), subset_num int32 [V]
 *   state  float [V][mh][mw][6] {d, sm, cs, nx, ny, nz}
 *   disp   float [V][H][W]     disparity in pixels (depth-map output)
 *   mw = ceil(W/S), mh = ceil(H/S) (pipeline.cpp:18-19)
 *
 * Not thread-safe per context.  One context per GPU; one process per GPU.
 */
#ifndef MVS_H
#define MVS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
  MVS_OK = 0,
  MVS_E_ARG = -1,      /* invalid argument / shape */
  MVS_E_HIP = -2,      /* HIP runtime error */
  MVS_E_NOMEM = -3,    /* device allocation failed */
  MVS_E_UNSUPPORTED = -4
};

typedef struct mvs_ctx mvs_ctx;

/* SLIC parameters: system_settings fields used by clSLIC (header.h:55-77).
 * ABI 0.3 (mvs_version): struct_size must be sizeof(mvs_slic_params) -- a
 * caller built against an older mvs.h (0.1: four ints, no size field) is
 * refused with MVS_E_ARG instead of having its fields misread. */
typedef struct {
  uint32_t struct_size;      /* = sizeof(mvs_slic_params) */
  int spixl_size;            /* S */
  float color_weight;        /* slic_color_weight (clMVDE.cpp:16 = 0.6) */
  int no_iter;               /* update/assign iterations (5) */
  int enforce_connectivity;  /* supress_local_lable x2 (clSLIC.cpp:373-411) */
  int edge_enable;           /* apply_edge_values (clSLIC.cpp:84-86, 186-233; clcode.cl:161-248):
                              * 0 off (the reference's default, header.h:61);
                              * 1 the reference's path as it behaves: the edge magnitude
                              *   overwrites the Lab image (L = a = b = e) and no centre moves
                              *   (apply_edge_alternative reads the never-written edge_img,
                              *   pinned as zeros);
                              * 2 the intended path: Lab kept, each centre moves to its
                              *   least-edge 8-neighbour and takes its colour. */
  int search;                /* candidate centres of find_center_association:
                              * 0 the active loop (clcode.cl:474-494: 2x2 cells, x/y
                              *   deltas swapped) -- the reference's default;
                              * 1 the 3x3 loop behind the reference's comment switch
                              *   (clcode.cl:496-516), with which its kept depth outputs
                              *   were produced. */
} mvs_slic_params;

/* Camera array / hypothesis set (pipeline::perform_depth_est).  Its arrays are
 * small metadata and are HOST pointers in both API flavours; the context keeps
 * a device copy (re-uploaded only when the contents change). */
typedef struct {
  int view_count;            /* V */
  int array_width;           /* cameras per row */
  float bl_ratio;            /* vertical / horizontal baseline ratio */
  const float* levels;       /* [D] host pointer */
  int num_levels;            /* D */
  const int32_t* view_subset;/* [V][V] */
  const int32_t* subset_num; /* [V] */
} mvs_array;

/* Refinement parameters (system_settings; clDepthRefinement::do_refinement).
 * ABI 0.3: struct_size must be sizeof(mvs_refine_params). */
typedef struct {
  uint32_t struct_size;      /* = sizeof(mvs_refine_params) */
  float gamma;               /* settings->gamma (2), or gamma' with prescaled = 1 */
  float alpha;               /* settings->alpha (6), or alpha' with prescaled = 1 */
  float fuse;                /* settings->fuse (1) */
  int kernel_step;           /* settings->kernel_step (13) */
  int kernel_size;           /* settings->kernel_size (1080), or its half with prescaled = 1 */
  int no_prop;               /* propagate iterations (5) */
  int fusion_compat;         /* 1: render current_state_dev as the reference does */
  int prescaled;             /* 0: the library applies pipeline::refine_depth_map's derivation
                              *    (pipeline.cpp:164-166: gamma' = 2 gamma^2, alpha' = 2 alpha^2,
                              *    kernel_size / 2);
                              * 1: gamma, alpha, kernel_size already are those values -- the
                              *    arguments clDepthRefinement::do_refinement receives
                              *    (depth_refinement.h:9), for a drop-in of that method */
} mvs_refine_params;

/* ---- context ----------------------------------------------------------- */
int mvs_create(int device, mvs_ctx** out);
void mvs_destroy(mvs_ctx* ctx);
const char* mvs_last_error(void);
int mvs_set_stream(mvs_ctx* ctx, void* hip_stream);   /* NULL = default stream */
int mvs_synchronize(mvs_ctx* ctx);
const char* mvs_version(void);

/* ---- device-pointer stage API ------------------------------------------ */
/* cvt kernel (clcode.cl:125-151) over V views; l8 may be NULL. */
int mvs_cvt_d(mvs_ctx* ctx, const uint8_t* rgbx, int V, int W, int H, float* lab, uint8_t* l8);

/* SLIC on V views of lab (clSLIC::do_super_pixel_seg, clSLIC.cpp:67-122,
 * minus the cvt it starts with).  spixl [V][mh][mw][8], labels [V][H][W].
 * lab is read only, except with p->edge_enable == 1, where the reference's
 * edge step overwrites it (as clSLIC's lab_img_dev).  Every spixl word is
 * written; s7 (disparity, untouched by the reference's SLIC on its zeroed
 * buffer) is set to 0.
 * W <= 65536 and H <= 65536 (otherwise the "bad arguments" failure, from
 * mvs_do_super_pixel_seg as well): the centre update sums a 16 x 16 tile's
 * member x and y as one integer converted to float, which equals the
 * reference's float tree only while that sum is exact in float -- 256 members
 * of x <= 65535 stay below 2^24 (likewise y).  The kernels' multiply-high
 * division by S, exact below 2^32 / S, is far inside its range there. */
int mvs_slic_d(mvs_ctx* ctx, float* lab, int V, int W, int H, const mvs_slic_params* p,
               float* spixl, uint32_t* labels);

/* SLIC-off grid mode: init_cluster_centers + init_label_per_pixl
 * (clcode.cl:259-294, 341-353). */
int mvs_grid_d(mvs_ctx* ctx, const float* lab, int V, int W, int H, int S, float* spixl, uint32_t* labels);

/* find_super_pixel_boundary (clcode.cl:791-855; photo_consistency.cpp:88-110). */
int mvs_boundary_d(mvs_ctx* ctx, int V, int W, int H, int S, const float* spixl, const uint32_t* labels,
                   uint8_t* rep);

/* initial_depth_estimation_v2 for reference views [z0, z1): writes spixl.s7
 * (clcode.cl:972-1069; photo_consistency.cpp:113-140). */
int mvs_sweep_spixl_d(mvs_ctx* ctx, int W, int H, int S, const float* lab, float* spixl, const uint8_t* rep,
                      const mvs_array* a, int z0, int z1);

/* The same sweep evaluated at S=1 grid semantics (per-pixel SAD, reference
 * parity mode) without materialising spixl: disp [z1-z0][H][W]. */
int mvs_sweep_pixel_sad_d(mvs_ctx* ctx, int W, int H, const float* lab, const mvs_array* a, int z0, int z1,
                          float* disp);

/* Build-defined per-pixel NCC KxK plane sweep (definition: csrc/ncc.hip).
 * box int32 [2][V][Hp][W][2] (Hp = H rounded up to even; 16 B/px), from
 * mvs_box_stats_d, rows stored pairwise interleaved: plane 0 per row pair
 * (2m, 2m+1) and column x the float4 {a(2m), a(2m+1), b(2m), b(2m+1)} with
 * s = 1/sqrt(n*sum q^2 - (sum q)^2) (0 if textureless, NaN if the window
 * leaves the image), a = n*s, b = (sum q - 128 n)*s; plane 1 the centred
 * packed intensities q-128 of columns x-R .. x-R+7 of each pixel's row (two
 * little-endian dwords at uint2 index ((y>>1)*W + x)*2 + (y&1)).
 * vol [D][H][W] float cost of reference view z = 1 - max(-1, best NCC over
 * valid neighbour windows); l8 is validated only. */
int mvs_box_stats_d(mvs_ctx* ctx, const uint8_t* l8, int V, int W, int H, int K, int32_t* box);
/* The same planes for views [z0, z1) only of a V-view box buffer (a view shard
 * converts just its block and the block's neighbours). */
int mvs_box_stats_range_d(mvs_ctx* ctx, const uint8_t* l8, int V, int W, int H, int K, int z0, int z1,
                          int32_t* box);
int mvs_ncc_volume_d(mvs_ctx* ctx, int W, int H, const uint8_t* l8, const int32_t* box, const mvs_array* a,
                     int K, int z, float* vol);
/* Winner-take-all over vol [D][H][W]: disp = levels[first argmin], conf =
 * (min cost outside best+-1) - best cost.  conf may be NULL. */
int mvs_wta_d(mvs_ctx* ctx, int W, int H, int D, const float* vol, const float* levels, float* disp, float* conf);
/* mvs_ncc_volume_d + mvs_wta_d fused: the cost volume never reaches HBM.
 * disp/conf [H][W] are bit-identical to the two-pass result (levels from a->levels);
 * conf may be NULL. */
int mvs_ncc_wta_d(mvs_ctx* ctx, int W, int H, const uint8_t* l8, const int32_t* box, const mvs_array* a,
                  int K, int z, float* disp, float* conf);
/* mvs_ncc_wta_d for reference views [z0, z1) into disp/conf [z1 - z0][H][W]:
 * runs of views that share a sweep variant go in one launch (bit-identical to
 * one mvs_ncc_wta_d per view; clPhotoConsistency enqueues one sweep per
 * reference view, photo_consistency.cpp:133). */
int mvs_ncc_wta_range_d(mvs_ctx* ctx, int W, int H, const uint8_t* l8, const int32_t* box, const mvs_array* a,
                        int K, int z0, int z1, float* disp, float* conf);
/* Sub-level disparity (0.9): a three-point parabola fit through the costs of
 * the winning level and its two neighbours in level order.  All arithmetic is
 * float32, each operation rounded, no fused multiply-add.  For a pixel with
 * costs vol[0..D-1] and levels[0..D-1]:
 *   b    = first index of the minimum in level order, strict < (mvs_wta_d's rule)
 *   cm, c0, cp = vol[b-1], vol[b], vol[b+1]
 *   ok   = 0 < b < D-1 and cm < 2 and cp < 2   (a cost of 2: no valid window)
 *   den  = (cm - c0) + (cp - c0)               (> 0 whenever ok)
 *   off  = (0.5 * (cm - cp)) / den             (|off| <= 0.5; +0.5 iff cp == c0)
 *   step = off < 0 ? levels[b] - levels[b-1] : levels[b+1] - levels[b]
 *   disp_sub = ok ? levels[b] + off * step : levels[b]
 * mvs_wta_sub_d applies it to a materialised volume: disp_sub [H][W]; levels
 * (device pointer, [D]) need not be ordered. */
int mvs_wta_sub_d(mvs_ctx* ctx, int W, int H, int D, const float* vol, const float* levels, float* disp_sub);
/* The same for reference views [z0, z1) without a volume: disp [z1-z0][H][W] is
 * the integer-level winner mvs_ncc_wta_range_d wrote; disp_sub may be the same
 * buffer (in place).  The three costs are recomputed from the box planes:
 * bit-identical to mvs_ncc_volume_d + mvs_wta_sub_d per view.  The winner's
 * index is recovered from its level by value, so a->levels must be strictly
 * increasing (MVS_E_ARG otherwise, as for K other than 5 or 7 or a bad view
 * range); a disparity that matches no level is copied.  l8 is validated only. */
int mvs_ncc_sub_range_d(mvs_ctx* ctx, int W, int H, const uint8_t* l8, const int32_t* box, const mvs_array* a,
                        int K, int z0, int z1, const float* disp, float* disp_sub);
/* Semi-global aggregation of a cost volume along the four axis-aligned paths
 * (0.9.1).  vol, agg [D][H][W]; vol holds no NaN and no -0.0 (mvs_ncc_volume_d's
 * output holds neither); P1, P2 finite with 0 <= P1 <= P2.  All arithmetic is
 * float32, every operation rounded; there is no multiply, so nothing fuses.
 * A path r visits the pixels of one image row or column in order; q is the
 * pixel before p on it:
 *   first pixel of the path:  L_r(p, d) = vol[d][p]
 *   else:  m = min over k of L_r(q, k)
 *          t = min( L_r(q, d),
 *                   L_r(q, d-1) + P1   (d > 0 only),
 *                   L_r(q, d+1) + P1   (d < D-1 only),
 *                   m + P2 )
 *          L_r(p, d) = (vol[d][p] + t) - m
 * d-1 and d+1 are index neighbours: the spacing of the levels plays no part.
 * paths is a mask: bit 0 left->right (+x in each row), bit 1 right->left,
 * bit 2 top->bottom (+y in each column), bit 3 bottom->top.
 *   agg = ((L_b0 + L_b1) + L_b2) + L_b3
 * over the set bits, in bit order, rounded after each add; the first set path
 * is stored as it is (whatever agg held before is overwritten).
 * mvs_wta_d on agg gives the aggregated disparity and confidence.
 * mvs_wta_sub_d on agg is NOT defined: its ok rule reads a cost of 2 as "no
 * measurement", which does not carry over to sums; take the sub-level
 * disparity from the raw volume.  mvs_wta_agg_sub_d and mvs_wta_u16_sub_d
 * (below, 0.9.1.1.1.1.1) do that at the aggregate's winner.
 * MVS_E_ARG: a null pointer, bad W or H, D < 1 or D > 16384, paths outside
 * 1..15, a penalty that is not finite, negative, or P1 > P2, agg == vol (the
 * two must not overlap at all).  Nothing is allocated. */
int mvs_sgm_d(mvs_ctx* ctx, int W, int H, int D, const float* vol, float P1, float P2, int paths, float* agg);
/* The same with the four diagonal paths as well (0.9.1.1).  The recurrence, the
 * treatment of the levels that do not exist and the rounding are mvs_sgm_d's;
 * paths is a mask in 1..255, bits 0..3 as above and
 *   bit 4: a step of (dx, dy) = (+1, +1) per pixel, down-right
 *   bit 5: (-1, -1), up-left   (bit 4's lines walked the other way)
 *   bit 6: (-1, +1), down-left
 *   bit 7: (+1, -1), up-right  (bit 6's lines walked the other way)
 * A diagonal path visits (x0 + i dx, y0 + i dy), i = 0, 1, ..; its first pixel
 * is a pixel whose predecessor (x - dx, y - dy) lies outside the image, and
 * there L = vol.  There are W + H - 1 lines per direction, of 1 .. min(W, H)
 * pixels; with W == 1 or H == 1 every diagonal line is one pixel and L is vol.
 *   agg = ((((((L_b0 + L_b1) + L_b2) + L_b3) + L_b4) + L_b5) + L_b6) + L_b7
 * over the set bits, in bit order, rounded after each add; the first set path
 * is stored as it is.  For paths <= 15 the result is mvs_sgm_d's, bit for bit,
 * through the same launches.  MVS_E_ARG as mvs_sgm_d, with paths outside
 * 1..255.  Nothing is allocated.  mvs_sgm_d itself keeps refusing masks above
 * 15. */
int mvs_sgm8_d(mvs_ctx* ctx, int W, int H, int D, const float* vol, float P1, float P2, int paths, float* agg);
/* The same for N volumes of one shape in one call (0.9.1.1.1): one launch per
 * path over all of them, so N times the traffic is in flight.  Measured at
 * 1920x1080, D = 128, N = 5 (profiles/sgm_batch/ab.json): paths =
 * 255 takes 50.6 ms against 117.8 ms for five mvs_sgm8_d calls, paths = 15 33.2
 * against 57.0 ms; the vertical and diagonal paths gain (4.2x, 3.1x), the
 * horizontal ones do not.
 * Element i (0 <= i < N) is the volume [D][H][W] at vol + i * vol_stride, and
 * its aggregate goes to agg + i * agg_stride; the strides count floats.
 * Element i of agg is, bit for bit, what
 *   mvs_sgm8_d(ctx, W, H, D, vol + i * vol_stride, P1, P2, paths, agg + i * agg_stride)
 * writes: masks 1..255, the same sum order, the first set path stores, no
 * atomics.  Nothing between the elements of agg or behind the last one is
 * written; vol is not written.  The strides need be no multiple of 4 floats
 * (when vol and agg are not equally aligned mod 16 bytes in every element the
 * call takes the slower 4-byte form of the horizontal paths, as mvs_sgm_d
 * does for one volume).
 * Span rule: vol occupies [vol, vol + (N-1) * vol_stride + D*H*W) and agg
 * [agg, agg + (N-1) * agg_stride + D*H*W), gaps included; the two spans must
 * not overlap (they may abut), so layouts that interleave vol and agg elements
 * are refused.
 * MVS_E_ARG: everything mvs_sgm8_d refuses; N < 1 or N > 65535 (one grid
 * axis); a stride below D*H*W; overlapping spans.  Nothing is allocated. */
int mvs_sgm8_batch_d(mvs_ctx* ctx, int W, int H, int D, int N, const float* vol, size_t vol_stride, float P1, float P2,
                     int paths, float* agg, size_t agg_stride);
/* Semi-global aggregation on 16-bit integer costs (0.9.1.1.1.1): half the bytes
 * per cell and exact arithmetic.  Three calls: quantise a float32 cost volume,
 * aggregate N quantised volumes, take the winner of an aggregate.  Everything is
 * integer arithmetic except where it says otherwise.  tests/sgm16_ref.py is the
 * definition in numpy (int64); DESIGN.md 4e has the accuracy against the float32
 * aggregate, the kernels and the measured times. */
#define MVS_SGM16_SCALE 2047     /* units per unit of NCC cost */
#define MVS_SGM16_MAX_COST 4094  /* the largest quantised cost: 2 * 2047 */
#define MVS_SGM16_MAX_P 4095     /* the largest penalty */
/* 1. Quantise: for i < n
 *   dst[i] = (uint16) rint_to_even( min(max(src[i], 0), 2) * 2047.0f )
 * -- one rounded float32 multiply, then round-to-nearest-even.  src holds no NaN
 * (as for mvs_sgm_d).  The clamp matters: mvs_ncc_volume_d returns costs down to
 * about -0.005, and exactly 2 where there is no valid window.  n is any size
 * (0: nothing happens); src is 4-byte and dst 2-byte aligned, nothing more is
 * assumed; the two must not overlap.  MVS_E_ARG otherwise.  Nothing is
 * allocated. */
int mvs_quant_u16_d(mvs_ctx* ctx, size_t n, const float* src, uint16_t* dst);
/* 2. Aggregate N volumes vol [D][H][W] of uint16 into agg [D][H][W] of uint16.
 * The recurrence, the eight path bits, their directions, the first pixel of a
 * path (L = vol there) and the treatment of the levels that do not exist are
 * mvs_sgm8_d's, in integers:
 *   m = min over k of L(q, k)
 *   t = min( L(q, d), L(q, d-1) + P1 (d > 0), L(q, d+1) + P1 (d < D-1), m + P2 )
 *   L(p, d) = vol[d][p] + t - m
 * agg is the integer sum of L over the set bits of paths.  The sum is exact, so
 * its order plays no part.  Whatever agg held before is overwritten.
 * Preconditions: every vol element <= MVS_SGM16_MAX_COST (what mvs_quant_u16_d
 * writes obeys it), and 0 <= P1 <= P2 <= MVS_SGM16_MAX_P.  Then no 16-bit value
 * wraps: t <= m + P2, so L(p, d) <= vol[d][p] + P2 <= 4094 + 4095 = 8189, and
 * eight paths sum to at most 8 * 8189 = 65512 < 65536.  (L >= vol[d][p] >= 0 as
 * well: t >= m, since every member of the minimum is at least m.)  The kernels
 * cannot check the device data: with larger vol values the result is
 * unspecified, but every access stays inside vol and agg.
 * Batch rules, those of mvs_sgm8_batch_d with 2-byte elements: element i
 * (0 <= i < N) is the volume at vol + i * vol_stride, its aggregate goes to
 * agg + i * agg_stride, and the strides count uint16 elements; element i holds
 * bit for bit what N = 1 gives on it; nothing between the elements of agg or
 * behind the last one is written; vol is not written; 1 <= N <= 65535; vol
 * occupies [vol, vol + (N-1) * vol_stride + D*H*W) and agg likewise, gaps
 * included, and the two spans must not overlap (they may abut).  vol and agg
 * are 2-byte aligned; when they are not equal mod 16 bytes in every element
 * (the bases differ mod 16, or with N > 1 the strides differ by no multiple of
 * 8 elements) the horizontal paths take the slower 2-byte form.
 * MVS_E_ARG: everything mvs_sgm8_batch_d refuses, translated to 2-byte
 * elements; a pointer that is not 2-byte aligned; P1 < 0, P1 > P2 or P2 > 4095;
 * paths outside 1..255.  MVS_E_UNSUPPORTED: D > 256 (the workloads use 128 and
 * 256 levels; the kernel forms for more are left out on purpose).  Nothing is
 * allocated. */
int mvs_sgm8_u16_batch_d(mvs_ctx* ctx, int W, int H, int D, int N, const uint16_t* vol, size_t vol_stride, int P1,
                         int P2, int paths, uint16_t* agg, size_t agg_stride);
/* 3. Winner of a uint16 aggregate agg [D][H][W] (D >= 1, any D), per pixel:
 *   b    = the FIRST index of the minimum (integer ties are common)
 *   disp = levels[b]
 *   c2   = the minimum of agg[k] over |k - b| > 1
 *   conf = (float)(c2 - agg[b]) / 2047.0f  -- one correctly rounded float32
 *          divide; 0 when no such k exists (D <= 3 cases)
 * levels [D] and disp, conf [H][W] are float32 on the device; conf may be NULL.
 * MVS_E_ARG: a null pointer other than conf, bad W or H, D < 1, agg not 2-byte
 * aligned. */
int mvs_wta_u16_d(mvs_ctx* ctx, int W, int H, int D, const uint16_t* agg, const float* levels, float* disp,
                  float* conf);
/* Sub-level disparity of a semi-global aggregate (0.9.1.1.1.1.1): the winner is
 * the aggregate's, the parabola goes through the RAW costs of the same view at
 * that winner and its two index neighbours.  (A fit through the aggregated
 * costs is biased: the +P1 branch of the recurrence caps the aggregate beside
 * the winner, which flattens the parabola; DESIGN.md 4f has both measured.)
 * tests/sgm_sub_ref.py is the definition in numpy.  agg and raw (vol) are
 * [D][H][W] of one shape, levels [D] float32 on the device, need not be
 * ordered.  Per pixel, uint16 form (mvs_wta_u16_sub_d):
 *   b    = first index of the minimum of agg                 (mvs_wta_u16_d's rule)
 *   rm, r0, rp = raw[b-1], raw[b], raw[b+1]                   (integers)
 *   ok   = 0 < b < D-1  and  rm < 4094  and  rp < 4094        (MVS_SGM16_MAX_COST: no valid window)
 *          and  rm > r0  and  rp >= r0                        (raw has a minimum at b, mvs_wta_d's tie rule)
 *   den  = (rm - r0) + (rp - r0)                              (integer, 1 .. 8186 when ok)
 *   off  = (float)(rm - rp) / (float)(2 * den)                (one correctly rounded float32 divide;
 *                                                              |off| <= 0.5; +0.5 iff rp == r0)
 *   step = off < 0 ? levels[b] - levels[b-1] : levels[b+1] - levels[b]
 *   disp_sub = ok ? levels[b] + off * step : levels[b]        (product rounded, then the sum; no fused multiply-add)
 * float32 form (mvs_wta_agg_sub_d): b by mvs_wta_d's rule on agg; cm, c0, cp =
 * vol[b-1], vol[b], vol[b+1]; ok = 0 < b < D-1 and cm < 2 and cp < 2 and
 * cm > c0 and cp >= c0; from there mvs_wta_sub_d's arithmetic: den =
 * (cm - c0) + (cp - c0), off = (0.5 * (cm - cp)) / den, step and disp_sub as
 * above.  With agg and vol holding the same values the result is
 * mvs_wta_sub_d's, bit for bit.  agg and vol hold no NaN; where no agg cost is
 * below 1e6 (mvs_wta_d writes disp 0 and conf 0 there) disp_sub is 0.
 * Without "raw has a minimum at b" nothing would keep den above 0 at a winner
 * the aggregation moved; such a pixel keeps levels[b], as does one whose side
 * has no valid window (on those a fit through the aggregate measured no gain).
 * disp and conf may each be NULL; where given they hold bit for bit what
 * mvs_wta_d(agg) / mvs_wta_u16_d(agg) writes.  disp_sub is required.  agg is
 * read once.  agg and vol / raw are read only and may overlap or be one buffer;
 * the three outputs [H][W] must overlap neither each other nor an input.
 * MVS_E_ARG: a null pointer other than disp or conf, bad W or H, D < 1, a uint16
 * pointer that is not 2-byte aligned, overlapping outputs.  Any D.  Nothing is
 * allocated. */
int mvs_wta_agg_sub_d(mvs_ctx* ctx, int W, int H, int D, const float* agg, const float* vol, const float* levels,
                      float* disp, float* conf, float* disp_sub);
int mvs_wta_u16_sub_d(mvs_ctx* ctx, int W, int H, int D, const uint16_t* agg, const uint16_t* raw, const float* levels,
                      float* disp, float* conf, float* disp_sub);
/* Tuning / test hook: the NCC sweep variant this context tries first (0 =
 * automatic): waves per workgroup 4|8, levels per wave 1|2|4,
 * minimum LDS band width 64|80|96|128|192|256 columns, general_rows 1 = the kernel
 * that handles band rows starting on either row parity even when all start
 * on a pair.  Variants that do not fit the LDS fall back as in the default
 * chain.  mvs_ncc_last_variant reports the last launch as
 * {K, TH, levels per wave, waves, band width, row parity (0 mixed, 1 every band
 * row pair-aligned, 2 every pk row odd and stats row even), fused}: seven
 * int32 (the 0.5 report).  mvs_ncc_last_variant_n (0.7) writes the first
 * min(cap, 8) of those eight -- the eighth: band buffers (1 single-buffered,
 * 2 double-buffered) -- and returns 8, the slots it has. */
int mvs_set_ncc_variant(mvs_ctx* ctx, int waves, int levels_per_wave, int band_w, int general_rows);
int mvs_ncc_last_variant(mvs_ctx* ctx, int32_t* out7);
int mvs_ncc_last_variant_n(mvs_ctx* ctx, int32_t* out, int cap);
/* Test hook (0.8): the kernel form of the last mvs_sweep_spixl_d launch as
 * {FORM, LPS, WPS, TMODE, RELAID}: FORM 0 the general row-major gathers, 1 the
 * same-camera-row integer-shift (HZ) gathers, 2 the HZ form on LDS-staged rows,
 * 3 the gathers from re-laid (transposed / sheared) neighbour copies; LPS the
 * lanes per superpixel (32: two superpixels per wave, 64); WPS the waves per
 * superpixel; TMODE the transposition mode in effect (MVS_SWEEP_TRANSPOSE);
 * RELAID the number of (view, kind) copies built, 0 when none was needed or
 * the scratch could not be had.  Writes the first min(cap, 5) slots and
 * returns 5, the slots it has. */
int mvs_sweep_last_variant_n(mvs_ctx* ctx, int32_t* out, int cap);
/* Kernel timing (a measurement aid, no reference counterpart): with timing on,
 * every fused NCC sweep launch (mvs_ncc_wta_d / mvs_ncc_wta_range_d) records
 * start / stop events of its own dispatch (hipExtLaunchKernel), so the time is
 * the kernel's alone -- an event recorded on the stream before a call can fire
 * while the previous kernel is still running.  mvs_kernel_times waits for the
 * recorded launches and returns their times in ms (*n = how many were
 * recorded), then starts a new record; switching timing on also does.  When
 * more launches were recorded than cap it fails (MVS_E_ARG) with *n set and the
 * record kept, so the caller can retry with a buffer of *n. */
int mvs_set_kernel_timing(mvs_ctx* ctx, int on);
int mvs_kernel_times(mvs_ctx* ctx, float* ms, int cap, int* n);

/* Superpixel-plane refinement (clDepthRefinement, depth_refinement.cpp:91-1470).
 * flat [V][mh][mw][2] and state/state2 [V][mh][mw][6] are caller-provided
 * workspaces; the final state is returned in *state (compat: see mvs_refine_params). */
int mvs_flatness_d(mvs_ctx* ctx, int V, int mw, int mh, const float* spixl, float gamma, float* flat);
int mvs_init_state_d(mvs_ctx* ctx, int W, int H, int S, const float* spixl, const uint32_t* labels,
                     const uint8_t* rep, const float* flat, const mvs_array* a, float gamma, float alpha,
                     int kernel_steps, float kss, float fuse, float* state);
/* init_current_state for views [z0, z1) only (state rows of other views untouched). */
int mvs_init_state_range_d(mvs_ctx* ctx, int W, int H, int S, const float* spixl, const uint32_t* labels,
                           const uint8_t* rep, const float* flat, const mvs_array* a, float gamma, float alpha,
                           int kernel_steps, float kss, float fuse, int z0, int z1, float* state);
int mvs_propagate_d(mvs_ctx* ctx, int W, int H, int S, const float* spixl, const uint32_t* labels,
                    const uint8_t* rep, const float* flat, const mvs_array* a, int iter, float alpha,
                    float gamma, float fuse, int kernel_steps, float kss, const float* st_in, float* st_out,
                    int z0, int z1);
int mvs_spixl_to_image_d(mvs_ctx* ctx, int V, int W, int H, int S, const float* spixl, const uint32_t* labels,
                         const float* state, float* disp);
/* ABI 0.5: the same three passes over 16-bit label maps (uint16 [V][H][W], the
 * view-sharded pipeline's narrowed labels all-gather; requires
 * mw * mh <= 65536, else MVS_E_ARG).  Results are identical to the uint32
 * entry points on the same label values. */
int mvs_init_state_range_l16_d(mvs_ctx* ctx, int W, int H, int S, const float* spixl, const uint16_t* labels,
                               const uint8_t* rep, const float* flat, const mvs_array* a, float gamma, float alpha,
                               int kernel_steps, float kss, float fuse, int z0, int z1, float* state);
int mvs_propagate_l16_d(mvs_ctx* ctx, int W, int H, int S, const float* spixl, const uint16_t* labels,
                        const uint8_t* rep, const float* flat, const mvs_array* a, int iter, float alpha,
                        float gamma, float fuse, int kernel_steps, float kss, const float* st_in, float* st_out,
                        int z0, int z1);
int mvs_spixl_to_image_l16_d(mvs_ctx* ctx, int V, int W, int H, int S, const float* spixl, const uint16_t* labels,
                             const float* state, float* disp);
int mvs_refine_d(mvs_ctx* ctx, int W, int H, int S, const float* spixl, const uint32_t* labels,
                 const uint8_t* rep, const mvs_array* a, const mvs_refine_params* p, float* flat,
                 float* state, float* state2, float* disp);

/* Cross-view consistency filter (clcode.cl:1995-2101, pinned order):
 * project_to_reference_inv for all views, then remove_view_inconsistency for
 * reference views [z0, z1).  proj/out [V][H][W]. */
int mvs_filter_d(mvs_ctx* ctx, int V, int W, int H, int array_width, float bl_ratio, float fuse,
                 const float* disp_full, float* proj, float* out, int z0, int z1);
/* The filter's two passes separately, for view sharding: project_to_reference_inv
 * (clcode.cl:1995-2034) writes proj slices [z0, z1); remove_view_inconsistency
 * (clcode.cl:2037-2101) for references [z0, z1) reads EVERY proj slice, so a
 * shard all-gathers proj in between.  mvs_filter_d == proj_inv(0, V) +
 * remove_inconsistency(z0, z1). */
int mvs_proj_inv_d(mvs_ctx* ctx, int V, int W, int H, int array_width, float bl_ratio, const float* disp_full,
                   float* proj, int z0, int z1);
int mvs_remove_inconsistency_d(mvs_ctx* ctx, int V, int W, int H, int array_width, float bl_ratio, float fuse,
                               const float* disp_full, const float* proj, float* out, int z0, int z1);
/* The same two passes over image rows [y0, y1) only (0 <= y0 <= y1 <= H), for
 * a shard that pipelines the proj all-gather in row bands: the removal at a
 * pixel reads the proj slices at that pixel only (clcode.cl:2054-2056), so a
 * band's removal can start once that band's proj rows have arrived.  The
 * disparity stack is read in full by both (reprojected gathers).  proj_band
 * 0: proj is the full [V][H][W] stack; 1: proj is the band alone,
 * [V][y1 - y0][W] (what a row band's all-gather delivers; the projection
 * writes its block's rows straight into the band buffer).  ABI 0.4: proj_band
 * added to mvs_proj_inv_rows_d. */
int mvs_proj_inv_rows_d(mvs_ctx* ctx, int V, int W, int H, int array_width, float bl_ratio, const float* disp_full,
                        float* proj, int proj_band, int z0, int z1, int y0, int y1);
int mvs_remove_inconsistency_rows_d(mvs_ctx* ctx, int V, int W, int H, int array_width, float bl_ratio, float fuse,
                                    const float* disp_full, const float* proj, int proj_band, float* out, int z0,
                                    int z1, int y0, int y1);

/* ---- host-pointer stage API (mirrors the reference stage methods) ------- */
/* clSLIC::do_super_pixel_seg(in_img, lab_out, spixl_out, idx_out), one view. */
int mvs_do_super_pixel_seg(mvs_ctx* ctx, const uint8_t* rgbx, int W, int H, const mvs_slic_params* p,
                           float* lab, float* spixl, uint32_t* labels);
/* clPhotoConsistency::do_initial_depth_estimation(spixl_inout, rep_out, lab,
 * idx, array_width, bl_ratio, view_subset, disp_levels), all V views. */
int mvs_do_initial_depth_estimation(mvs_ctx* ctx, int W, int H, int S, float* spixl, uint8_t* rep,
                                    const float* lab, const uint32_t* labels, const mvs_array* a);
/* clDepthRefinement(...)->do_refinement(...) + fusion output disp [V][H][W]. */
int mvs_do_refinement(mvs_ctx* ctx, int W, int H, int S, const float* spixl, const uint32_t* labels,
                      const uint8_t* rep, const mvs_array* a, const mvs_refine_params* p, float* state_out,
                      float* disp);

/* project_to_reference_inv + remove_view_inconsistency over all V views
 * (clcode.cl:1995-2101; the reference's disabled call site
 * depth_refinement.cpp:1398-1451), host pointers [V][H][W]. */
int mvs_do_consistency_filter(mvs_ctx* ctx, int V, int W, int H, int array_width, float bl_ratio, float fuse,
                              const float* disp_full, float* out);

#ifdef __cplusplus
}
#endif
#endif /* MVS_H */
