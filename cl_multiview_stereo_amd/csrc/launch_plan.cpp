// The launch planners of launch_plan.h.  Host code only; built with
// -ffp-contract=off: the HZ and SAD tests compare the kernels' float products
// d * (float)dx and (bl * d) * (float)dy, and the SLIC normalisers are the
// reference's host float arithmetic.
#include "launch_plan.h"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdlib>
#include <cstring>

extern char** environ;

namespace mvs {
namespace plan {

Tuning plan_tuning() {
  Tuning t;
  // The launchers plan every step, and each getenv walks the whole
  // environment: one walk finds out whether any knob is set at all (they all
  // begin MVS_S or MVS_F), so the usual call costs less than the four to six
  // lookups a launcher used to make.
  bool any = false;
  for (char** e = environ; e && *e && !any; e++) {
    const char* s = *e;  // compared in line: a library call per entry costs more than the lookups saved
    any = s[0] == 'M' && s[1] == 'V' && s[2] == 'S' && s[3] == '_' && (s[4] == 'S' || s[4] == 'F');
  }
  if (!any) return t;
  const auto num = [](const char* name, int dflt) {
    const char* e = getenv(name);
    return e ? atoi(e) : dflt;
  };
  const auto is = [](const char* name, const char* value) {
    const char* e = getenv(name);
    return e && !strcmp(e, value);
  };
  const int wps = num("MVS_SWEEP_WPS", 0);
  t.sweep_wps = (wps == 1 || wps == 2 || wps == 4) ? wps : 0;
  t.sweep_transpose = num("MVS_SWEEP_TRANSPOSE", 2);
  t.sweep_hz = num("MVS_SWEEP_HZ", 1) != 0;
  t.sweep_ring = num("MVS_SWEEP_RING", 1) != 0;
  t.sweep_ring_fast = num("MVS_SWEEP_RING_FAST", 1) != 0;
  if (const char* kv = getenv("MVS_SAD_KERNEL")) {
    t.sad_kernel = kv;
    t.sad_named = true;
  }
  t.sad_aff = getenv("MVS_SAD_AFF") == nullptr;
  t.filter_px = is("MVS_FILTER_KERNEL", "px");
  t.filter_fb_q = num("MVS_FILTER_FB", 2);
  t.filter_fb_px = num("MVS_FILTER_FB", 4);
  t.filter_ns = num("MVS_FILTER_NS", 2);
  t.filter_bound = num("MVS_FILTER_BOUND", 1) != 0;
  t.filter_ref_order = is("MVS_FILTER_ORDER", "ref");
  t.slic_tiles9 = num("MVS_SLIC_TILES9", 0) == 1;
  t.slic_update_walk = num("MVS_SLIC_UPDATE", 1) != 0;
  return t;
}

SlicPlan plan_slic(const Tuning& t, int V, int W, int H, int S, int no_iter, int edge_enable, int search,
                   int enforce_connectivity) {
  SlicPlan p;
  p.V = V, p.W = W, p.H = H, p.S = S;
  const int mw = p.mw = map_dim(W, S), mh = p.mh = map_dim(H, S);
  // clSLIC ctor, clSLIC.cpp:15-18 (host float arithmetic)
  float xy = 1.0f / (1.4242f * (float)S);
  float col = 15.0f / (1.7321f * 128.0f);
  p.xy = xy * xy;
  p.col = col * col;
  const bool tiles = S % kLocal == 0;
  const int cpl = p.cpl = S * 3 / kLocal;
  // (the two agree where both apply; each path keeps the reference's formula it was written with)
  const int G = p.G = tiles ? cpl * cpl : (int)__builtin_ceilf((float)(S * S * 9) / (float)(kLocal * kLocal));
  const int ntx = p.ntx = (W + 15) / 16, nty = p.nty = (H + 15) / 16;
  const size_t P = (size_t)V * W * H;
  const bool l16 = !tiles && no_iter > 0 && (long)mw * mh <= 65536;
  size_t sb = tiles ? sizeof(float) * 6 * (size_t)G * mw * mh * V : 0;
  if (enforce_connectivity || edge_enable) sb = std::max(sb, sizeof(uint32_t) * P);
  if (l16) sb = std::max(sb, sizeof(uint16_t) * P);
  p.scratch_bytes = sb;

  p.steps.reserve(6 + 2 * (size_t)no_iter);
  const auto step = [&p](SlicKernel k, unsigned gx, unsigned gy, unsigned gz, unsigned block) -> SlicStep& {
    p.steps.push_back(SlicStep{k, 0, 0, 0, 0, 0, {gx, gy, gz}, block, false, false, false, false});
    return p.steps.back();
  };
  const unsigned cx = (mw + 63) / 64, px = (W + 255) / 256;
  step(kSlicInitCenters, cx, mh, V, 64);
  if (edge_enable == 1 || edge_enable == 2) {  // clSLIC::apply_edge_values (clSLIC.cpp:186-233)
    step(kSlicEdge, px, H, V, 256);
    // 1, the reference's path: the magnitude into the Lab image;
    // apply_edge_alternative then reads the never-written edge_img (pinned as
    // zeros): no centre moves
    if (edge_enable == 1)
      step(kSlicEdgeStore, (unsigned)std::min<long>(((long)P + 255) / 256, 8192), 1, 1, 256);
    else
      step(kSlicApplyEdge, cx, mh, V, 64);
  }
  // k_assign_tiles4: the 2x2 loop at S = 32 or 64, 32-bit byte offsets into a view and into part
  const bool tiles4 = !search && (S == 32 || S == 64) && (long)W * H * 16 < (1L << 31) &&
                      (long)mw * mh * G * 24 < (1L << 31) && !t.slic_tiles9;
  // more: an update follows this assignment
  const auto assign = [&](bool more) {
    if (tiles) {
      SlicStep& s = tiles4 ? step(kSlicAssignTiles4, (ntx + 3) / 4, nty, V, 256)
                           : step(kSlicAssignTiles9, (ntx * nty + 3) / 4, V, 1, 256);
      if (tiles4)
        s.S16 = S / 16;
      else
        s.S3 = search;
      s.labels = !more, s.part = more;
    } else {
      SlicStep& s = step(kSlicAssign, (W + kAssignTW - 1) / kAssignTW, (H + kAssignTH - 1) / kAssignTH, V, 256);
      s.S3 = search;
      s.labels = !(more && l16), s.lb16 = more && l16;
    }
  };
  // k_update_walk's 32-bit byte offsets span a view's Lab: W H 16 < 2^31
  const bool walk = (long)W * H * 16 < (1L << 31) && t.slic_update_walk;
  assign(no_iter > 0);
  for (int i = 0; i < no_iter; i++) {
    if (tiles) {
      step(kSlicUpdateFinalize, (mw * mh + 31) / 32, V, 1, 256).CPL = cpl == 6 ? 6 : 0;
    } else {
      SlicStep& s = step(walk ? kSlicUpdateWalk : kSlicUpdate, (mw * mh + 3) / 4, V, 1, 256);
      s.UT = G > 4 ? 4 : 1;
      s.LT = l16 ? 16 : 32;
    }
    assign(i + 1 < no_iter);
  }
  if (enforce_connectivity) {
    step(kSlicSuppress, px, H, V, 256).to_scratch = true;
    step(kSlicSuppress, px, H, V, 256);
  }
  return p;
}

SpixlSweepPlan plan_sweep_spixl(const Tuning& t, int V, int W, int H, int S, int D, const float* levels,
                                const int* vs, const int* sn, int aw, int z0, int z1, bool allow_relayout) {
  SpixlSweepPlan p;
  if (z1 <= z0) return p;
  // k_sweep_spixl's 32-bit byte offsets within a view (a re-laid one spans
  // at most (W + H) H elements; a row-major one, W H, is covered by the same test)
  if ((long)(W + H) * H * 16 >= (1L << 31)) {
    p.err = "superpixel sweep: image too large for 32-bit offsets";
    return p;
  }
  p.launch = true;
  p.mw = map_dim(W, S);
  p.mh = map_dim(H, S);
  const long M = (long)p.mw * p.mh;
  const bool half = D <= 32;  // two superpixels per wave
  int wps = (D + 63) / 64;
  wps = wps >= 3 ? 4 : wps;  // waves per superpixel: 1, 2 or 4
  const int wps_env = half ? 0 : t.sweep_wps;
  if (wps_env) wps = wps_env;
  // the vertical and diagonal neighbours of the references, re-laid into the
  // context scratch.  Slot offsets are in units of H elements (tstride = H): a
  // transposed slot takes W units, a sheared one W + H - 1.
  const int tmode = t.sweep_transpose;
  p.tstride = H;
  if (tmode > 0 && allow_relayout) {
    std::vector<int32_t> slot(4 * (size_t)V, -1);
    long units = 0;
    for (int z = z0; z < z1; z++)
      for (int k = 0; k < sn[z]; k++) {
        const int v = vs[(size_t)V * z + k];
        if (v < 0 || v >= V) continue;
        const int dx = v % aw - z % aw, dy = v / aw - z / aw;
        const int kind = dx == 0 ? 1 : tmode < 2 ? 0 : dx == dy ? 2 : dx == -dy ? 3 : 0;
        if (kind && slot[4 * v + kind] < 0 && units + W + H <= INT32_MAX) {
          slot[4 * v + kind] = (int32_t)units;
          units += kind == 1 ? W : W + H - 1;
        }
      }
    if (units > 0) {
      for (int v = 0; v < V; v++)
        for (int kind = 1; kind < 4; kind++)
          if (slot[4 * v + kind] >= 0) p.relayouts.push_back({v, kind, slot[4 * v + kind]});
      p.slot = std::move(slot);
      p.units = units;
    }
  }
  const bool relaid = p.units > 0;
  // HZ: every neighbour of [z0, z1) in the reference's camera row and every
  // level x column offset an integer of magnitude below 2^24
  bool hz = !relaid && t.sweep_hz;
  for (int z = z0; z < z1 && hz; z++)
    for (int k = 0; k < sn[z] && hz; k++) {
      const int v = vs[(size_t)V * z + k];
      if (v / aw != z / aw) hz = false;
      const float fdxv = (float)(v % aw - z % aw);
      for (int l = 0; l < D && hz; l++) {
        const float f = levels[l] * fdxv;  // the kernel's d * (float)(vx - rx)
        if (!(fabsf(f) < 16777216.0f) || f != truncf(f)) hz = false;
      }
    }
  // HZ with 64 levels per wave: the LDS-staged rows
  bool ring = hz && !half && t.sweep_ring;
  if (ring) {  // every staged window fits kSwU columns (see k_sweep_spixl_ring)
    float rng = 0.0f;
    for (int c0 = 0; c0 < D; c0 += 64) {
      float lo = levels[c0], hi = lo;
      for (int l = c0; l < std::min(D, c0 + 64); l++) {
        lo = std::min(lo, levels[l]);
        hi = std::max(hi, levels[l]);
      }
      rng = std::max(rng, hi - lo);
    }
    int mdx = 0;
    for (int z = z0; z < z1; z++)
      for (int k = 0; k < sn[z]; k++) mdx = std::max(mdx, std::abs(vs[(size_t)V * z + k] % aw - z % aw));
    if (2.0 * (S - 1) + 2.0 + (double)rng * mdx + 1.0 > (double)kSwU) ring = false;
  }
  p.form = ring ? kSweepHzRing : relaid ? kSweepRelaid : hz ? kSweepHzGather : kSweepGeneral;
  p.lps = half ? 32 : 64;
  // ring: one wave per superpixel, its 64-level passes in turn: the ring form's
  // cost is per staged row and level, not per wave, and four superpixels per
  // workgroup share its setup and tail (C5, D = 256: 1.19 ms per launch
  // against 1.42 with four waves per superpixel; C2 alike at 1 and 2:
  // profiles/r06/sweep_ring_waves.txt)
  p.wps = ring ? (wps_env ? wps_env : 1) : wps;
  const int spb = half ? 8 : 4 / p.wps;  // superpixels per workgroup
  const long nb = (M + spb - 1) / spb;
  p.grid_x = (unsigned)(8 * ((nb + 7) / 8));
  p.grid_y = (unsigned)(z1 - z0);
  const int last[5] = {p.form, p.lps, p.wps, tmode, (int)p.relayouts.size()};
  std::copy(last, last + 5, p.last);
  return p;
}

bool sad_band_geometry(int DC, int RR, bool aff, int V, int W, int H, int D, const float* levels, const int* vs,
                       const int* sn, int aw, float bl, int z, SadPlan& p) {
  const int TH = RR - 4, PPW = DC / 8;
  const int nn = sn[z];
  const int nch = (D + DC - 1) / DC;
  const int rx = z % aw, ry = z / aw;
  constexpr int RW = sizeof(SadRec) / 4;
  std::vector<int32_t> table((size_t)std::max(1, nch * nn) * RW, 0);
  int span_x = 0;
  float span_y = 0.0f;
  for (int c = 0; c < nch; c++)
    for (int n = 0; n < nn; n++) {
      SadRec e{};
      const int view = vs[V * z + n];
      const int dx = view % aw - rx, dy = view / aw - ry;
      e.view = view;
      e.sxmin = 1 << 30;
      e.sxmax = -(1 << 30);
      e.fdymin = INFINITY;
      e.fdymax = -INFINITY;
      for (int j = 0; j < DC; j++) {
        const int dl = std::min(c * DC + j, D - 1);  // past the end: the last level (rows masked)
        const float d = levels[dl];
        const float fdx = d * (float)dx;  // the reference's float shifts (clcode.cl:1033-1034)
        const float fdy = (bl * d) * (float)dy;
        if (fdx != std::trunc(fdx) || std::fabs(fdx) > 1e6f) return false;
        e.sx[j] = (int)fdx;
        e.fdy[j] = fdy;
        if (fdy != std::trunc(fdy) || std::fabs(fdy) > 1e6f) aff = false;
        if (c * DC + j < D) {
          e.sxmin = std::min(e.sxmin, e.sx[j]);
          e.sxmax = std::max(e.sxmax, e.sx[j]);
          e.fdymin = std::min(e.fdymin, fdy);
          e.fdymax = std::max(e.fdymax, fdy);
        }
      }
      span_x = std::max(span_x, e.sxmax - e.sxmin);
      span_y = std::max(span_y, e.fdymax - e.fdymin);
      std::memcpy(table.data() + ((size_t)c * nn + n) * RW, &e, sizeof(SadRec));
    }
  SadArgs a{};
  a.W = W; a.H = H; a.D = D; a.nn = nn; a.z = z; a.nch = nch;
  a.bw = (64 + span_x + 63) & ~63;  // whole 64-pixel LDS-DMA pieces per band row
  // a step's band spans at most RR + ceil(span_y) rows (sad_band_of: the
  // truncated ends differ by < RR + span_y); one spare row for the float
  // rounding of fractional shifts, none when every shift is integral
  a.brows = RR + (int)std::ceil(span_y) + (aff ? 0 : 1);
  const size_t lds = 16 * 2 * (size_t)a.brows * a.bw + (aff ? 0 : 4 * 2 * (size_t)DC * RR);
  // band columns: SB_NBLK pieces of 64 at most (the systolic tile's reach)
  if (a.bw > 64 * SB_NBLK) return false;
  if (lds > 160 * 1024 || (size_t)4 * TH * 64 * 8 > 16 * 2 * (size_t)a.brows * a.bw) return false;
  a.tiles_x = (W + SB_TW - 1) / SB_TW;
  a.ntiles = a.tiles_x * ((H + TH - 1) / TH);
  a.tiles_per_xcd = (a.ntiles + 7) / 8;
  p.band = true;
  p.TH = TH;
  p.PPW = PPW;
  p.AFF = aff;
  p.BWT = aff ? (a.bw == 64 ? 64 : 128) : 0;
  p.table = std::move(table);
  p.args = a;
  p.lds = lds;
  p.grid_x = 8 * a.tiles_per_xcd;
  p.grid_y = 1;
  return true;
}

SadPlan plan_sad(const Tuning& t, int V, int W, int H, int D, const float* levels, const int* vs, const int* sn,
                 int aw, float bl, int z) {
  SadPlan p;
  const std::string& kind = t.sad_kernel;
  // the band forms tried, in order: (TH, PPW) = (8, 2), then (8, 1)
  const bool try2 = kind == "auto" || kind == "sys8x2", try1 = kind == "auto" || kind == "sys8";
  if (try2 && sad_band_geometry(16, 12, t.sad_aff, V, W, H, D, levels, vs, sn, aw, bl, z, p)) return p;
  if (try1 && sad_band_geometry(8, 12, t.sad_aff, V, W, H, D, levels, vs, sn, aw, bl, z, p)) return p;
  if (t.sad_named && kind != "gather") {
    p.err = "k_sad_band variant " + kind + " cannot stage this geometry (MVS_SAD_KERNEL set explicitly)";
    return p;
  }
  p.grid_x = (W + PT - 1) / PT;
  p.grid_y = (H + PT - 1) / PT;
  return p;
}

FilterPlan plan_remove_incons(const Tuning& t, int V, int W, int H, int aw, int z0, int z1, int ya, int yb,
                              bool band) {
  FilterPlan p;
  const int NR = yb - ya;  // rows [ya, yb) only (the caller checks 0 <= ya <= yb <= H)
  // band: proj holds rows [ya, yb) only, as [V][yb - ya][W] (the kernels index
  // proj[PP * view + y * W + x], so the band's base moves up by ya rows)
  p.PP = band ? (long)NR * W : (long)W * H;
  p.proj_off = band ? -(long)ya * W : 0;
  if (z1 <= z0 || NR <= 0) return p;
  const unsigned gx = (W + 255) / 256;
  const auto grid = [&p](unsigned x, unsigned y, unsigned z) { p.grid[0] = x, p.grid[1] = y, p.grid[2] = z; };
  // few views: one thread per (reference, pixel) keeps more threads in flight
  // (measured at V = 5: 350 vs 395 us); many views: one thread per pixel
  const bool off32 = (long)V * W * H * 4 < (1L << 31);  // 32-bit gather offsets (the sel / q kernels)
  if (V <= 8 && off32) {
    p.kernel = kFilterSel8;
    grid(gx, NR, z1 - z0);
  } else if (V <= 16) {
    p.kernel = kFilterPx16_8;
    grid(gx, NR, 1);
  } else if (V <= 32 && off32 && !t.filter_px) {
    // 32-bit gather offsets: one work queue per lane (k_remove_incons_q,
    // MVS_FILTER_NS candidates at once, MVS_FILTER_FB views per gather block);
    // MVS_FILTER_KERNEL=px: the per-pixel form below.
    // Measured at C4, all 32 references with k_proj_inv
    // (scripts/bench_filter.py): q 18.1 ms (NS 2, FB 2); the lane-balanced
    // hand-out of (pixel, candidate) items 21.1 ms and the lock-step walk
    // 27.9 ms (both removed in round 3).
    p.kernel = kFilterQ;
    p.FB = t.filter_fb_q == 4 ? 4 : 2;
    p.NS = t.filter_ns == 1 ? 1 : 2;
    p.ROWB = aw % p.FB == 0;
    p.RM = !t.filter_ref_order;
    p.inb = (V % aw == 0 && t.filter_bound) ? 1 : 0;
    const unsigned tx = (W + 63) / 64, groups = (z1 - z0 + kFilterRG - 1) / kFilterRG;
    if (p.RM)
      grid(tx * groups, NR, 1);
    else
      grid(tx, NR, groups);
    p.block = 64 * kFilterRG;
  } else if (V <= 32) {
    // MVS_FILTER_FB: views per gather block.  Measured at C4
    // (scripts/bench_filter.py): blocks of 8 gathers 54 ms for all 32
    // references, 4: 35 ms, 2: 35 ms -- a candidate's early exit comes after
    // ~3 gathers, so 8-wide blocks fetched twice what the vote needed
    p.kernel = kFilterPx32;
    p.FB = t.filter_fb_px == 4 ? 4 : t.filter_fb_px == 2 ? 2 : 8;
    grid(gx, NR, 1);
  } else if (V <= 64 && off32) {
    p.kernel = kFilterSel64;
    grid(gx, NR, z1 - z0);
  } else {
    p.kernel = kFilterPlain;
    grid(gx, NR, z1 - z0);
  }
  return p;
}

SgmPlan plan_sgm(int W, int H, int D, int path) {
  SgmPlan p;
  if (W < 1 || H < 1 || D < 1 || path < 0 || path > 3) {
    p.err = "sgm: bad dimensions or path";
    return p;
  }
  if (D > kSgmMaxD) {
    p.err = "sgm: more than 16384 levels";
    return p;
  }
  const bool vertical = path >= 2;
  p.rev = path & 1;
  p.n = vertical ? H : W;
  p.lines = vertical ? W : H;
  if (vertical && D <= kSgmColumnsMaxD) {
    p.form = kSgmColumns;
    p.lpl = kSgmColumnsLpw;
    p.waves = (D + kSgmColumnsLpw - 1) / kSgmColumnsLpw;
    p.sstride = W;
    p.lstride = 1;
    p.grid = (unsigned)((W + 63) / 64);
    // two buffers of {minimum, first, last} per wave and column; the kernel is built for 8 or 16 waves
    p.lds = sizeof(float) * 2 * (p.waves <= 8 ? 8 : 16) * 3 * 64;
  } else {
    p.form = kSgmLanes;
    p.sstride = vertical ? W : 1;
    p.lstride = vertical ? 1 : W;
    p.vec = !vertical;
    if (D <= kSgmLanesOneWave) {
      p.lpl = 1;
      while (64 * p.lpl < D) p.lpl *= 2;
      p.waves = 1;
    } else {  // (the multi-wave kernel is held to 128 registers: no 16-byte pieces)
      p.lpl = kSgmMaxLpl;
      p.waves = (D + kSgmLanesOneWave - 1) / kSgmLanesOneWave;
      p.vec = false;
      p.lds = sizeof(float) * 2 * 16 * 3;  // two buffers of {minimum, first, last} per wave
    }
    p.grid = (unsigned)p.lines;
  }
  p.block = 64u * (unsigned)p.waves;
  return p;
}

SgmPlan plan_sgm_diag(int W, int H, int D, int path) {
  SgmPlan p;
  if (W < 1 || H < 1 || D < 1 || path < 4 || path > 7) {
    p.err = "sgm: bad dimensions or path";
    return p;
  }
  if (D > kSgmMaxD) {
    p.err = "sgm: more than 16384 levels";
    return p;
  }
  p.sx = path < 6 ? 1 : -1;
  p.rev = path & 1;
  p.lines = W + H - 1;
  p.n = W, p.lstride = H;  // (what k_sgm_lanes at DIAG takes in these places)
  p.sstride = W + p.sx;
  if (D <= kSgmColumnsMaxD) {
    p.form = kSgmSheared;
    p.lpl = kSgmColumnsLpw;
    p.waves = (D + kSgmColumnsLpw - 1) / kSgmColumnsLpw;
    p.grid = (unsigned)((p.lines + 63) / 64);
    p.lds = sizeof(float) * 2 * (p.waves <= 8 ? 8 : 16) * 3 * 64;  // as the columns form
  } else {
    p.form = kSgmLanes;
    if (D <= kSgmLanesOneWave) {
      p.lpl = D <= 64 * 8 ? 8 : kSgmMaxLpl;  // (D > 256 here: 8 or 16 levels per lane)
    } else {
      p.lpl = kSgmMaxLpl;
      p.waves = (D + kSgmLanesOneWave - 1) / kSgmLanesOneWave;
      p.lds = sizeof(float) * 2 * 16 * 3;
    }
    p.grid = (unsigned)p.lines;
  }
  p.block = 64u * (unsigned)p.waves;
  return p;
}

SgmBatchPlan plan_sgm_batch(SgmCost cost, int W, int H, int D, int N, uintptr_t vol_addr, size_t vol_stride,
                            uintptr_t agg_addr, size_t agg_stride) {
  SgmBatchPlan p;
  const unsigned esize = 16u / (unsigned)cost.piece;
  if (W < 1 || H < 1 || D < 1 || (long)W * H > (1L << 27)) {
    p.err = "bad dimensions";
    return p;
  }
  if (D > cost.max_d) {
    p.err = cost.unsupported ? "more than 256 levels: the 16-bit forms are not built for them" : "bad dimensions";
    p.unsupported = cost.unsupported;
    return p;
  }
  if (N < 1 || N > kSgmMaxBatch) {
    p.err = "N must be in 1..65535";
    return p;
  }
  if (esize == 2 && ((vol_addr | agg_addr) & 1)) {
    p.err = "a pointer that is not 2-byte aligned";
    return p;
  }
  const size_t dhw = (size_t)D * (size_t)H * (size_t)W;  // <= 2^41
  if (vol_stride < dhw || agg_stride < dhw) {
    p.err = "a stride below D*H*W";
    return p;
  }
  // the spans in bytes; 128 bits: a stride is any size_t
  typedef unsigned __int128 u128;
  const u128 v0 = vol_addr, v1 = v0 + esize * ((u128)(N - 1) * vol_stride + dhw);
  const u128 a0 = agg_addr, a1 = a0 + esize * ((u128)(N - 1) * agg_stride + dhw);
  if (v0 < a1 && a0 < v1) {
    p.err = "the vol and agg spans overlap";
    return p;
  }
  p.grid_y = (unsigned)N;
  p.vec_ok = sgm_piece_vec_ok(cost.piece, N, vol_addr, vol_stride, agg_addr, agg_stride);
  return p;
}

}  // namespace plan
}  // namespace mvs
