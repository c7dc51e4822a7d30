// The NCC sweep's launch planner (see ncc_plan.h).  Built with
// -ffp-contract=off like the rest of the library: the shifts
// (roundf(d * dx), roundf((bl * d) * dy)) are the definition's (ncc.hip).
#include "ncc_plan.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>

namespace mvs {
namespace ncc {
namespace {

int env_int(const char* name, int unset) {
  const char* e = getenv(name);
  return e ? atoi(e) : unset;
}

constexpr size_t kLdsCu = (size_t)160 * 1024;   // a CU's LDS: one workgroup
constexpr size_t kLdsTwo = (size_t)80 * 1024;   // two workgroups per CU

}  // namespace

NccTuning ncc_tuning(int force_nw, int force_dpw, int force_bw, int force_general) {
  static const int dpw_env = env_int("MVS_NCC_DPW", 4);
  static const int nw_env = env_int("MVS_NCC_NW", 8);
  NccTuning t;
  t.dpw = dpw_env;
  t.nw = nw_env;
  t.nb = env_int("MVS_NCC_NB", 0);
  t.mfma = env_int("MVS_NCC_MFMA", 1);
  t.mfma_v = env_int("MVS_NCC_MFMA_V", 1);
  t.mfma7 = env_int("MVS_NCC_MFMA7", 1);
  t.mfma_dbg = env_int("MVS_NCC_MFMA_DBG", 0);
  t.run = std::max(1, std::min(kMaxRef, env_int("MVS_NCC_RUN", kMaxRef)));
  t.plane32 = env_int("MVS_NCC_PLANE32", 1);
  t.force_nw = force_nw;
  t.force_dpw = force_dpw;
  t.force_bw = force_bw;
  t.force_general = force_general;
  return t;
}

size_t scalar_lds_bytes(int nb, int pairs, int pitch, int nw, bool fuse) {
  const size_t bands = (size_t)nb * 16 * pairs * pitch;
  if (!fuse) return bands;
  return std::max(bands, (size_t)3 * 4 * nw * kTileH * 64) + 4 * kTileH * 64;  // WTA partials; + s_r [64][TH]
}

size_t mfma_lds_bytes(int pitch, int nb, int pairs, int tmax, int dc) {
  return std::max((size_t)nb * 16 * pairs * (pitch + 1), (size_t)3 * 16 * kMfMergeStride * 4) + 2 * 64 * kTileH * 4 +
         (size_t)tmax * dc * 2;
}

// A vertical-only list needs 64, a diagonal or horizontal neighbour 64 + the
// chunk's shift range (C4: 71 / 79 / 95)
int scalar_pitch(int band_w) {
  return band_w <= 64 ? 64 : band_w <= 80 ? 80 : band_w <= 96 ? 96 : band_w <= 128 ? 128 : band_w <= 192 ? 192 : 256;
}

// VERT (K = 5 only): 80 | 96 | 128, the tail kernels one pitch; horizontal
// lists (K = 5 and 7 alike): 128 | 192, the tail kernels 192
int mfma_pitch(bool vert, bool tail, int K, int band_w) {
  (void)K;
  if (vert) return tail ? 128 : band_w <= 80 ? 80 : band_w <= 96 ? 96 : 128;
  return tail || band_w > 128 ? 192 : 128;
}

namespace {

// ---- shift geometry of one reference view's list, in chunks of dc levels ----
// Per (chunk c, neighbour n): the shift extents of the chunk's levels and the
// row-pair bands covering them.  The pk band's first image row is
// y0 - R - tymax, the stats band's y0 - tymax; y0 is even (TH even), so their
// parities pr, sr in the pair band are independent of y0.
struct ChunkGeom {
  int txmin, txmax, tymin, tymax;
  int pr, sr;    // parity of the pk / stats band's first row
  int bhp, shp;  // pk / stats pair rows covering every level's rows
};
struct SweepGeom {
  int nch = 0, nn = 0, dc = 0;
  std::vector<int> tx, ty;     // [D][nn] shifts
  std::vector<ChunkGeom> ch;   // [nch][nn]
  int band_w = 64;             // columns per pair row: 64 + the widest chunk span (stage() never writes past them)
  int pk_pairs = 0, st_pairs = 0;  // the tallest step's bands
  const ChunkGeom& at(int c, int n) const { return ch[(size_t)c * nn + n]; }
};

SweepGeom chunk_geometry(int K, int dc, const float* levels, int D, int nn, const float* fdx, const float* fdy,
                         float bl) {
  const int R = K / 2, NR = kTileH + 2 * R;
  SweepGeom g;
  g.nch = (D + dc - 1) / dc;
  g.nn = nn;
  g.dc = dc;
  g.tx.resize((size_t)D * nn);
  g.ty.resize((size_t)D * nn);
  for (int dl = 0; dl < D; dl++)
    for (int n = 0; n < nn; n++) {
      g.tx[(size_t)dl * nn + n] = (int)roundf(levels[dl] * fdx[n]);
      g.ty[(size_t)dl * nn + n] = (int)roundf((bl * levels[dl]) * fdy[n]);
    }
  g.ch.resize((size_t)g.nch * nn);
  int spx = 0;
  for (int c = 0; c < g.nch; c++)
    for (int n = 0; n < nn; n++) {
      ChunkGeom& e = g.ch[(size_t)c * nn + n];
      e.txmin = e.tymin = 1 << 30;
      e.txmax = e.tymax = -(1 << 30);
      for (int dl = c * dc; dl < std::min(D, c * dc + dc); dl++) {
        const int tx = g.tx[(size_t)dl * nn + n], ty = g.ty[(size_t)dl * nn + n];
        e.txmin = std::min(e.txmin, tx);
        e.txmax = std::max(e.txmax, tx);
        e.tymin = std::min(e.tymin, ty);
        e.tymax = std::max(e.tymax, ty);
      }
      e.pr = (R + e.tymax) & 1;
      e.sr = e.tymax & 1;
      e.bhp = (e.pr + NR + e.tymax - e.tymin + 1) >> 1;
      e.shp = (e.sr + kTileH + e.tymax - e.tymin + 1) >> 1;
      spx = std::max(spx, e.txmax - e.txmin);
      g.pk_pairs = std::max(g.pk_pairs, e.bhp);
      g.st_pairs = std::max(g.st_pairs, e.shp);
    }
  g.band_w = 64 + spx;
  return g;
}

// One reference view's choice: its form, its shift table and what a run
// needs to know to merge it.
struct ViewPlan {
  bool mfma = false, vert = false;
  int dpw = 0, nw = 0;  // scalar: levels per wave, waves
  int ndb = 0;          // matrix-core: 16-level blocks per chunk
  int nb = 2;           // band buffers
  int width = 0;        // scalar: the pitch template; matrix-core: the band's columns
  int pk_pairs = 0, st_pairs = 0;
  int par = kParMixed;  // (scalar)
  int steps = 0;        // (matrix-core) chunks x neighbours
  size_t cap = 0;       // the LDS bytes its bands were fitted to
  std::vector<int32_t> table;
};

// ---- the scalar kernels' table: NccRec [nchunks][nn][NW waves] as int32 ----
ViewPlan make_plan(int K, int dpw, int nw, const float* levels, int D, int nn, const float* fdx, const float* fdy,
                   float bl) {
  const SweepGeom g = chunk_geometry(K, nw * dpw, levels, D, nn, fdx, fdy, bl);
  ViewPlan p;
  p.dpw = dpw;
  p.nw = nw;
  p.width = g.band_w;
  p.pk_pairs = g.pk_pairs;
  p.st_pairs = g.st_pairs;
  p.table.assign((size_t)g.nch * nn * nw * kRecWords, 0);
  bool even = true;  // every level's band rows start on a pair boundary (kParEven)
  bool odd = true;   // every pk start odd, every stats start even (kParOdd)
  for (int c = 0; c < g.nch; c++)
    for (int n = 0; n < nn; n++) {
      const ChunkGeom& q = g.at(c, n);
      for (int w = 0; w < nw; w++) {
        int32_t* e = p.table.data() + (((size_t)c * nn + n) * nw + w) * kRecWords;
        e[0] = q.txmax;
        e[1] = q.tymax;
        e[2] = q.bhp;
        e[3] = q.shp | ((q.txmax - q.txmin) << 16);  // stage(): pieces of 64 columns covering 64 + span
        for (int j = 0; j < dpw; j++) {
          const int dl = c * g.dc + w + nw * j;
          if (dl >= D) {  // dummy level past the end: the band origin's even rows
            e[4 + 2 * j] = 0;
            e[5 + 2 * j] = q.pr | (q.sr << 16);  // same parity as the real levels'
            continue;
          }
          const int ty = g.ty[(size_t)dl * nn + n];
          const int prow = q.pr + q.tymax - ty, srow = q.sr + q.tymax - ty;
          e[4 + 2 * j] = q.txmax - g.tx[(size_t)dl * nn + n];
          e[5 + 2 * j] = prow | (srow << 16);
          if ((prow | srow) & 1) even = false;
          if (!(prow & 1) || (srow & 1)) odd = false;
        }
      }
    }
  p.par = even ? kParEven : odd ? kParOdd : kParMixed;
  return p;
}

// One reference view's variant: its shift plan for (K, DPW, NW) and the band
// pitch (the template BW, or a wider one forced through mvs_set_ncc_variant),
// if its nb band buffers fit `cap` bytes of LDS.
bool try_plan(const NccTuning& t, int K, int dpw, int nw, const float* levels, int D, int nn, const float* fdx,
              const float* fdy, float bl, size_t cap, int nb, ViewPlan& o) {
  ViewPlan p = make_plan(K, dpw, nw, levels, D, nn, fdx, fdy, bl);
  const int bw = std::max(p.width, t.force_bw);
  const int pitch = scalar_pitch(bw);
  if (scalar_lds_bytes(nb, p.pk_pairs + p.st_pairs, pitch, nw, false) > cap || bw > 256) return false;
  p.nb = nb;
  p.width = pitch;
  p.cap = cap;
  o = std::move(p);
  return true;
}

// waves per workgroup and levels per wave: MVS_NCC_NW (4|8), MVS_NCC_DPW
// (1|2|4), or the override (mvs_set_ncc_variant), tried first.  Then the
// widest variant whose double-buffered bands leave room for two workgroups per
// CU (vertical shifts grow the bands: fewer levels per step then beat a single
// resident workgroup), then any that fits the LDS.
bool choose_variant(const NccTuning& t, int K, const float* levels, int D, int nn, const float* fdx,
                    const float* fdy, float bl, ViewPlan& o) {
  const int dpw_pref = t.force_dpw ? t.force_dpw : t.dpw;
  const int nw_pref = t.force_nw ? t.force_nw : t.nw;
  auto fits = [&](int dpw, int nw, size_t cap, int nb) {
    return try_plan(t, K, dpw, nw, levels, D, nn, fdx, fdy, bl, cap, nb, o);
  };
  if (t.force_nw || t.force_dpw) {  // a forced variant is tried first, at the full LDS
    const int nw = nw_pref >= 8 && dpw_pref >= 2 ? 8 : 4;
    const int dpw = dpw_pref >= 4 ? 4 : dpw_pref >= 2 ? 2 : 1;
    if (fits(dpw, nw, kLdsCu, 2)) return true;
  }
  // A K = 5 list whose double-buffered 32-level bands miss two workgroups per
  // CU (C4's 5-NN lists: vertical and diagonal bands) tries them single-
  // buffered before halving the chunk (k_ncc_volume's NB), and a list too
  // tall even for that (C4's corner views: a neighbour two rows away) takes
  // 8 waves x 2 levels single-buffered before 4 waves: C4 step 48.1 -> 46.6 ms,
  // fused sweep 0.71 -> 0.66 ms per view (interleaved A/B,
  // profiles/r04/abenv_c4_nb1_corner.txt).  MVS_NCC_NB=2 keeps the
  // double-buffered forms.
  const bool nb1 = K == 5 && t.nb != 2;
  const bool w8 = nw_pref >= 8;
  for (size_t cap : {kLdsTwo, kLdsCu}) {
    const bool one = nb1 && cap == kLdsTwo;
    if (w8 && dpw_pref >= 4 && (fits(4, 8, cap, 2) || (one && fits(4, 8, cap, 1)))) return true;
    if (w8 && dpw_pref >= 2 && (fits(2, 8, cap, 2) || (one && fits(2, 8, cap, 1)))) return true;  // (C4's corner views)
    if (dpw_pref >= 4 && fits(4, 4, cap, 2)) return true;
    if (dpw_pref >= 2 && fits(2, 4, cap, 2)) return true;
    if (fits(1, 4, cap, 2)) return true;
  }
  return false;
}

// ---- the matrix-core form's table: one NccMRec per (chunk of 16 ndb levels, neighbour) ----

// LDS cycles of the B-operand / stats ds_read_b128 of one step (MI355X_MICROARCH.md,
// LDS table): 4 groups of 16 lanes, one cycle per group plus one per further
// distinct 16-byte entry on a busy bank quad (entry index mod 16; identical
// entries broadcast); summed over the chunk's level blocks and the 16
// residues c of the block column.  Lane l = 16 g + n reads entry
// row(g) (BW + 1) + sh (g & 1) + col(g) + c + colo[n], BW + 1 = 1 mod 16 for
// every horizontal pitch (129, 193): B operands row(g) = g, col(g) = 0;
// K = 7 stats row(g) = 2 (g & 1), col(g) = g >> 1.  (K = 5 stats: every lane
// of a read on one row, column g -- no shift changes them.)
int bank_cycles(const int16_t* colo, int dc, int sh, bool k7_stats) {
  static const int grp[4][16] = {{0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27},
                                 {4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31},
                                 {32, 33, 34, 35, 44, 45, 46, 47, 52, 53, 54, 55, 56, 57, 58, 59},
                                 {36, 37, 38, 39, 40, 41, 42, 43, 48, 49, 50, 51, 60, 61, 62, 63}};
  // (a residue c adds to every entry alike: it rotates the quads and leaves
  // the count unchanged, so c = 0 stands for all 16)
  int cyc = 0;
  for (int b0 = 0; b0 < dc; b0 += 16)
      for (const auto& gr : grp) {
        int ent[16], most = 1;
        for (int i = 0; i < 16; i++) {
          const int l = gr[i], g = l >> 4;
          const int row = k7_stats ? 2 * (g & 1) : g, col = k7_stats ? g >> 1 : 0;
          ent[i] = row * 129 + sh * (g & 1) + col + (colo[b0 + (l & 15)] & 0xff) + 64;
        }
        for (int q = 0; q < 16; q++) {  // distinct entries on bank quad q
          int n = 0;
          for (int i = 0; i < 16; i++) {
            if ((ent[i] & 15) != q) continue;
            bool dup = false;
            for (int k = 0; k < i; k++) dup |= ent[k] == ent[i];
            n += !dup;
          }
          most = std::max(most, n);
        }
        cyc += most;
      }
  return cyc;
}
// the shift of fewest cycles among those the band's slack allows (a shifted
// row must stay inside its BW + 1 slot: |sh| <= BW + 1 - band_w; ties: the
// smaller |sh|, then the negative one)
int bank_shift_eval(const int16_t* colo, int dc, bool k7_stats, int slack) {
  int best = 0, best_cyc = bank_cycles(colo, dc, 0, k7_stats);
  for (int sh : {-1, 1, -2, 2}) {
    if (std::abs(sh) > slack) continue;
    const int c = bank_cycles(colo, dc, sh, k7_stats);
    if (c < best_cyc) {
      best_cyc = c;
      best = sh;
    }
  }
  return best;
}
// memoised: the plan is rebuilt per call, and a level block's offsets repeat
// from call to call (a pure function of them, shared by every context)
int bank_shift(const int16_t* colo, int dc, bool k7_stats, int slack) {
  static std::mutex mu;
  static std::map<std::vector<int16_t>, int> memo;
  std::vector<int16_t> key(colo, colo + dc);
  key.push_back((int16_t)(k7_stats ? 1 : 0));
  key.push_back((int16_t)std::min(slack, 2));  // (shifts beyond 2 are never tried)
  std::lock_guard<std::mutex> lock(mu);
  const auto it = memo.find(key);
  if (it != memo.end()) return it->second;
  const int v = bank_shift_eval(colo, dc, k7_stats, slack);
  if (memo.size() >= (1u << 16)) memo.clear();  // bounded: ~64 K level blocks (a few MB)
  memo.emplace(std::move(key), v);
  return v;
}

ViewPlan make_plan_mfma(int K, int ndb, int nb, const float* levels, int D, int nn, const float* fdx,
                        const float* fdy, float bl) {
  const int dc = 16 * ndb;
  const SweepGeom g = chunk_geometry(K, dc, levels, D, nn, fdx, fdy, bl);
  ViewPlan p;
  p.mfma = true;
  p.ndb = ndb;
  p.nb = nb;
  p.width = g.band_w;
  p.pk_pairs = g.pk_pairs;
  p.st_pairs = g.st_pairs;
  p.steps = g.nch * nn;
  for (int n = 0; n < nn; n++)
    if (fdy[n] != 0.0f) p.vert = true;
  p.table.assign((size_t)g.nch * nn * kRecWords, 0);
  for (int c = 0; c < g.nch; c++)
    for (int n = 0; n < nn; n++) {
      const ChunkGeom& q = g.at(c, n);
      int32_t* e = p.table.data() + ((size_t)c * nn + n) * kRecWords;
      e[0] = q.txmax;
      e[1] = q.tymax;
      e[2] = q.bhp;                              // pk pair rows: every level's y0-R .. y0+TH+R-1 shifted
      e[3] = q.shp | ((q.txmax - q.txmin) << 16);  // stats pair rows | the chunk's column span
      // per level j of the chunk: txmax - tx(j) | o_j << 8, o_j the band row of
      // the level's footprint (the pk and stats bands start sr off a pair alike)
      int16_t co[32];
      for (int j = 0; j < dc; j++) {
        const int dl = c * dc + j;
        // a dummy level past the end: the band origin (in-band)
        co[j] = (int16_t)(dl < D ? (q.txmax - g.tx[(size_t)dl * nn + n]) | ((q.sr + q.tymax - g.ty[(size_t)dl * nn + n]) << 8)
                                 : q.sr << 8);
      }
      std::memcpy(e + 4, co, sizeof(int16_t) * dc);
      // horizontal lists: the odd pk rows' shift (bits 24..31 of word 3) and,
      // K = 7, the stats rows' (bits 8..15) that leave step()'s reads the
      // fewest LDS cycles.  Slack: the band pitch BW + 1 less this step's
      // 64 + span columns
      if (!p.vert) {
        const int bw = 64 + q.txmax - q.txmin, slack = mfma_pitch(false, false, K, bw) + 1 - bw;
        e[3] |= (bank_shift(co, dc, false, slack) & 0xff) << 24;
        if (K == 7) e[3] |= (bank_shift(co, dc, true, slack) & 0xff) << 8;
      }
    }
  return p;
}

// ---- runs: consecutive views of one form share a launch ----
bool same_form(const ViewPlan& a, const ViewPlan& b) {
  return a.mfma == b.mfma && a.vert == b.vert && a.dpw == b.dpw && a.nw == b.nw && a.ndb == b.ndb && a.nb == b.nb;
}
struct Run {
  int width, pk_pairs, st_pairs, par, steps;
  size_t cap;
  explicit Run(const ViewPlan& v)
      : width(v.width), pk_pairs(v.pk_pairs), st_pairs(v.st_pairs), par(v.par), steps(v.steps), cap(v.cap) {}
  // the bands of the run with v merged in: the widest, the tallest, under every member's cap
  size_t lds(const ViewPlan& form, int K, int D) const {
    if (!form.mfma) return scalar_lds_bytes(form.nb, pk_pairs + st_pairs, width, form.nw, false);
    const int dc = 16 * form.ndb;
    return mfma_lds_bytes(mfma_pitch(form.vert, D % dc != 0, K, width), form.nb, pk_pairs + st_pairs, steps, dc);
  }
  bool add(const ViewPlan& v, int K, int D) {
    Run m = *this;
    m.width = std::max(width, v.width);
    m.pk_pairs = std::max(pk_pairs, v.pk_pairs);
    m.st_pairs = std::max(st_pairs, v.st_pairs);
    m.steps = std::max(steps, v.steps);
    m.cap = std::min(cap, v.cap);
    if (v.par != par) m.par = kParMixed;
    if (m.lds(v, K, D) > m.cap) return false;
    *this = m;
    return true;
  }
};

// One reference view's form.  The matrix-core form (k_ncc_mfma, where mf_on)
// takes horizontal lists (every vertical shift 0) in 32-level (K = 5) or
// 16-level (K = 7: its 2 x 8-pixel blocks' operands take 32 VGPRs) double-
// buffered chunks, and K = 5 lists with vertical / diagonal neighbours (VERT)
// in the first of 32-level double- / single-buffered, 16-level double- /
// single-buffered chunks whose bands leave two workgroups per CU (mfma_v 1;
// 22 | 21 | 12 | 11: that form at the full LDS; 0: the scalar kernels).  Every
// other view takes the scalar kernels; false if no band holds its shifts.
bool choose_view(const NccTuning& t, bool mf_on, bool horiz, int K, const float* levels, int D, int nn,
                 const float* fdx, const float* fdy, float bl, ViewPlan& o) {
  if (mf_on && horiz && nn > 0) {
    // the run keeps every step's level offsets in LDS: past the 160 KB of a
    // CU (large D with many neighbours) the scalar kernels take the view
    ViewPlan pm = make_plan_mfma(K, K == 5 ? 2 : 1, 2, levels, D, nn, fdx, fdy, bl);
    pm.cap = kLdsCu;
    if (pm.width <= 192 && Run(pm).lds(pm, K, D) <= pm.cap) {
      o = std::move(pm);
      return true;
    }
  }
  if (mf_on && K == 5 && !horiz && nn > 0 && t.mfma_v != 0) {
    static const int forms[4][2] = {{2, 2}, {2, 1}, {1, 2}, {1, 1}};  // {16-level blocks, band buffers}
    const bool forced = t.mfma_v > 1;
    for (const auto& f : forms) {
      if (forced && t.mfma_v != 10 * f[0] + f[1]) continue;
      ViewPlan pm = make_plan_mfma(K, f[0], f[1], levels, D, nn, fdx, fdy, bl);
      pm.cap = forced ? kLdsCu : kLdsTwo;
      if (pm.width > 128 || Run(pm).lds(pm, K, D) > pm.cap) continue;
      pm.cap = kLdsTwo;  // a run of them stays under two workgroups per CU
      o = std::move(pm);
      return true;
    }
  }
  return choose_variant(t, K, levels, D, nn, fdx, fdy, bl, o);
}

void fill_work_map(NccArgs& a, int dc) {
  a.tiles_x = (a.W + 63) / 64;
  a.ntiles = a.tiles_x * ((a.H + kTileH - 1) / kTileH);
  a.tiles_per_xcd = (a.nref * a.ntiles + 7) / 8;
  a.nch = (a.D + dc - 1) / dc;
}

}  // namespace

// Each view's variant is chosen on its own shifts; runs of consecutive views
// of the same form whose merged bands still fit every member's LDS cap share
// one launch (up to kMaxRef views, fused sweep only: a cost volume holds one
// view), with the widest band stride and a parity-specific kernel only when
// every member has that parity -- the same arithmetic, one kernel boundary
// (~11 us between two of these launches) per run.
bool plan_ncc_launches(const NccTuning& t, int V, int W, int H, int K, int D, const float* levels, const int* vs,
                       const int* sn, int aw, float bl, int z0, int z1, bool want_volume,
                       std::vector<NccLaunch>& out, std::string& err) {
  out.clear();
  auto fail = [&](const char* what) {
    err = what;
    return false;
  };
  if (want_volume && z1 - z0 != 1) return fail("the NCC cost volume holds one reference view");
  if (W < 2) return fail("NCC sweep needs W >= 2");
  if (K != 5 && K != 7) return fail("NCC window must be 5 or 7");
  if (!want_volume && D > 65535) return fail("fused NCC sweep: at most 65535 levels");  // K = 7 packs levels in 16 bits
  const int n = z1 - z0;
  if (n <= 0) return true;
  // the matrix-core form: fused views only; a forced variant (mvs_set_ncc_variant) keeps the scalar
  // kernels, and so does a view plane of 2 GB or more (the band DMA addresses it by 32-bit byte offsets)
  const bool small_plane = (long)W * (H + (H & 1)) * 8 < 0x7fffffffL;
  const bool mf_on = !want_volume && (K == 5 || t.mfma7 != 0) && t.mfma != 0 && !t.force_nw && !t.force_dpw &&
                     !t.force_general && !t.force_bw && small_plane;
  std::vector<ViewPlan> vp(n);
  for (int r = 0; r < n; r++) {
    const int z = z0 + r, nn = sn[z];
    if (nn > kMaxNbr) return fail("NCC sweep supports at most 16 neighbours per reference view");
    float fdx[kMaxNbr], fdy[kMaxNbr];
    bool horiz = true;
    for (int k = 0; k < nn; k++) {
      const int v = vs[V * z + k];
      if (v < 0 || v >= V) return fail("view_subset entry out of range");
      fdx[k] = (float)(v % aw - z % aw);
      fdy[k] = (float)(v / aw - z / aw);
      if (fdy[k] != 0.0f) horiz = false;
    }
    if (!choose_view(t, mf_on, horiz, K, levels, D, nn, fdx, fdy, bl, vp[r]))
      return fail("NCC sweep: neighbour shifts too large for the LDS band");
  }
  for (int i = 0; i < n;) {
    const ViewPlan& f = vp[i];
    Run run(f);
    int j = i + 1;
    while (j < n && j - i < t.run && same_form(f, vp[j]) && run.add(vp[j], K, D)) j++;
    NccLaunch L;
    L.mfma = f.mfma;
    L.K = K;
    L.first = i;
    L.FUSE = want_volume ? 0 : 1;
    NccArgs& a = L.args;
    a.W = W;
    a.H = H;
    a.D = D;
    a.nref = j - i;
    a.pk_pairs = run.pk_pairs;
    a.st_pairs = run.st_pairs;
    for (int r = i; r < j; r++) {
      const int z = z0 + r, nn = sn[z];
      a.z[r - i] = z;
      a.nn[r - i] = nn;
      a.plan[r - i] = (int)(L.table.size() / kRecWords);
      for (int k = 0; k < nn; k++) a.view[r - i][k] = vs[V * z + k];
      const size_t r0 = L.table.size();
      L.table.insert(L.table.end(), vp[r].table.begin(), vp[r].table.end());
      if (!f.mfma) continue;
      // each record's neighbour plane as a byte offset (words 22, 23): the
      // kernel rebases its band DMA on it with no per-step multiply
      for (size_t rr = r0; rr < L.table.size(); rr += kRecWords) {
        const int nloc = (int)((rr - r0) / kRecWords) % nn;
        const unsigned long long off = (unsigned long long)a.view[r - i][nloc] * (unsigned long long)W *
                                       (unsigned long long)((H + 1) >> 1) * 16ull;  // 16 B per (pair row, column)
        L.table[rr + 22] = (int32_t)(off & 0xffffffffull);
        L.table[rr + 23] = (int32_t)(off >> 32);
        a.txmax_all = std::max(a.txmax_all, L.table[rr]);
      }
    }
    if (f.mfma) {
      const int dc = 16 * f.ndb;
      L.TAIL = D % dc != 0;
      L.VERT = f.vert;
      L.NDB = f.ndb;
      L.NB = f.nb;
      L.BW = mfma_pitch(f.vert, L.TAIL, K, run.width);
      L.tmax = run.steps;
      // timing probes, on the three shapes that have one (C5's, C2's, C4's interior lists)
      if (t.mfma_dbg && !L.TAIL) {
        if (f.vert) {
          if (L.NDB == 1 && L.NB == 2 && L.BW == 80 && (t.mfma_dbg == 1 || t.mfma_dbg == 2)) L.DBG = t.mfma_dbg;
        } else if ((K == 7 && L.BW == 128) || (K == 5 && L.BW == 192)) {
          L.DBG = t.mfma_dbg == 1 ? 1 : 2;
        }
      }
      L.lds = mfma_lds_bytes(L.BW, L.NB, run.pk_pairs + run.st_pairs, L.tmax, dc);
      fill_work_map(a, dc);
      const int last[8] = {K, kTileH, dc, 8, L.BW, f.vert ? kParMixed : (K == 5 ? kParEven : kParOdd), 1, L.NB};
      std::copy(last, last + 8, L.last);
    } else {
      // the parity-specific kernels only where they occur (kParEven for K = 5,
      // kParOdd for K = 7: horizontal bands); single-buffered bands take any parity
      const int kpar = K == 5 ? kParEven : kParOdd;
      L.DPW = f.dpw;
      L.NW = f.nw;
      L.NB = f.nb;
      L.BW = run.width;
      L.PAR = f.nb == 2 && run.par == kpar && !t.force_general ? kpar : kParMixed;
      a.plane32 = small_plane && t.plane32 != 0;
      L.lds = scalar_lds_bytes(f.nb, run.pk_pairs + run.st_pairs, run.width, f.nw, !want_volume);
      fill_work_map(a, f.nw * f.dpw);
      const int last[8] = {K, kTileH, f.dpw, f.nw, L.BW, L.PAR, L.FUSE, L.NB};
      std::copy(last, last + 8, L.last);
    }
    out.push_back(std::move(L));
    i = j;
  }
  return true;
}

}  // namespace ncc
}  // namespace mvs
