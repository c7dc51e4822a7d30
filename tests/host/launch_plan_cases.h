// Cases of the golden of the SLIC, superpixel-sweep, SAD and filter launch
// planners (tests/golden/launch_plans.txt) and the canonical line a planned
// launch prints as.  Numbers only, no images: a case is a set of MVS_SLIC_*,
// MVS_SWEEP_*, MVS_SAD_* and MVS_FILTER_* knobs and a list of planner calls.
#pragma once
#include <array>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <string>
#include <utility>
#include <vector>

namespace plancase {

enum Kind { kSweep, kSad, kFilter, kSlic };
struct Call {
  Kind kind = kSweep;
  int aw = 1, ah = 1, W = 96, H = 64, S = 8;
  int V = 0;  // 0: aw * ah (the filter takes any V)
  int D = 32;
  float dmin = 0.0f, dinc = 1.0f;                  // level l = dmin + l * dinc ...
  std::vector<std::pair<int, float>> level_patch;  // ... but for these
  float bl = 1.0f;
  int nh = 0, nv = 0;                         // neighbour lists: the (2nh+1) x (2nv+1) box around a view
  std::vector<std::pair<int, int>> vs_patch;  // view_subset entries overwritten (index, value)
  int z0 = 0, z1 = -1;                        // reference views (z1 < 0: all of them)
  bool allow_relayout = true;                 // sweep: false plans as after a failed scratch allocation
  int ya = 0, yb = -1;                        // filter: rows (yb < 0: H)
  bool band = false;
  int no_iter = 5, edge = 0, search = 0, conn = 0;  // SLIC: mvs_slic_params
};
struct Case {
  std::string name;
  std::vector<std::pair<const char*, const char*>> env;
  std::vector<Call> calls;
};

// the arrays a call hands to the planner (cl_multiview_stereo_amd/params.py's lists)
struct Inputs {
  int V = 0;
  std::vector<float> levels;
  std::vector<int> vs, sn;
};
inline Inputs make_inputs(const Call& c) {
  Inputs in;
  const int V = in.V = c.aw * c.ah;
  for (int l = 0; l < c.D; l++) in.levels.push_back(c.dmin + (float)l * c.dinc);
  for (const auto& p : c.level_patch) in.levels[p.first] = p.second;
  in.vs.assign((size_t)V * V, 0);
  in.sn.assign(V, 0);
  for (int i = 0; i < V; i++) {
    const int cx = i % c.aw, cy = i / c.aw;
    int n = 0;
    for (int x = cx - c.nh; x <= cx + c.nh; x++)
      for (int y = cy - c.nv; y <= cy + c.nv; y++)
        if (x >= 0 && x < c.aw && y >= 0 && y < c.ah && y * c.aw + x != i) in.vs[(size_t)i * V + n++] = y * c.aw + x;
    in.sn[i] = n;
  }
  for (const auto& p : c.vs_patch) in.vs[p.first] = p.second;
  return in;
}

inline uint64_t fnv1a(const int32_t* w, size_t n) {
  uint64_t h = 0xcbf29ce484222325ull;
  for (size_t i = 0; i < n; i++)
    for (int b = 0; b < 4; b++) {
      h ^= ((uint32_t)w[i] >> (8 * b)) & 0xffu;
      h *= 0x100000001b3ull;
    }
  return h;
}

// ---- the canonical lines -----------------------------------------------------
inline void print_none(FILE* f, int call) { fprintf(f, "c%d none\n", call); }
inline void print_error(FILE* f, int call, int z, const char* msg) {  // z < 0: a whole call
  if (z < 0)
    fprintf(f, "c%d error: %s\n", call, msg);
  else
    fprintf(f, "c%d z%d error: %s\n", call, z, msg);
}
// one superpixel-sweep launch: the form (0 general, 1 HZ gathers, 2 HZ ring, 3
// re-laid), the kernel's template and wave-count arguments, the grid, the
// superpixel map, the slot table as uploaded (length 0 without re-laid views)
// and the re-layout launches in order as view:kind:slot
inline void print_sweep(FILE* f, int call, int form, int lps, int wps, unsigned gx, unsigned gy, int mw, int mh,
                        long tstride, long units, const int32_t* slot, size_t nslot,
                        const std::vector<std::array<int, 3>>& relayouts, const int last[5]) {
  fprintf(f, "c%d sweep form=%d lps=%d wps=%d grid=%u,%u map=%d,%d tstride=%ld units=%ld slots=%zu:%016llx relayouts=",
          call, form, lps, wps, gx, gy, mw, mh, tstride, units, nslot, (unsigned long long)fnv1a(slot, nslot));
  for (size_t i = 0; i < relayouts.size(); i++)
    fprintf(f, "%s%d:%d:%d", i ? "," : "", relayouts[i][0], relayouts[i][1], relayouts[i][2]);
  if (relayouts.empty()) fprintf(f, "-");
  fprintf(f, " last=%d,%d,%d,%d,%d\n", last[0], last[1], last[2], last[3], last[4]);
}
// one SAD launch of reference view z; args: SadArgs as its 11 ints
// W,H,D,nn,z,tiles_x,ntiles,tiles_per_xcd,nch,bw,brows
inline void print_sad_band(FILE* f, int call, int z, int TH, int PPW, int AFF, int BWT, const int32_t* args,
                           unsigned gx, size_t lds, const int32_t* table, size_t ntable) {
  fprintf(f, "c%d z%d sad kern=band TH=%d PPW=%d AFF=%d BWT=%d args=", call, z, TH, PPW, AFF, BWT);
  for (int i = 0; i < 11; i++) fprintf(f, "%s%d", i ? "," : "", args[i]);
  fprintf(f, " grid=%u lds=%zu table=%zu:%016llx\n", gx, lds, ntable, (unsigned long long)fnv1a(table, ntable));
}
inline void print_sad_gather(FILE* f, int call, int z, unsigned gx, unsigned gy) {
  fprintf(f, "c%d z%d sad kern=gather grid=%u,%u\n", call, z, gx, gy);
}
// one filter launch; kern: sel8 px16_8 q px32 sel64 plain; FB NS ROWB RM inb are q's (px32: FB), else 0
inline void print_filter(FILE* f, int call, const char* kern, int FB, int NS, int ROWB, int RM, int inb,
                         const unsigned grid[3], unsigned block, long PP, long proj_off) {
  fprintf(f, "c%d filter kern=%s FB=%d NS=%d ROWB=%d RM=%d inb=%d grid=%u,%u,%u block=%u PP=%ld off=%ld\n", call, kern,
          FB, NS, ROWB, RM, inb, grid[0], grid[1], grid[2], block, PP, proj_off);
}
// one SLIC launch: the kernel and its template coordinates, the grid and
// block, the pointer arguments by role (lab, spixl, labels, scratch, null) and
// the scalar arguments in the kernel's parameter order (xy, col: the float's
// bits); colour weight, passed through untouched, is left out
using SlicInt = std::pair<const char*, long>;
using SlicBuf = std::pair<const char*, const char*>;
inline void print_slic(FILE* f, int call, const char* kern, std::initializer_list<SlicInt> tmpl, unsigned gx,
                       unsigned gy, unsigned gz, unsigned block, std::initializer_list<SlicBuf> bufs,
                       std::initializer_list<SlicInt> args, const float* xy_col = nullptr) {
  fprintf(f, "c%d slic %s", call, kern);
  const char* sep = "<";
  for (const SlicInt& t : tmpl) fprintf(f, "%s%s=%ld", sep, t.first, t.second), sep = ",";
  fprintf(f, "%s grid=%u,%u,%u block=%u bufs=", tmpl.size() ? ">" : "", gx, gy, gz, block);
  sep = "";
  for (const SlicBuf& b : bufs) fprintf(f, "%s%s:%s", sep, b.first, b.second), sep = ",";
  fprintf(f, " args=");
  sep = "";
  for (const SlicInt& a : args) fprintf(f, "%s%s:%ld", sep, a.first, a.second), sep = ",";
  if (xy_col) {
    uint32_t u[2];
    memcpy(u, xy_col, sizeof u);
    fprintf(f, ",xy:%08x,col:%08x", u[0], u[1]);
  }
  fprintf(f, "\n");
}
inline void print_slic_scratch(FILE* f, int call, size_t bytes) { fprintf(f, "c%d slic scratch=%zu\n", call, bytes); }

// ---- the cases -----------------------------------------------------------------
inline Call sweep(int aw, int ah, int nh, int nv, int D) {
  Call c;
  c.kind = kSweep, c.aw = aw, c.ah = ah, c.nh = nh, c.nv = nv, c.D = D;
  return c;
}
inline Call sad(int aw, int ah, int nh, int nv, int D, float dinc = 1.0f, float bl = 1.0f) {
  Call c;
  c.kind = kSad, c.aw = aw, c.ah = ah, c.nh = nh, c.nv = nv, c.D = D, c.dinc = dinc, c.bl = bl;
  c.W = 100, c.H = 70;
  return c;
}
inline Call filter(int V, int aw, int W = 100, int H = 70) {
  Call c;
  c.kind = kFilter, c.V = V, c.aw = aw, c.W = W, c.H = H;
  return c;
}
inline Call slic(int V, int W, int H, int S, int no_iter = 5) {
  Call c;
  c.kind = kSlic, c.V = V, c.W = W, c.H = H, c.S = S, c.no_iter = no_iter, c.D = 0;
  return c;
}

// planner inputs of bench configuration C4's size (8 x 4 array, 1920 x 1080,
// S = 32, 128 levels; the 3 x 3 box of neighbours), one call per launcher: --time
inline std::vector<Call> c4_calls() {
  Call w = sweep(8, 4, 1, 1, 128), s = sad(8, 4, 1, 1, 128), f = filter(32, 8, 1920, 1080);
  w.W = s.W = 1920, w.H = s.H = 1080, w.S = 32;
  s.z0 = 9, s.z1 = 10;  // an inner view: 8 neighbours
  return {w, s, f};
}
// the SLIC call of bench configuration C2 (5 views, 1920 x 1080, S = 32, 5 iterations): --time
inline Call c2_slic_call() { return slic(5, 1920, 1080, 32, 5); }

inline std::vector<Case> cases() {
  std::vector<Case> cs;
  const int Ds[7] = {32, 33, 64, 65, 130, 200, 256};
  // -- superpixel sweep: a 5 x 1 array, integer levels: ring (half-wave HZ at D = 32), under each knob
  std::vector<Call> row;
  for (int D : Ds) row.push_back(sweep(5, 1, 2, 0, D));
  cs.push_back({"sweep_row", {}, row});
  cs.push_back({"sweep_row_ring0", {{"MVS_SWEEP_RING", "0"}}, row});
  cs.push_back({"sweep_row_hz0", {{"MVS_SWEEP_HZ", "0"}}, row});
  cs.push_back({"sweep_row_wps1", {{"MVS_SWEEP_WPS", "1"}}, row});
  cs.push_back({"sweep_row_wps2", {{"MVS_SWEEP_WPS", "2"}}, row});
  cs.push_back({"sweep_row_wps4", {{"MVS_SWEEP_WPS", "4"}}, row});
  cs.push_back({"sweep_row_wps3_invalid", {{"MVS_SWEEP_WPS", "3"}}, row});
  cs.push_back({"sweep_row_wps2_ring0", {{"MVS_SWEEP_WPS", "2"}, {"MVS_SWEEP_RING", "0"}}, row});
  cs.push_back({"sweep_row_tr0", {{"MVS_SWEEP_TRANSPOSE", "0"}}, row});
  cs.push_back({"sweep_row_tr1", {{"MVS_SWEEP_TRANSPOSE", "1"}}, row});
  cs.push_back({"sweep_row_tr2", {{"MVS_SWEEP_TRANSPOSE", "2"}}, row});
  {  // fractional levels: the general form; a huge level: not below 2^24
    Call a = sweep(5, 1, 2, 0, 32), b = sweep(5, 1, 2, 0, 100), c = sweep(5, 1, 1, 0, 64);
    a.dinc = b.dinc = 0.5f;
    c.level_patch = {{63, 16777216.0f}};
    cs.push_back({"sweep_fractional", {}, {a, b, c}});
  }
  {  // a 3 x 3 array, vertical and both diagonal neighbours: re-laid; without the scratch: general
    std::vector<Call> sq;
    for (int D : {32, 64, 200}) {
      Call a = sweep(3, 3, 1, 1, D);
      a.W = 100, a.H = 70;
      sq.push_back(a);
      a.allow_relayout = false;
      sq.push_back(a);
    }
    Call v = sweep(1, 3, 0, 1, 64);  // one camera column
    sq.push_back(v);
    cs.push_back({"sweep_square", {}, sq});
    cs.push_back({"sweep_square_tr0", {{"MVS_SWEEP_TRANSPOSE", "0"}}, sq});  // another camera row: no HZ
    cs.push_back({"sweep_square_tr1", {{"MVS_SWEEP_TRANSPOSE", "1"}}, sq});
    cs.push_back({"sweep_square_wps1", {{"MVS_SWEEP_WPS", "1"}}, sq});
    Call r = sweep(3, 3, 1, 1, 64);  // a sub-range of references
    r.z0 = 3, r.z1 = 5;
    Call r2 = sweep(4, 3, 1, 1, 40);
    r2.z0 = 0, r2.z1 = 1;
    cs.push_back({"sweep_square_range", {}, {r, r2}});
  }
  {  // the ring form's window bound: S = 40, |dx| = 4, range 63 over 64 levels (333 columns) and 64 (337)
    Call a = sweep(5, 1, 4, 0, 64), b = a, c = sweep(5, 1, 4, 0, 128), d = c;
    a.S = b.S = c.S = d.S = 40;
    a.W = b.W = c.W = d.W = 640, a.H = b.H = c.H = d.H = 480;
    b.level_patch = {{63, 64.0f}};
    d.level_patch = {{127, 128.0f}};  // the second chunk's range
    Call e = a;
    e.S = 41;  // 2 (S - 1) = 80: 335 columns
    Call g = e;
    g.S = 42;  // 337
    cs.push_back({"sweep_ring_bound", {}, {a, b, c, d, e, g}});
  }
  {
    Call a = sweep(5, 1, 2, 0, 64);
    a.z0 = 1, a.z1 = 3;
    Call b = a;
    b.z0 = 4, b.z1 = 5;
    Call e = a;
    e.z0 = e.z1 = 2;  // an empty range
    cs.push_back({"sweep_row_range", {}, {a, b, e}});
  }
  {  // view_subset entries out of range: skipped by the slot loop, seen by the HZ and ring loops
    Call a = sweep(5, 1, 2, 0, 64), b = a, c = sweep(3, 3, 1, 1, 64), d = c, s = sweep(5, 1, 1, 0, 64);
    a.vs_patch = {{0, 5}};
    b.vs_patch = {{1, -1}};
    c.vs_patch = {{0, 9}, {1, -3}};
    d.vs_patch = {{0, 9}, {1, -3}};
    d.allow_relayout = false;
    // a view listed as its own neighbour is re-laid (same camera column) and
    // lies in the reference's camera row: without the scratch the call is HZ
    s.vs_patch = {{0, 0}};
    Call s2 = s;
    s2.allow_relayout = false;
    Call s3 = s2;
    s3.D = 32;
    cs.push_back({"sweep_bad_views", {}, {a, b, c, d, s, s2, s3}});
  }
  {
    Call a = sweep(3, 1, 1, 0, 64);
    a.W = 8192, a.H = 8192;  // (W + H) H 16 = 2^31
    Call b = a;
    b.W = 8191;  // just under
    Call e = a;
    e.z0 = e.z1 = 1;  // empty comes first
    cs.push_back({"sweep_too_large", {}, {a, b, e}});
  }

  // -- SAD
  {
    std::vector<Call> h = {sad(3, 1, 1, 0, 32),   // horizontal integer shifts: bw 128
                           sad(1, 3, 0, 1, 32),   // vertical: bw 64
                           sad(3, 1, 1, 0, 21),   // D no multiple of the chunk
                           sad(3, 1, 1, 0, 7),
                           sad(3, 3, 1, 1, 20),
                           sad(3, 1, 1, 0, 32, 5.0f),    // bw past 64 SB_NBLK with 16 levels: 8-level chunks
                           sad(3, 1, 1, 0, 32, 10.0f),   // and with 8: gather
                           sad(3, 1, 1, 0, 32, 0.5f),    // fractional column shifts: gather
                           sad(1, 3, 0, 1, 32, 1.0f, 1.3f),  // integral fdx, fractional fdy: the row table
                           sad(3, 3, 1, 1, 16, 1.0f, 0.5f),
                           sad(1, 3, 0, 1, 32, 5.0f),    // LDS over 160 KB with 16 levels
                           sad(1, 3, 0, 1, 32, 10.0f),   // and with 8: gather
                           sad(3, 1, 1, 0, 16, 100000.0f)};  // a shift past 1e6
    h[4].z0 = 3, h[4].z1 = 6;
    cs.push_back({"sad_auto", {}, h});
    cs.push_back({"sad_aff_off", {{"MVS_SAD_AFF", "1"}}, h});
    cs.push_back({"sad_named_gather", {{"MVS_SAD_KERNEL", "gather"}}, {h[0], h[7]}});
    cs.push_back({"sad_named_sys8x2", {{"MVS_SAD_KERNEL", "sys8x2"}}, {h[0], h[1], h[8]}});
    cs.push_back({"sad_named_sys8", {{"MVS_SAD_KERNEL", "sys8"}}, {h[0], h[5], h[10]}});
    cs.push_back({"sad_named_sys8x2_unfit", {{"MVS_SAD_KERNEL", "sys8x2"}}, {h[5]}});
    cs.push_back({"sad_named_sys8_unfit", {{"MVS_SAD_KERNEL", "sys8"}}, {h[6]}});
    cs.push_back({"sad_named_auto", {{"MVS_SAD_KERNEL", "auto"}}, {h[0], h[7]}});
    cs.push_back({"sad_named_unknown", {{"MVS_SAD_KERNEL", "sys16"}}, {h[0]}});
  }

  // -- filter
  {
    std::vector<Call> vv = {filter(5, 5),   filter(8, 4),   filter(9, 3),   filter(16, 4), filter(17, 17),
                            filter(32, 8),  filter(33, 11), filter(64, 8),  filter(65, 13)};
    std::vector<Call> big = {filter(8, 4, 8192, 8192), filter(32, 8, 4096, 4096), filter(64, 8, 4096, 2048),
                             filter(8, 4, 8192, 8191), filter(32, 8, 4096, 4095), filter(64, 8, 4096, 2047)};
    cs.push_back({"filter_views", {}, vv});
    cs.push_back({"filter_off32", {}, big});
    cs.push_back({"filter_px", {{"MVS_FILTER_KERNEL", "px"}}, vv});
    // 16 < V <= 32: q's coordinates; aw = 8, 5 (no multiple of 2 or 4), 6 (of 2 only), V % aw != 0
    std::vector<Call> q = {filter(32, 8), filter(25, 5), filter(30, 6), filter(30, 8), big[1]};
    Call sub = filter(32, 8);
    sub.z0 = 3, sub.z1 = 12;
    q.push_back(sub);
    static const char* const fb[4] = {nullptr, "2", "4", "8"};
    static const char* const ns[3] = {nullptr, "1", "2"};
    static const char* const ord[2] = {nullptr, "ref"};
    for (const char* f : fb)
      for (const char* n : ns)
        for (const char* o : ord) {
          Case c{std::string("filter_q") + (f ? std::string("_fb") + f : "") + (n ? std::string("_ns") + n : "") +
                     (o ? "_ref" : ""),
                 {}, q};
          if (f) c.env.push_back({"MVS_FILTER_FB", f});
          if (n) c.env.push_back({"MVS_FILTER_NS", n});
          if (o) c.env.push_back({"MVS_FILTER_ORDER", o});
          cs.push_back(c);
        }
    for (const char* f : {"2", "4", "8"})
      cs.push_back({std::string("filter_px_fb") + f, {{"MVS_FILTER_KERNEL", "px"}, {"MVS_FILTER_FB", f}}, q});
    cs.push_back({"filter_bound0", {{"MVS_FILTER_BOUND", "0"}}, q});
    cs.push_back({"filter_order_other", {{"MVS_FILTER_ORDER", "rm"}, {"MVS_FILTER_KERNEL", "q"}}, q});
    // a row band, both proj layouts; no rows; no views
    std::vector<Call> rows;
    for (int V : {5, 16, 32, 64, 65})
      for (int b = 0; b < 2; b++) {
        Call c = filter(V, V == 5 ? 5 : V == 65 ? 13 : 8);
        c.ya = 10, c.yb = 30, c.band = b != 0;
        rows.push_back(c);
      }
    Call e1 = filter(32, 8), e2 = e1, e3 = e1;
    e1.ya = e1.yb = 20;
    e2.z0 = e2.z1 = 4;
    e3.ya = e3.yb = 20, e3.band = true;
    rows.insert(rows.end(), {e1, e2, e3});
    cs.push_back({"filter_rows", {}, rows});
  }

  // -- SLIC
  {
    // every S class at an image size (331 x 251) that is a multiple of neither 16 nor S; two views
    std::vector<Call> sizes, iters, srch, knob, edge;
    for (int S : {6, 8, 12, 16, 32, 40, 48, 64, 96}) sizes.push_back(slic(2, 331, 251, S));
    cs.push_back({"slic_sizes", {}, sizes});
    // no_iter 0, 1, 2, 5 on the walk path (S = 8), the 4-cell (32) and the 9-cell (48) tile path
    for (int S : {8, 32, 48})
      for (int n : {0, 1, 2, 5}) iters.push_back(slic(3, 331, 251, S, n));
    cs.push_back({"slic_iters", {}, iters});
    // search 1: k_assign<true>; the 9-cell tile kernel at S = 32 too
    for (int S : {8, 40, 32, 48, 64})
      for (int se : {0, 1})
        for (int n : {0, 5}) {
          Call c = slic(1, 331, 251, S, n);
          c.search = se;
          srch.push_back(c);
        }
    cs.push_back({"slic_search", {}, srch});
    for (int S : {32, 64, 48, 8}) knob.push_back(slic(2, 331, 251, S));
    knob.push_back(slic(2, 331, 251, 32, 0));
    cs.push_back({"slic_tiles9", {{"MVS_SLIC_TILES9", "1"}}, knob});
    cs.push_back({"slic_tiles9_other", {{"MVS_SLIC_TILES9", "2"}}, knob});
    // 16-bit label copies need mw mh <= 65536: S = 6 at 1600 x 1480 is 267 x 247 = 65949 superpixels
    // (UT = 1), S = 12 at 3200 x 2960 likewise (UT = 4); one superpixel fewer: 16-bit again
    std::vector<Call> upd = {slic(3, 100, 70, 8),        slic(2, 331, 251, 40),      slic(1, 1600, 1480, 6),
                             slic(1, 3200, 2960, 12),    slic(1, 1600, 1480, 6, 0),  slic(1, 1590, 1480, 6),
                             slic(1, 1536, 1536, 6),     slic(2, 331, 251, 32),      slic(1, 100, 70, 8, 1)};
    upd[2].conn = 1;
    cs.push_back({"slic_update", {}, upd});
    cs.push_back({"slic_update0", {{"MVS_SLIC_UPDATE", "0"}}, upd});
    cs.push_back({"slic_update1", {{"MVS_SLIC_UPDATE", "1"}}, {upd[0], upd[1]}});
    cs.push_back({"slic_update_nan", {{"MVS_SLIC_UPDATE", "walk"}}, {upd[0], upd[1]}});  // atoi: 0
    cs.push_back({"slic_both_knobs", {{"MVS_SLIC_UPDATE", "0"}, {"MVS_SLIC_TILES9", "1"}}, {upd[1], upd[7]}});
    // the edge step and the connectivity pass, both paths; no_iter = 0: the scratch is theirs alone
    for (int S : {8, 32})
      for (int e : {0, 1, 2})
        for (int cn : {0, 1}) {
          Call c = slic(2, 331, 251, S, e == 2 && cn ? 0 : 5);
          c.edge = e, c.conn = cn;
          edge.push_back(c);
        }
    Call hd = slic(1, 1920, 1080, 32);  // k_edge_store's grid: 8192 workgroups at most
    hd.edge = 1;
    edge.push_back(hd);
    cs.push_back({"slic_edge_conn", {}, edge});
    // W H = 2^27, the largest image: W H 16 = 2^31 is past the walk's and the
    // 4-cell kernel's 32-bit offsets (k_update by size, the 9-cell kernel); just under it
    cs.push_back({"slic_largest", {}, {slic(1, 16384, 8192, 40, 1), slic(1, 16384, 8192, 32, 1),
                                       slic(1, 16384, 8192, 6, 1), slic(1, 16384, 8191, 40, 1),
                                       slic(1, 16384, 8191, 32, 1)}});
    cs.push_back({"slic_c2_c5", {}, {c2_slic_call(), slic(5, 1920, 1080, 40)}});
  }
  return cs;
}

}  // namespace plancase
