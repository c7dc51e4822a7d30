// Cases of the NCC launch planner's golden (tests/golden/ncc_launch_plans.txt)
// and the canonical line a launch prints as.  Numbers only, no images: a case
// is a set of MVS_NCC_* knobs and a list of planner calls.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <string>
#include <utility>
#include <vector>

namespace plancase {

struct Call {
  int force_nw = 0, force_dpw = 0, force_bw = 0, force_general = 0;  // mvs_set_ncc_variant
  int aw = 1, ah = 1, W = 0, H = 0, K = 5;
  int dmin = 0, dmax = 0, dinc = 1;
  float bl = 1.0f;
  int nh = 0, nv = 0, knn = 0;  // neighbour lists: a (2nh+1) x (2nv+1) box, or the knn nearest
  int z0 = 0, z1 = -1;          // reference views (z1 < 0: all of them)
  bool vol = false;             // a cost volume (else the fused sweep)
  bool bad_view = false;        // view 0's first neighbour id = V (out of range)
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
  for (int d = c.dmin; d <= c.dmax; d += c.dinc) in.levels.push_back((float)d);
  in.vs.assign((size_t)V * V, 0);
  in.sn.assign(V, 0);
  for (int i = 0; i < V; i++) {
    const int cx = i % c.aw, cy = i / c.aw;
    std::vector<int> lst;
    if (c.knn) {
      std::vector<std::pair<int, int>> cand;
      for (int v = 0; v < V; v++)
        if (v != i) cand.push_back({(v % c.aw - cx) * (v % c.aw - cx) + (v / c.aw - cy) * (v / c.aw - cy), v});
      std::sort(cand.begin(), cand.end());
      for (int k = 0; k < c.knn && k < (int)cand.size(); k++) lst.push_back(cand[k].second);
    } else {
      for (int x = cx - c.nh; x <= cx + c.nh; x++)
        for (int y = cy - c.nv; y <= cy + c.nv; y++)
          if (x >= 0 && x < c.aw && y >= 0 && y < c.ah && y * c.aw + x != i) lst.push_back(y * c.aw + x);
    }
    in.sn[i] = (int)lst.size();
    for (size_t k = 0; k < lst.size() && k < (size_t)V; k++) in.vs[(size_t)i * V + k] = lst[k];
  }
  if (c.bad_view) in.vs[0] = V;
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

// One launch as one line.  coords: the template coordinates (scalar: K DPW NW
// BW PAR NB FUSE; matrix-core: K BW TAIL VERT NDB NB DBG); args: NccArgs as
// its 164 ints (every field is an int): the twelve scalars in declaration
// order, then per view of the launch "z@first record:neighbour ids", and a
// hash of the whole struct.
inline void print_launch(FILE* f, int call, bool mfma, const int coords[7], int first, const int32_t* args,
                         size_t table_len, uint64_t table_hash, int tmax, size_t lds, const int last[8]) {
  static const char* sn[7] = {"K", "DPW", "NW", "BW", "PAR", "NB", "FUSE"};
  static const char* mn[7] = {"K", "BW", "TAIL", "VERT", "NDB", "NB", "DBG"};
  fprintf(f, "c%d launch fam=%s", call, mfma ? "mfma" : "scalar");
  for (int i = 0; i < 7; i++) fprintf(f, " %s=%d", mfma ? mn[i] : sn[i], coords[i]);
  fprintf(f, " first=%d", first);
  fprintf(f, " args=");  // W,H,D,nref,tiles_x,ntiles,tiles_per_xcd,nch,pk_pairs,st_pairs,txmax_all,plane32
  for (int i = 0; i < 12; i++) fprintf(f, "%s%d", i ? "," : "", args[i]);
  const int nref = args[3];
  const int32_t *z = args + 12, *nn = z + 8, *plan = nn + 8, *view = plan + 8;
  fprintf(f, " refs=");
  for (int r = 0; r < nref && r < 8; r++) {
    fprintf(f, "%s%d@%d:", r ? ";" : "", z[r], plan[r]);
    for (int k = 0; k < nn[r] && k < 16; k++) fprintf(f, "%s%d", k ? "," : "", view[16 * r + k]);
  }
  fprintf(f, " argshash=%016llx table=%zu:%016llx tmax=%d lds=%zu last=", (unsigned long long)fnv1a(args, 164), table_len,
          (unsigned long long)table_hash, tmax, lds);
  for (int i = 0; i < 8; i++) fprintf(f, "%s%d", i ? "," : "", last[i]);
  fprintf(f, "\n");
}
inline void print_error(FILE* f, int call, const char* msg) { fprintf(f, "c%d error: %s\n", call, msg); }

inline std::vector<Case> cases() {
  std::vector<Case> out;
  auto call = [](int aw, int ah, int W, int H, int K, int dmax, int nh, int nv) {
    Call c;
    c.aw = aw, c.ah = ah, c.W = W, c.H = H, c.K = K, c.dmax = dmax, c.nh = nh, c.nv = nv;
    return c;
  };
  auto knn = [&](int aw, int ah, int W, int H, int dmax, int k, float bl) {
    Call c = call(aw, ah, W, H, 5, dmax, 0, 0);
    c.knn = k, c.bl = bl;
    return c;
  };
  typedef std::vector<std::pair<const char*, const char*>> Env;
  auto add = [&](const char* name, Env env, std::vector<Call> calls) { out.push_back({name, env, calls}); };

  // ---- horizontal lists ----
  const Call c2 = call(5, 1, 1920, 1080, 5, 127, 4, 0);         // C2: 1 x 5, band > 128 columns, D % 32 == 0
  const Call h5n = call(3, 1, 640, 480, 5, 127, 1, 0);          // band <= 128
  const Call h5t = call(5, 1, 640, 480, 5, 99, 2, 0);           // D = 100: the tail kernel
  const Call h5tn = call(3, 1, 333, 77, 5, 40, 1, 0);           // D = 41, narrow band: still the tail pitch
  const Call c5 = call(5, 1, 4096, 3072, 7, 255, 4, 0);         // C5: K = 7, pitch 128
  Call h7w = call(5, 1, 1000, 600, 7, 254, 4, 0);               // K = 7, levels 2 apart: pitch 192
  h7w.dinc = 2;
  const Call h7t = call(5, 1, 640, 480, 7, 99, 2, 0);           // K = 7, D = 100: the tail kernel
  add("horizontal_k5", {}, {c2, h5n, h5t, h5tn});
  add("horizontal_k7", {}, {c5, h7w, h7t});
  add("horizontal_k7_mfma7_off", {{"MVS_NCC_MFMA7", "0"}}, {c5, h7w, h7t, c2});
  add("mfma_off", {{"MVS_NCC_MFMA", "0"}}, {c2, h5n, h5t, c5, h7w, h7t});

  // ---- vertical and diagonal lists ----
  const Call g33 = call(3, 3, 128, 32, 5, 47, 1, 1);  // 3 x 3, 8-neighbour lists (the GPU test's shape)
  Call g33f = g33;
  g33f.bl = 1.0359f;
  const Call g55 = knn(5, 5, 256, 72, 127, 5, 1.0f);   // 5 x 5, 5 nearest, corner views included
  const Call g55t = knn(5, 5, 200, 69, 99, 5, 1.0359f);
  const Call c4 = knn(8, 4, 1920, 1080, 127, 5, 1.0f);  // C4
  const Call c4f = knn(8, 4, 256, 72, 127, 5, 1.0359f);
  const Call vo = call(1, 3, 100, 56, 5, 63, 0, 1);     // a column of cameras: no column shift, the 80-column pitch
  Call w2 = call(3, 2, 160, 40, 5, 63, 2, 1);          // small vertical shifts (bl 0.25) beside column shifts of
  Call w3 = call(4, 2, 160, 40, 5, 63, 3, 1);          // two and three views: the 128-column pitch
  w2.bl = w3.bl = 0.25f;
  Call w2t = w2;
  w2t.dmax = 49;
  const std::vector<Call> vert = {g33, g55, vo, w2, w3, w2t};
  add("grid3x3", {}, {g33});
  add("vertical_auto", {}, {g33f, g55, g55t, c4, vo, w2, w3, w2t});
  add("vertical_v0", {{"MVS_NCC_MFMA_V", "0"}}, {g33f, g55});
  add("vertical_v22", {{"MVS_NCC_MFMA_V", "22"}}, vert);
  add("vertical_v21", {{"MVS_NCC_MFMA_V", "21"}}, vert);
  add("vertical_v12", {{"MVS_NCC_MFMA_V", "12"}}, vert);
  add("vertical_v11", {{"MVS_NCC_MFMA_V", "11"}}, vert);
  add("vertical_v0_nb2", {{"MVS_NCC_MFMA_V", "0"}, {"MVS_NCC_NB", "2"}}, {g33f, g55});

  // ---- scalar kernels: every (waves, levels per wave, pitch, general_rows) variant that
  // tests/test_gpu_ncc_configs.py forces, plain and fused, each kernel instantiation once ----
  static const int variants[5][2] = {{8, 4}, {8, 2}, {4, 4}, {4, 2}, {4, 1}};
  static const int bands[6] = {64, 80, 96, 128, 192, 256};
  for (int general = 0; general < 2; general++) {
    // general_rows off: one level beside a horizontal neighbour a side (no shift range, so every pitch
    // from 64 up and the parity-specific kernel); on: a column of cameras at fractional vertical shifts
    std::vector<Call> cs;
    for (int K : {5, 7})
      for (const auto& v : variants)
        for (int bw : bands)
          for (int vol = 1; vol >= 0; vol--) {
            Call c = general ? call(1, 3, 100, 56, K, 4, 0, 1) : call(3, 1, 100, 40, K, 0, 1, 0);
            if (general) c.bl = 1.0359f;
            c.z0 = 1, c.z1 = 2, c.force_nw = v[0], c.force_dpw = v[1], c.force_bw = bw, c.vol = vol;
            c.force_general = general;
            cs.push_back(c);
          }
    if (!general)  // general_rows on a list the parity-specific kernel could take
      for (int K : {5, 7}) {
        Call c = call(3, 1, 100, 40, K, 0, 1, 0);
        c.z0 = 1, c.z1 = 2, c.force_nw = 8, c.force_dpw = 4, c.force_bw = 128, c.force_general = 1;
        cs.push_back(c);
      }
    add(general ? "forced_general_rows" : "forced_parity", {}, cs);
  }
  {  // the single-buffered K = 5 kernels (a forced pitch alone leaves waves and levels automatic): a
     // column of cameras whose vertical shift per level (bl) puts the bands, per pitch, between
     // "double-buffered misses 80 KB" and "single-buffered fits": 32-level chunks, then 16-level ones
    static const float bl4[6] = {1.13f, 1.13f, 0.9f, 0.65f, 0.26f, 0.17f}, bl2[6] = {2.3f, 2.3f, 2.3f, 1.6f, 0.9f, 0.4f};
    std::vector<Call> cs;
    for (const float* bls : {bl4, bl2})
      for (int b = 0; b < 6; b++)
        for (int vol = 1; vol >= 0; vol--) {
          Call c = call(1, 3, 100, 56, 5, 63, 0, 1);
          c.bl = bls[b], c.z0 = 1, c.z1 = 2, c.force_bw = bands[b], c.vol = vol;
          cs.push_back(c);
        }
    add("single_buffered", {}, cs);
  }
  {  // test_ncc_wta_range's and test_scalar_band_dma_forms' forced variants, over every view
    Call a = call(5, 1, 300, 50, 7, 63, 2, 0), b = call(3, 3, 200, 48, 5, 31, 1, 1);
    a.force_nw = 4, a.force_dpw = 2, a.force_bw = 192;
    b.force_nw = 8, b.force_dpw = 4, b.force_bw = 192;
    add("forced_runs", {}, {a, b});
    add("plane32_off", {{"MVS_NCC_PLANE32", "0"}, {"MVS_NCC_MFMA_V", "0"}}, {b, g33});
  }
  {  // a cost volume of one view; views without neighbours
    Call v5 = c2, v7 = c5, vg = g55, lone = call(1, 1, 100, 40, 5, 31, 0, 0), lone7 = lone;
    v5.vol = v7.vol = vg.vol = true;
    v5.z0 = 2, v5.z1 = 3, v7.z0 = 0, v7.z1 = 1, vg.z0 = 12, vg.z1 = 13;
    lone7.K = 7;
    Call lonev = lone;
    lonev.vol = true;
    add("volume_and_lone_views", {}, {v5, v7, vg, lone, lone7, lonev});
  }
  // the per-process knobs (levels per wave, waves)
  add("env_dpw2", {{"MVS_NCC_DPW", "2"}, {"MVS_NCC_MFMA", "0"}}, {c2, c5, g33});
  add("env_nw4", {{"MVS_NCC_NW", "4"}, {"MVS_NCC_MFMA", "0"}}, {c2, c5, g33});
  add("env_nw4_dpw1", {{"MVS_NCC_NW", "4"}, {"MVS_NCC_DPW", "1"}, {"MVS_NCC_MFMA", "0"}}, {c2, c5, g33});

  // ---- run forming ----
  add("run2", {{"MVS_NCC_RUN", "2"}}, {c2, g33});
  add("run2_scalar", {{"MVS_NCC_RUN", "2"}, {"MVS_NCC_MFMA", "0"}}, {c2, g33f});
  {  // runs broken by a change of form: 32 views (more than 8) of C4's array at fractional vertical
     // shifts, levels 2 apart (the corner and edge views' bands are taller)
    Call w = c4f;
    w.dinc = 2, w.dmax = 254;
    // a column of six cameras, levels 8 apart: the end views (a neighbour two rows away) fit only the
    // whole LDS, the inner ones 80 KB, all in the same form -- the cap breaks the run after view 0 and before view 5
    Call ends = knn(1, 6, 64, 64, 248, 2, 1.0f);
    ends.dinc = 8;
    add("runs_broken", {}, {w, ends});
    add("runs_broken_scalar", {{"MVS_NCC_MFMA", "0"}}, {w, ends});
  }

  // ---- size thresholds ----
  {
    Call big = call(5, 1, 16384, 16384, 5, 31, 4, 0);  // a view plane of 2 GB: plane32 off, no matrix-core form
    Call big7 = big;
    big7.K = 7;
    Call deep = call(5, 1, 640, 480, 5, 22399, 4, 0);  // 22400 levels x 4 neighbours: level offsets past 160 KB
    deep.z0 = 2, deep.z1 = 3;
    add("size_thresholds", {}, {big, big7, deep});
  }

  // ---- the timing probes, on the three shapes that have one ----
  add("mfma_dbg1", {{"MVS_NCC_MFMA_DBG", "1"}, {"MVS_NCC_MFMA_V", "12"}}, {c5, c2, g33, h5n, h7t});
  add("mfma_dbg2", {{"MVS_NCC_MFMA_DBG", "2"}, {"MVS_NCC_MFMA_V", "12"}}, {c5, c2, g33, h5n, h7t});

  // ---- errors ----
  {
    Call d = call(3, 1, 64, 16, 5, 65535, 1, 0);         // D = 65536 fused
    Call many = call(5, 5, 64, 16, 5, 15, 2, 2);         // 24 neighbours
    Call bad = call(3, 1, 64, 16, 5, 15, 1, 0);          // a view id out of range
    bad.bad_view = true;
    Call thin = call(3, 1, 1, 16, 5, 15, 1, 0);          // W < 2
    Call k6 = call(3, 1, 64, 16, 6, 15, 1, 0);           // K = 6
    Call far = call(3, 1, 640, 48, 5, 3000, 1, 0);       // levels 300 apart: no band holds a chunk's shifts
    far.dinc = 300;
    Call vol2 = call(3, 1, 64, 16, 5, 15, 1, 0);         // a volume of two views
    vol2.vol = true, vol2.z0 = 0, vol2.z1 = 2;
    Call none = call(3, 1, 64, 16, 5, 15, 1, 0);         // no views: no launches, no error
    none.z0 = 1, none.z1 = 1;
    add("errors", {}, {d, many, bad, thin, k6, far, vol2, none});
  }
  return out;
}

// the C4 list (bench.py's c4), the --time loop's call
inline Call c4_call() {
  Call c;
  c.aw = 8, c.ah = 4, c.W = 1920, c.H = 1080, c.K = 5, c.dmax = 127, c.knn = 5;
  return c;
}

}  // namespace plancase
