// Prints the decisions of the SLIC, superpixel-sweep, SAD and filter launch planners
// (csrc/launch_plan.cpp) for a named case, one canonical line per planned
// launch: tests/test_launch_plan_cpu.py compares them with
// tests/golden/launch_plans.txt.  Links only launch_plan.cpp; no GPU.
//   launch_plan_check --list        the case names
//   launch_plan_check CASE          the case's lines (its knobs set in this process's environment)
//   launch_plan_check --time [N]    host time per planner call on C4-sized inputs (SLIC: C2's), N (1000) calls each
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../cl_multiview_stereo_amd/csrc/launch_plan.h"
#include "launch_plan_cases.h"

using namespace mvs::plan;
using plancase::Call;

// one line per step of a SLIC plan, as launch_slic hands the step to its kernel, then the scratch size
static void print_slic_plan(FILE* out, int i, const SlicPlan& p) {
  const long W = p.W, H = p.H, S = p.S, mw = p.mw, mh = p.mh, G = p.G, cpl = p.cpl, ntx = p.ntx, nty = p.nty;
  const float xy_col[2] = {p.xy, p.col};
  for (const SlicStep& s : p.steps) {
    const unsigned gx = s.grid[0], gy = s.grid[1], gz = s.grid[2], b = s.block;
    const char* const labels = s.labels ? "labels" : "null";
    const char* const lb16 = s.lb16 ? "scratch" : "null";
    const char* const part = s.part ? "scratch" : "null";
    const char* const read = s.LT == 16 ? "scratch" : "labels";
    switch (s.kernel) {
      case kSlicInitCenters:
        plancase::print_slic(out, i, "k_init_centers", {}, gx, gy, gz, b, {{"lab", "lab"}, {"spixl", "spixl"}},
                             {{"W", W}, {"H", H}, {"S", S}, {"mw", mw}, {"mh", mh}});
        break;
      case kSlicEdge:
        plancase::print_slic(out, i, "k_edge", {}, gx, gy, gz, b, {{"lab", "lab"}, {"edge", "scratch"}},
                             {{"W", W}, {"H", H}});
        break;
      case kSlicEdgeStore:
        plancase::print_slic(out, i, "k_edge_store", {}, gx, gy, gz, b, {{"edge", "scratch"}, {"lab", "lab"}},
                             {{"n", (long)p.V * W * H}});
        break;
      case kSlicApplyEdge:
        plancase::print_slic(out, i, "k_apply_edge", {}, gx, gy, gz, b,
                             {{"lab", "lab"}, {"edge", "scratch"}, {"spixl", "spixl"}},
                             {{"W", W}, {"H", H}, {"mw", mw}, {"mh", mh}});
        break;
      case kSlicAssign:
        plancase::print_slic(out, i, "k_assign", {{"S3", s.S3}}, gx, gy, gz, b,
                             {{"lab", "lab"}, {"spixl", "spixl"}, {"labels", labels}, {"lb16", lb16}},
                             {{"W", W}, {"H", H}, {"S", S}, {"mw", mw}, {"mh", mh}}, xy_col);
        break;
      case kSlicAssignTiles9:
        plancase::print_slic(out, i, "k_assign_tiles", {{"S3", s.S3}}, gx, gy, gz, b,
                             {{"lab", "lab"}, {"spixl", "spixl"}, {"labels", labels}, {"part", part}},
                             {{"W", W}, {"H", H}, {"S", S}, {"mw", mw}, {"mh", mh}, {"G", G}, {"cpl", cpl},
                              {"ntx", ntx}, {"nty", nty}}, xy_col);
        break;
      case kSlicAssignTiles4:
        plancase::print_slic(out, i, "k_assign_tiles4", {{"S16", s.S16}}, gx, gy, gz, b,
                             {{"lab", "lab"}, {"spixl", "spixl"}, {"labels", labels}, {"part", part}},
                             {{"W", W}, {"H", H}, {"mw", mw}, {"mh", mh}, {"G", G}, {"cpl", cpl}, {"ntx", ntx}},
                             xy_col);
        break;
      case kSlicUpdateFinalize:
        plancase::print_slic(out, i, "k_update_finalize", {{"CPL", s.CPL}}, gx, gy, gz, b,
                             {{"part", "scratch"}, {"spixl", "spixl"}},
                             {{"mw", mw}, {"mh", mh}, {"S", S}, {"G", G}, {"cpl", cpl}, {"ntx", ntx}, {"nty", nty}});
        break;
      case kSlicUpdateWalk:
      case kSlicUpdate:
        plancase::print_slic(out, i, s.kernel == kSlicUpdate ? "k_update" : "k_update_walk",
                             {{"UT", s.UT}, {"LT", s.LT}}, gx, gy, gz, b,
                             {{"lab", "lab"}, {"labels", read}, {"spixl", "spixl"}},
                             {{"W", W}, {"H", H}, {"S", S}, {"mw", mw}, {"mh", mh}, {"G", G}, {"cpl", cpl}});
        break;
      case kSlicSuppress:
        plancase::print_slic(out, i, "k_suppress", {}, gx, gy, gz, b,
                             {{"in", s.to_scratch ? "labels" : "scratch"}, {"out", s.to_scratch ? "scratch" : "labels"}},
                             {{"W", W}, {"H", H}});
        break;
    }
  }
  plancase::print_slic_scratch(out, i, p.scratch_bytes);
}

// plans the call as its launcher does (every knob read per call); out: where the lines go, or null
static void run_call(int i, const Call& c, const plancase::Inputs& in, FILE* out) {
  const Tuning t = plan_tuning();
  const int V = c.V ? c.V : in.V, D = (int)in.levels.size();
  const int z1 = c.z1 < 0 ? V : c.z1;
  if (c.kind == plancase::kSweep) {
    const SpixlSweepPlan p = plan_sweep_spixl(t, V, c.W, c.H, c.S, D, in.levels.data(), in.vs.data(), in.sn.data(),
                                              c.aw, c.z0, z1, c.allow_relayout);
    if (!out) return;
    if (p.err) return plancase::print_error(out, i, -1, p.err);
    if (!p.launch) return plancase::print_none(out, i);
    std::vector<std::array<int, 3>> rel;
    for (const SpixlRelayout& r : p.relayouts) rel.push_back({r.view, r.kind, r.slot});
    plancase::print_sweep(out, i, p.form, p.lps, p.wps, p.grid_x, p.grid_y, p.mw, p.mh, p.tstride, p.units,
                          p.slot.data(), p.slot.size(), rel, p.last);
  } else if (c.kind == plancase::kSad) {
    for (int z = c.z0; z < z1; z++) {
      const SadPlan p = plan_sad(t, V, c.W, c.H, D, in.levels.data(), in.vs.data(), in.sn.data(), c.aw, c.bl, z);
      if (!out) continue;
      if (!p.err.empty()) return plancase::print_error(out, i, z, p.err.c_str());  // the launcher stops here
      if (p.band)
        plancase::print_sad_band(out, i, z, p.TH, p.PPW, p.AFF, p.BWT, (const int32_t*)&p.args, p.grid_x, p.lds,
                                 p.table.data(), p.table.size());
      else
        plancase::print_sad_gather(out, i, z, p.grid_x, p.grid_y);
    }
  } else if (c.kind == plancase::kSlic) {
    const SlicPlan p = plan_slic(t, V, c.W, c.H, c.S, c.no_iter, c.edge, c.search, c.conn);
    if (out) print_slic_plan(out, i, p);
  } else {
    const FilterPlan p = plan_remove_incons(t, V, c.W, c.H, c.aw, c.z0, z1, c.ya, c.yb < 0 ? c.H : c.yb, c.band);
    if (!out) return;
    if (p.kernel == kFilterNone) return plancase::print_none(out, i);
    static const char* const names[] = {"none", "sel8", "px16_8", "q", "px32", "sel64", "plain"};
    plancase::print_filter(out, i, names[p.kernel], p.FB, p.NS, p.ROWB, p.RM, p.inb, p.grid, p.block, p.PP,
                           p.proj_off);
  }
}

int main(int argc, char** argv) {
  static_assert(sizeof(mvs::SadArgs) == 11 * 4, "print_sad_band reads SadArgs as 11 ints");
  if (argc < 2) return fprintf(stderr, "usage: %s --list | --time [N] | CASE\n", argv[0]), 2;
  const std::vector<plancase::Case> cases = plancase::cases();
  if (!strcmp(argv[1], "--list")) {
    for (const auto& c : cases) printf("%s\n", c.name.c_str());
    return 0;
  }
  if (!strcmp(argv[1], "--time")) {
    const int reps = argc > 2 ? atoi(argv[2]) : 1000;
    static const char* const what[] = {"sweep", "sad (one view)", "filter"};
    for (const Call& c : plancase::c4_calls()) {
      const plancase::Inputs in = plancase::make_inputs(c);
      const auto t0 = std::chrono::steady_clock::now();
      for (int i = 0; i < reps; i++) run_call(0, c, in, nullptr);
      const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
      printf("c4 %s: %d calls, %.2f us per call\n", what[c.kind], reps, us / reps);
    }
    const Call c = plancase::c2_slic_call();
    const plancase::Inputs in = plancase::make_inputs(c);
    const auto t0 = std::chrono::steady_clock::now();
    for (int i = 0; i < reps; i++) run_call(0, c, in, nullptr);
    const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    printf("c2 slic (S = 32, 5 iterations): %d calls, %.2f us per call\n", reps, us / reps);
    return 0;
  }
  for (const auto& cs : cases) {
    if (cs.name != argv[1]) continue;
    for (const auto& e : cs.env) setenv(e.first, e.second, 1);
    for (size_t i = 0; i < cs.calls.size(); i++) run_call((int)i, cs.calls[i], plancase::make_inputs(cs.calls[i]), stdout);
    return 0;
  }
  return fprintf(stderr, "unknown case %s\n", argv[1]), 2;
}
