// Prints the decisions of the superpixel-sweep, SAD and filter launch planners
// (csrc/launch_plan.cpp) for a named case, one canonical line per planned
// launch: tests/test_launch_plan_cpu.py compares them with
// tests/golden/launch_plans.txt.  Links only launch_plan.cpp; no GPU.
//   launch_plan_check --list        the case names
//   launch_plan_check CASE          the case's lines (its knobs set in this process's environment)
//   launch_plan_check --time [N]    host time per planner call on C4-sized inputs, N (1000) calls each
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../cl_multiview_stereo_amd/csrc/launch_plan.h"
#include "launch_plan_cases.h"

using namespace mvs::plan;
using plancase::Call;

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
