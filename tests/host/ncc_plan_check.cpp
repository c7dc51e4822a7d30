// Prints the NCC launch planner's decisions (csrc/ncc_plan.cpp) for a named
// case, one canonical line per launch: tests/test_ncc_plan_cpu.py compares
// them with tests/golden/ncc_launch_plans.txt.  Links only ncc_plan.cpp; no GPU.
//   ncc_plan_check --list        the case names
//   ncc_plan_check CASE          the case's lines (its knobs set in this process's environment)
//   ncc_plan_check --time [N]    host time of N (100) planner calls on the C4 list
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../cl_multiview_stereo_amd/csrc/ncc_plan.h"
#include "ncc_plan_cases.h"

using namespace mvs::ncc;

static bool run_call(const plancase::Call& c, const plancase::Inputs& in, std::vector<NccLaunch>& ls, std::string& err) {
  const NccTuning t = ncc_tuning(c.force_nw, c.force_dpw, c.force_bw, c.force_general);
  return plan_ncc_launches(t, in.V, c.W, c.H, c.K, (int)in.levels.size(), in.levels.data(), in.vs.data(),
                           in.sn.data(), c.aw, c.bl, c.z0, c.z1 < 0 ? in.V : c.z1, c.vol, ls, err);
}

int main(int argc, char** argv) {
  static_assert(sizeof(NccArgs) == 164 * 4, "print_launch reads NccArgs as 164 ints");
  if (argc < 2) return fprintf(stderr, "usage: %s --list | --time [N] | CASE\n", argv[0]), 2;
  const std::vector<plancase::Case> cases = plancase::cases();
  if (!strcmp(argv[1], "--list")) {
    for (const auto& c : cases) printf("%s\n", c.name.c_str());
    return 0;
  }
  if (!strcmp(argv[1], "--time")) {
    const int reps = argc > 2 ? atoi(argv[2]) : 100;
    const plancase::Call c = plancase::c4_call();
    const plancase::Inputs in = plancase::make_inputs(c);
    std::vector<NccLaunch> ls;
    std::string err;
    const auto t0 = std::chrono::steady_clock::now();
    size_t launches = 0;
    for (int i = 0; i < reps; i++) {
      if (!run_call(c, in, ls, err)) return fprintf(stderr, "error: %s\n", err.c_str()), 1;
      launches += ls.size();
    }
    const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    printf("c4 list: %d calls, %zu launches, %.1f us per call\n", reps, launches, us / reps);
    return 0;
  }
  for (const auto& cs : cases) {
    if (cs.name != argv[1]) continue;
    for (const auto& e : cs.env) setenv(e.first, e.second, 1);
    for (size_t i = 0; i < cs.calls.size(); i++) {
      const plancase::Call& c = cs.calls[i];
      const plancase::Inputs in = plancase::make_inputs(c);
      std::vector<NccLaunch> ls;
      std::string err;
      if (!run_call(c, in, ls, err)) {
        plancase::print_error(stdout, (int)i, err.c_str());
        continue;
      }
      for (const NccLaunch& L : ls) {
        const int sc[7] = {L.K, L.DPW, L.NW, L.BW, L.PAR, L.NB, L.FUSE};
        const int mc[7] = {L.K, L.BW, L.TAIL, L.VERT, L.NDB, L.NB, L.DBG};
        plancase::print_launch(stdout, (int)i, L.mfma, L.mfma ? mc : sc, L.first, (const int32_t*)&L.args,
                               L.table.size(), plancase::fnv1a(L.table.data(), L.table.size()), L.tmax, L.lds,
                               L.last);
      }
    }
    return 0;
  }
  return fprintf(stderr, "unknown case %s\n", argv[1]), 2;
}
