// plan_sgm (csrc/launch_plan.cpp) on the CPU: walks image sizes and level
// counts on and around every threshold of the planner, checks each plan's
// invariants and prints one line per case.  Links only the planner; built
// with the address and undefined-behaviour sanitizers (Makefile: sgmplancheck).
// Exit status 0: every invariant held.
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../cl_multiview_stereo_amd/csrc/launch_plan.h"

using namespace mvs::plan;

static int g_bad = 0;

#define CHECK(cond)                                                                        \
  do {                                                                                     \
    if (!(cond)) {                                                                         \
      std::printf("  FAILED: %s (W=%d H=%d D=%d path=%d)\n", #cond, W, H, D, path);        \
      g_bad++;                                                                             \
    }                                                                                      \
  } while (0)

static void check(int W, int H, int D, int path) {
  const SgmPlan p = plan_sgm(W, H, D, path);
  if (p.err) {
    std::printf("W=%d H=%d D=%d path=%d error: %s\n", W, H, D, path, p.err);
    g_bad++;
    return;
  }
  std::printf("W=%d H=%d D=%d path=%d form=%s lpl=%d waves=%d vec=%d n=%d lines=%d sstride=%d lstride=%d rev=%d "
              "grid=%u block=%u lds=%zu\n",
              W, H, D, path, p.form == kSgmColumns ? "columns" : "lanes", p.lpl, p.waves, (int)p.vec, p.n, p.lines,
              p.sstride, p.lstride, (int)p.rev, p.grid, p.block, p.lds);
  const bool vertical = path >= 2;
  CHECK(p.form == kSgmLanes || p.form == kSgmColumns);
  CHECK(p.rev == (bool)(path & 1));
  CHECK(p.n == (vertical ? H : W) && p.lines == (vertical ? W : H));
  CHECK(p.sstride == (vertical ? W : 1) && p.lstride == (vertical ? 1 : W));
  CHECK(p.grid > 0 && p.grid <= (unsigned)INT_MAX);
  CHECK(p.block > 0 && p.block <= 1024 && p.block == 64u * (unsigned)p.waves && p.waves >= 1 && p.waves <= 16);
  CHECK(p.lds <= 160u * 1024u);
  // every line (row or column) exactly once
  std::vector<int> seen((size_t)p.lines, 0);
  const unsigned per = p.form == kSgmColumns ? 64u : 1u;  // lines per workgroup
  for (unsigned b = 0; b < p.grid; b++)
    for (unsigned l = 0; l < per; l++) {
      const unsigned line = b * per + l;
      if (p.form == kSgmLanes) CHECK(line < (unsigned)p.lines);  // (the columns form masks x >= W)
      if (line < (unsigned)p.lines) seen[line]++;
    }
  bool once = true;
  for (int v : seen) once = once && v == 1;
  CHECK(once);
  // the last element of the last line stays inside a plane
  CHECK((long)(p.lines - 1) * p.lstride + (long)(p.n - 1) * p.sstride == (long)W * H - 1);
  // levels
  if (p.form == kSgmColumns) {
    CHECK(vertical && D <= kSgmColumnsMaxD && p.lpl == kSgmColumnsLpw);
    CHECK(p.waves * p.lpl >= D && (p.waves - 1) * p.lpl < D);
    CHECK(p.lds == sizeof(float) * 2 * (p.waves <= 8 ? 8 : 16) * 3 * 64);
    CHECK(!p.vec);
  } else {
    CHECK(p.lpl == 1 || p.lpl == 2 || p.lpl == 4 || p.lpl == 8 || p.lpl == 16);
    CHECK(64 * p.waves * p.lpl >= D);
    CHECK(p.waves == 1 ? (p.lpl == 1 || 64 * (p.lpl / 2) < D) : 64 * (p.waves - 1) * p.lpl < D);
    CHECK(p.lds == (p.waves > 1 ? sizeof(float) * 2 * 16 * 3 : 0));
    CHECK(!p.vec || (p.sstride == 1 && p.waves == 1));  // 16-byte pieces: contiguous lines, the one-wave kernel
    CHECK(!vertical || D > kSgmColumnsMaxD);
  }
}

int main() {
  const int sizes[] = {1, 2, 3, 63, 64, 65, 300, 1920, 4096};
  const int levels[] = {1, 2, 63, 64, 65, 128, 256, 257, 1100};
  for (int W : sizes)
    for (int H : sizes)
      for (int D : levels)
        for (int path = 0; path < 4; path++) check(W, H, D, path);
  // the limits: the largest level count, one more, a bad path
  {
    const int W = 64, H = 3, path = 0;
    int D = kSgmMaxD;
    check(W, H, D, 0);
    check(W, H, D, 2);
    D = kSgmMaxD + 1;
    CHECK(plan_sgm(W, H, D, path).err != nullptr);
    D = 1;
    CHECK(plan_sgm(W, H, D, 4).err != nullptr && plan_sgm(W, H, D, -1).err != nullptr);
    CHECK(plan_sgm(0, H, D, path).err != nullptr && plan_sgm(W, 0, D, path).err != nullptr &&
          plan_sgm(W, H, 0, path).err != nullptr);
  }
  if (g_bad) std::printf("%d checks failed\n", g_bad);
  return g_bad ? 1 : 0;
}
