// plan_sgm_diag (csrc/launch_plan.cpp) on the CPU: walks image sizes and level
// counts on and around every threshold of the planner over the four diagonal
// paths, checks each plan's invariants and prints one line per case.  For
// images up to 65 x 65 it enumerates the plan's own map (workgroup, lane, row)
// -> (x, y), or (line, element) -> (x, y) in the lanes form, with the functions
// the kernels use (launch_plan.h), in the order the kernels walk: every pixel
// is visited exactly once, and each visit's predecessor (x - dx, y - dy) is the
// pixel the same lane or line visited one step earlier, or lies outside the
// image on the lane's or line's first visit.  Links only the planner; built
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

static const int kDx[4] = {1, -1, -1, 1}, kDy[4] = {1, -1, 1, -1};  // paths 4..7

// one visit of a walker (a lane of the sheared form, a line of the lanes form); px, py: its last visit (-1: none)
static bool visit(int W, int H, int dx, int dy, int x, int y, int& px, int& py, std::vector<int>& seen) {
  if (x < 0 || x >= W || y < 0 || y >= H) return false;
  seen[(size_t)y * W + x]++;
  const int qx = x - dx, qy = y - dy;
  const bool q_in = qx >= 0 && qx < W && qy >= 0 && qy < H;
  const bool ok = px < 0 ? !q_in : (q_in && qx == px && qy == py);
  px = x;
  py = y;
  return ok;
}

static void check(int W, int H, int D, int path) {
  const SgmPlan p = plan_sgm_diag(W, H, D, path);
  if (p.err) {
    std::printf("W=%d H=%d D=%d path=%d error: %s\n", W, H, D, path, p.err);
    g_bad++;
    return;
  }
  std::printf("W=%d H=%d D=%d path=%d form=%s lpl=%d waves=%d sx=%d rev=%d lines=%d sstride=%d grid=%u block=%u lds=%zu\n",
              W, H, D, path, p.form == kSgmSheared ? "sheared" : "lanes", p.lpl, p.waves, p.sx, (int)p.rev, p.lines,
              p.sstride, p.grid, p.block, p.lds);
  const int dx = kDx[path - 4], dy = kDy[path - 4];
  CHECK(p.form == kSgmSheared || p.form == kSgmLanes);
  CHECK(p.sx == dx * dy && p.rev == (dy < 0));
  CHECK(p.lines == W + H - 1 && p.sstride == W + p.sx);
  CHECK(p.grid > 0 && p.grid <= (unsigned)INT_MAX);
  CHECK(p.block > 0 && p.block <= 1024 && p.block == 64u * (unsigned)p.waves && p.waves >= 1 && p.waves <= 16);
  if (p.form == kSgmSheared) {
    CHECK(D <= kSgmColumnsMaxD && p.lpl == kSgmColumnsLpw);
    CHECK(p.waves * p.lpl >= D && (p.waves - 1) * p.lpl < D);
    // k_sgm_diag<512> up to 8 waves, <1024> above: float ex[2][NT / 64][3][64]
    CHECK(p.lds == sizeof(float) * 2 * (p.waves <= 8 ? 8 : 16) * 3 * 64 && p.lds <= 64u * 1024u);
    CHECK(p.grid == (unsigned)((W + H - 1 + 63) / 64));
  } else {
    CHECK(D > kSgmColumnsMaxD && (p.lpl == 8 || p.lpl == 16));
    CHECK(64 * p.waves * p.lpl >= D);
    CHECK(p.waves == 1 ? (p.lpl == 8 || 64 * 8 < D) : 64 * (p.waves - 1) * p.lpl < D);
    // k_sgm_lanes<16, false, true, true>: float ex[2][16][3]
    CHECK(p.lds == (p.waves > 1 ? sizeof(float) * 2 * 16 * 3 : 0));
    CHECK(p.grid == (unsigned)(W + H - 1));
  }
  if (W > 65 || H > 65) {
    // the row ranges and the lines stay inside the image at any size
    if (p.form == kSgmSheared) {
      for (unsigned g = 0; g < p.grid; g++) {
        const int ylo = sgm_diag_ylo((int)g, W, H, p.sx), yhi = sgm_diag_yhi((int)g, W, H, p.sx);
        CHECK(0 <= ylo && ylo <= yhi && yhi < H);
      }
    } else {
      for (int l = 0; l < p.lines; l++) {
        const SgmDiagLine ln = sgm_diag_line(W, H, p.sx, l);
        CHECK(ln.n >= 1 && ln.first >= 0 && (long)ln.first + (long)(ln.n - 1) * p.sstride < (long)W * H);
      }
    }
    return;
  }
  std::vector<int> seen((size_t)W * H, 0);
  bool chain = true;
  if (p.form == kSgmSheared) {
    for (unsigned g = 0; g < p.grid; g++) {
      const int ylo = sgm_diag_ylo((int)g, W, H, p.sx), yhi = sgm_diag_yhi((int)g, W, H, p.sx);
      CHECK(0 <= ylo && ylo <= yhi && yhi < H);
      for (int lane = 0; lane < 64; lane++) {
        const int x0 = sgm_diag_x0((int)g, lane, H, p.sx);
        int px = -1, py = -1;
        bool left = false;  // the lane was live and is not any more: it must stay out
        for (int i = 0; i <= yhi - ylo; i++) {
          const int y = p.rev ? yhi - i : ylo + i, x = x0 + p.sx * y;
          const bool in = x >= 0 && x < W;
          if (in) {
            chain = chain && !left && visit(W, H, dx, dy, x, y, px, py, seen);
          } else if (px >= 0) {
            left = true;
          }
        }
        // no live row of the lane lies outside the rows walked
        for (int y = 0; y < H; y++) {
          const int x = x0 + p.sx * y;
          if (x >= 0 && x < W) CHECK(y >= ylo && y <= yhi);
        }
      }
    }
  } else {
    for (int l = 0; l < p.lines; l++) {
      const SgmDiagLine ln = sgm_diag_line(W, H, p.sx, l);
      CHECK(ln.n >= 1 && ln.n <= (W < H ? W : H) && ln.first >= 0 && ln.first < W * H);
      int px = -1, py = -1;
      for (int i = 0; i < ln.n; i++) {
        const int j = p.rev ? ln.n - 1 - i : i;
        const int o = ln.first + j * p.sstride;
        CHECK(o >= 0 && o < W * H);
        // (a line of one pixel has stride W - 1 = 0 at W = 1: the stride is never applied)
        chain = chain && visit(W, H, dx, dy, o % W, o / W, px, py, seen);
      }
      // the line ends at the image's edge: the pixel after its last lies outside
      const int ax = px + dx, ay = py + dy;
      CHECK(ax < 0 || ax >= W || ay < 0 || ay >= H);
    }
  }
  bool once = true;
  for (int v : seen) once = once && v == 1;
  CHECK(once);
  CHECK(chain);
}

int main() {
  const int sizes[] = {1, 2, 3, 63, 64, 65, 300, 1920};
  const int levels[] = {1, 16, 17, 128, 256, 257, 1100};
  for (int W : sizes)
    for (int H : sizes)
      for (int D : levels)
        for (int path = 4; path < 8; path++) check(W, H, D, path);
  // the limits: the largest level count, one more, the paths next to 4..7, a zero dimension
  {
    const int W = 64, H = 3, path = 4;
    int D = kSgmMaxD;
    check(W, H, D, 4);
    check(W, H, D, 7);
    D = kSgmMaxD + 1;
    CHECK(plan_sgm_diag(W, H, D, path).err != nullptr);
    D = 1;
    CHECK(plan_sgm_diag(W, H, D, 3).err != nullptr && plan_sgm_diag(W, H, D, 8).err != nullptr);
    CHECK(plan_sgm_diag(0, H, D, path).err != nullptr && plan_sgm_diag(W, 0, D, path).err != nullptr &&
          plan_sgm_diag(W, H, 0, path).err != nullptr);
  }
  if (g_bad) std::printf("%d checks failed\n", g_bad);
  return g_bad ? 1 : 0;
}
