// plan_sgm_batch (csrc/launch_plan.cpp) on the CPU: the argument rules of
// mvs_sgm8_batch_d and the choice of the 16-byte-pieces form, against brute
// force.  Walks N in {1, 2, 3, 5, 65535, 65536, 0, -1}, strides
// D H W + {-1, 0, 1, 2, 3, 4} for each buffer and base offsets of 0..3 floats
// for each buffer; per case the planner's error equals the rules stated in
// include/mvs.h, vec_ok equals "vol and agg are equal mod 16 bytes in every
// element" computed element by element over i < min(N, 8), and the overlap
// rule equals an interval test on the spans.  Overlapping, nested and abutting
// span pairs follow, then the largest shape (W H = 2^27, D = 16384, N = 65535),
// whose spans must be formed without overflow.  Links only the planner; built
// with the address and undefined-behaviour sanitizers (Makefile: sgmplancheck).
// Prints one line per case.  Exit status 0: every check held.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../cl_multiview_stereo_amd/csrc/launch_plan.h"

using namespace mvs::plan;

static int g_bad = 0;

#define CHECK(cond)                                                   \
  do {                                                                \
    if (!(cond)) {                                                    \
      std::printf("  FAILED: %s (line %d)\n", #cond, __LINE__);       \
      g_bad++;                                                        \
    }                                                                 \
  } while (0)

typedef unsigned __int128 u128;

// the spans of include/mvs.h in bytes, and whether they share a byte
static bool spans_overlap(int D, int H, int W, int N, uint64_t va, uint64_t vs, uint64_t aa, uint64_t as) {
  const u128 dhw = (u128)D * (u128)H * (u128)W;
  const u128 v0 = va, v1 = v0 + 4 * ((u128)(N - 1) * vs + dhw);
  const u128 a0 = aa, a1 = a0 + 4 * ((u128)(N - 1) * as + dhw);
  return !(v1 <= a0 || a1 <= v0);
}

// one case against the rules; returns the plan
static SgmBatchPlan check(int W, int H, int D, int N, uint64_t va, uint64_t vs, uint64_t aa, uint64_t as) {
  const SgmBatchPlan p = plan_sgm_batch(kSgmF32, W, H, D, N, (uintptr_t)va, (size_t)vs, (uintptr_t)aa, (size_t)as);
  std::printf("W=%d H=%d D=%d N=%d vol=%llu+%llu agg=%llu+%llu -> %s grid_y=%u vec_ok=%d\n", W, H, D, N,
              (unsigned long long)va, (unsigned long long)vs, (unsigned long long)aa, (unsigned long long)as,
              p.err ? p.err : "ok", p.grid_y, (int)p.vec_ok);
  const uint64_t dhw = (uint64_t)D * (uint64_t)H * (uint64_t)W;
  const bool bad_n = N < 1 || N > 65535, bad_stride = vs < dhw || as < dhw;
  const bool want_err = bad_n || bad_stride || spans_overlap(D, H, W, N, va, vs, aa, as);
  CHECK((p.err != nullptr) == want_err);
  if (p.err) {
    // the message says which rule (the span rule is tested only for a valid N and valid strides)
    if (bad_n) CHECK(std::strstr(p.err, "N must be") != nullptr);
    else if (bad_stride) CHECK(std::strstr(p.err, "stride") != nullptr);
    else CHECK(std::strstr(p.err, "overlap") != nullptr);
    CHECK(p.grid_y == 0 && !p.vec_ok);
    return p;
  }
  CHECK(p.grid_y == (unsigned)N && p.grid_y <= 65535u);
  bool congruent = true;  // element by element
  for (int i = 0; i < (N < 8 ? N : 8); i++)
    congruent = congruent && ((va + 4 * (uint64_t)i * vs) & 15) == ((aa + 4 * (uint64_t)i * as) & 15);
  CHECK(p.vec_ok == congruent);
  return p;
}

int main() {
  const int W = 67, H = 5, D = 66;
  const uint64_t dhw = (uint64_t)W * H * D;
  const int ns[] = {1, 2, 3, 5, 65535, 65536, 0, -1};
  const int ds[] = {-1, 0, 1, 2, 3, 4};
  // two 16-byte-aligned bases far enough apart for 65535 elements of the widest stride
  const uint64_t vbase = 1ull << 20, abase = 1ull << 40;
  int vec = 0, scalar = 0;
  for (int N : ns)
    for (int dv : ds)
      for (int da : ds)
        for (int ov = 0; ov < 4; ov++)
          for (int oa = 0; oa < 4; oa++) {
            const SgmBatchPlan p = check(W, H, D, N, vbase + 4 * ov, dhw + dv, abase + 4 * oa, dhw + da);
            if (!p.err) (p.vec_ok ? vec : scalar)++;
          }
  CHECK(vec > 0 && scalar > 0);
  // span pairs: N = 2, tight strides, vol = [v, v + 2 dhw)
  {
    const int N = 2;
    const uint64_t v = 1ull << 20, f = 4;  // bytes per float
    CHECK(check(W, H, D, N, v, dhw, v + f * dhw, dhw).err != nullptr);          // agg = vol + D H W: inside vol's span
    CHECK(check(W, H, D, N, v, dhw, v + f * (2 * dhw - 1), dhw).err != nullptr);  // one float shared
    CHECK(check(W, H, D, N, v, dhw, v + f * 2 * dhw, dhw).err == nullptr);      // abutting behind
    CHECK(check(W, H, D, N, v, dhw, v - f * 2 * dhw, dhw).err == nullptr);      // abutting in front
    CHECK(check(W, H, D, N, v, dhw, v - f * (2 * dhw - 1), dhw).err != nullptr);
    CHECK(check(W, H, D, N, v, dhw, v, dhw).err != nullptr);                    // agg == vol
    // interleaved: vol elements at even slots, agg at odd ones; disjoint element by element, refused by the spans
    CHECK(check(W, H, D, N, v, 2 * dhw, v + f * dhw, 2 * dhw).err != nullptr);
    // the gap of a padded vol counts: agg inside the gap
    CHECK(check(W, H, D, 1, v, 3 * dhw, v + f * dhw, dhw).err == nullptr);  // (N = 1: no gap, the stride is not used)
    CHECK(check(W, H, D, N, v, 3 * dhw, v + f * dhw, dhw).err != nullptr);
    // with one element the spans are the volumes themselves
    CHECK(check(W, H, D, 1, v, dhw, v + f * dhw, dhw).err == nullptr);
    CHECK(check(W, H, D, 1, v, dhw, v + f * (dhw - 1), dhw).err != nullptr);
  }
  // the largest shape: (N - 1) stride + D H W = 65535 * 2^41 floats, 2^59 bytes
  {
    const int W2 = 1 << 14, H2 = 1 << 13, D2 = 16384, N = 65535;
    const uint64_t big = (uint64_t)W2 * H2 * D2;  // 2^41
    CHECK(big == 1ull << 41);
    const uint64_t span = 4 * ((uint64_t)(N - 1) * big + big);  // bytes, below 2^59
    CHECK(span == 65535ull << 43);
    CHECK(check(W2, H2, D2, N, 4096, big, 4096 + span, big).err == nullptr);      // abutting
    CHECK(check(W2, H2, D2, N, 4096, big, 4096 + span - 4, big).err != nullptr);  // one float shared
    CHECK(check(W2, H2, D2, N, 4096 + span, big, 4096, big).err == nullptr);
    // strides whose span does not fit 64 bits: the far span still does not reach the near one's start
    const uint64_t huge = ~0ull / 8;
    CHECK(check(W2, H2, D2, N, 1ull << 62, huge, 4096, big).err == nullptr);
    CHECK(check(W2, H2, D2, N, 4096, huge, 1ull << 62, big).err != nullptr);
    // one more pixel, one more level
    CHECK(plan_sgm_batch(kSgmF32, W2 + 1, H2, D2, N, 4096, 2 * big, 4096 + 16 * span, 2 * big).err != nullptr);
    CHECK(plan_sgm_batch(kSgmF32, W2, H2, D2 + 1, N, 4096, 2 * big, 4096 + 16 * span, 2 * big).err != nullptr);
    CHECK(plan_sgm_batch(kSgmF32, 0, H2, D2, N, 4096, big, 4096 + span, big).err != nullptr);
  }
  if (g_bad) std::printf("%d checks failed\n", g_bad);
  return g_bad ? 1 : 0;
}
