// plan_sgm_batch at kSgmU16, sgm_piece_vec_ok and the piece phase (csrc/launch_plan.{h,cpp}) on the CPU: the argument
// rules of mvs_sgm8_u16_batch_d in 2-byte elements, against brute force.
//  1. N in {1, 2, 3, 5, 65535, 65536, 0, -1}, strides D H W + {-1, 0, 1, 7, 8, 9} for each buffer and base offsets
//     of {0, 1, 3, 7} elements for each buffer: the planner's error equals the rules of include/mvs.h, vec_ok equals
//     "vol and agg are equal mod 16 bytes in every element" computed element by element over i < min(N, 16), and the
//     overlap rule equals an interval test on the spans in bytes.
//  2. Odd addresses, the level limit (256 accepted, 257 unsupported), span pairs (nested, interleaved, abutting).
//  3. Element strides near 2^41 with N = 65535: the spans must be formed without overflow.
//  4. The phase: for every line address mod 16 bytes (even addresses), every line length n in 1..40 and every
//     pixel x, the piece of pixel x starts at a multiple of 16 bytes, holds x at element sgm_piece_elem, and
//     sgm_piece_inside equals "all eight pixels of that piece lie in [0, n)"; the pieces inside a line are
//     disjoint and every pixel is either in exactly one of them or handled singly.
//  5. The same for the general piece arithmetic (sgm_piece_phase, sgm_piece_elem, sgm_piece_inside) at both piece
//     sizes, 4 float32 and 8 uint16 pixels, and sgm_piece_vec_ok against its rule.
// Links only the planner; built with the address and undefined-behaviour sanitizers (Makefile: sgmplancheck).
// Prints one line per case of 1 to 4.  Exit status 0: every check held.
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

static bool spans_overlap(int D, int H, int W, int N, uint64_t va, uint64_t vs, uint64_t aa, uint64_t as) {
  const u128 dhw = (u128)D * (u128)H * (u128)W;
  const u128 v0 = va, v1 = v0 + 2 * ((u128)(N - 1) * vs + dhw);
  const u128 a0 = aa, a1 = a0 + 2 * ((u128)(N - 1) * as + dhw);
  return !(v1 <= a0 || a1 <= v0);
}

static SgmBatchPlan check(int W, int H, int D, int N, uint64_t va, uint64_t vs, uint64_t aa, uint64_t as) {
  const SgmBatchPlan p = plan_sgm_batch(kSgmU16, W, H, D, N, (uintptr_t)va, (size_t)vs, (uintptr_t)aa, (size_t)as);
  std::printf("W=%d H=%d D=%d N=%d vol=%llu+%llu agg=%llu+%llu -> %s grid_y=%u vec_ok=%d\n", W, H, D, N,
              (unsigned long long)va, (unsigned long long)vs, (unsigned long long)aa, (unsigned long long)as,
              p.err ? p.err : "ok", p.grid_y, (int)p.vec_ok);
  const uint64_t dhw = (uint64_t)D * (uint64_t)H * (uint64_t)W;
  const bool many = D > 256, bad_n = N < 1 || N > 65535, odd = ((va | aa) & 1) != 0;
  const bool bad_stride = vs < dhw || as < dhw;
  const bool want_err = many || bad_n || odd || bad_stride || spans_overlap(D, H, W, N, va, vs, aa, as);
  CHECK((p.err != nullptr) == want_err);
  CHECK(p.unsupported == many);
  if (p.err) {
    if (many) CHECK(std::strstr(p.err, "256 levels") != nullptr);
    else if (bad_n) CHECK(std::strstr(p.err, "N must be") != nullptr);
    else if (odd) CHECK(std::strstr(p.err, "2-byte aligned") != nullptr);
    else if (bad_stride) CHECK(std::strstr(p.err, "stride") != nullptr);
    else CHECK(std::strstr(p.err, "overlap") != nullptr);
    CHECK(p.grid_y == 0 && !p.vec_ok);
    return p;
  }
  CHECK(p.grid_y == (unsigned)N && p.grid_y <= 65535u);
  bool congruent = true;  // element by element
  for (int i = 0; i < (N < 16 ? N : 16); i++)
    congruent = congruent && ((va + 2 * (uint64_t)i * vs) & 15) == ((aa + 2 * (uint64_t)i * as) & 15);
  CHECK(p.vec_ok == congruent);
  CHECK(p.vec_ok == sgm_piece_vec_ok(kSgm16Piece, N, (uintptr_t)va, (size_t)vs, (uintptr_t)aa, (size_t)as));
  return p;
}

int main() {
  const int W = 67, H = 5, D = 66;
  const uint64_t dhw = (uint64_t)W * H * D;
  // 1.
  {
    const int ns[] = {1, 2, 3, 5, 65535, 65536, 0, -1};
    const int ds[] = {-1, 0, 1, 7, 8, 9};
    const int os[] = {0, 1, 3, 7};
    const uint64_t vbase = 1ull << 20, abase = 1ull << 40;
    int vec = 0, scalar = 0;
    for (int N : ns)
      for (int dv : ds)
        for (int da : ds)
          for (int ov : os)
            for (int oa : os) {
              const SgmBatchPlan p = check(W, H, D, N, vbase + 2 * ov, dhw + dv, abase + 2 * oa, dhw + da);
              if (!p.err) (p.vec_ok ? vec : scalar)++;
            }
    CHECK(vec > 0 && scalar > 0);
  }
  // 2.
  {
    const int N = 2;
    const uint64_t v = 1ull << 20, e = 2;  // bytes per element
    CHECK(check(W, H, D, N, v + 1, dhw, 1ull << 30, dhw).err != nullptr);  // odd vol
    CHECK(check(W, H, D, N, v, dhw, (1ull << 30) + 1, dhw).err != nullptr);  // odd agg
    CHECK(check(W, 2, 256, N, v, 256ull * 2 * W, 1ull << 30, 256ull * 2 * W).err == nullptr);
    CHECK(check(W, 2, 257, N, v, 257ull * 2 * W, 1ull << 30, 257ull * 2 * W).unsupported);
    CHECK(check(W, H, D, N, v, dhw, v + e * dhw, dhw).err != nullptr);            // agg = vol + D H W: inside vol's span
    CHECK(check(W, H, D, N, v, dhw, v + e * (2 * dhw - 1), dhw).err != nullptr);  // one element shared
    CHECK(check(W, H, D, N, v, dhw, v + e * 2 * dhw, dhw).err == nullptr);        // abutting behind
    CHECK(check(W, H, D, N, v, dhw, v - e * 2 * dhw, dhw).err == nullptr);        // abutting in front
    CHECK(check(W, H, D, N, v, dhw, v - e * (2 * dhw - 1), dhw).err != nullptr);
    CHECK(check(W, H, D, N, v, dhw, v, dhw).err != nullptr);                      // agg == vol
    CHECK(check(W, H, D, N, v, 2 * dhw, v + e * dhw, 2 * dhw).err != nullptr);    // interleaved
    CHECK(check(W, H, D, 1, v, 3 * dhw, v + e * dhw, dhw).err == nullptr);  // (N = 1: no gap, the stride is not used)
    CHECK(check(W, H, D, N, v, 3 * dhw, v + e * dhw, dhw).err != nullptr);  // agg inside vol's gap
    CHECK(check(W, H, D, 1, v, dhw, v + e * (dhw - 1), dhw).err != nullptr);
    CHECK(plan_sgm_batch(kSgmU16, 0, H, D, N, v, dhw, 1ull << 30, dhw).err != nullptr);
    CHECK(plan_sgm_batch(kSgmU16, (1 << 14) + 1, 1 << 13, D, N, v, 1ull << 50, 1ull << 62, 1ull << 50).err != nullptr);
  }
  // 3. the largest planes (W H = 2^27) at 256 levels are 2^35 elements; strides near 2^41 with N = 65535
  {
    const int W2 = 1 << 14, H2 = 1 << 13, D2 = 256, N = 65535;
    const uint64_t vol1 = (uint64_t)W2 * H2 * D2;  // 2^35
    CHECK(vol1 == 1ull << 35);
    for (const uint64_t st : {(1ull << 41) - 1, 1ull << 41, (1ull << 41) + 1, (1ull << 41) + 8}) {
      const uint64_t span = 2 * ((uint64_t)(N - 1) * st + vol1);  // bytes, below 2^58
      CHECK(check(W2, H2, D2, N, 4096, st, 4096 + span, st).err == nullptr);      // abutting
      CHECK(check(W2, H2, D2, N, 4096, st, 4096 + span - 2, st).err != nullptr);  // one element shared
      CHECK(check(W2, H2, D2, N, 4096 + span, st, 4096, st).err == nullptr);
      const uint64_t far = (4096 + span + 8 * 65535ull * 2 + 31) & ~15ull;  // 16-byte aligned, behind vol's span
      CHECK(check(W2, H2, D2, N, 4096, st, far, st + 8).vec_ok);
      CHECK(!check(W2, H2, D2, N, 4096, st, far, st + 1).vec_ok);
    }
    // strides whose span does not fit 64 bits: the far span still does not reach the near one's start
    const uint64_t huge = ~0ull / 8;
    CHECK(check(W2, H2, D2, N, 1ull << 62, huge, 4096, 1ull << 41).err == nullptr);
    CHECK(check(W2, H2, D2, N, 4096, huge, 1ull << 62, 1ull << 41).err != nullptr);
  }
  // 4. the phase
  {
    int whole = 0, single = 0;
    for (uint64_t a = 4096; a < 4096 + 16; a += 2) {
      const int ph = sgm_piece_phase(kSgm16Piece, (uintptr_t)a);
      CHECK(ph == (int)((a / 2) % 8));
      for (int n = 1; n <= 40; n++) {
        int owner[40];
        for (int x = 0; x < n; x++) owner[x] = -2;  // -2: unseen, -1: single, else the piece's first pixel
        for (int x = 0; x < n; x++) {
          const int j = sgm_piece_elem(kSgm16Piece, ph, x), xs = x - j;
          CHECK(j >= 0 && j < kSgm16Piece);
          CHECK(((int64_t)a + 2 * (int64_t)xs) % 16 == 0);  // the piece's own address, xs may be negative
          const bool inside = xs >= 0 && xs + kSgm16Piece - 1 < n;
          CHECK(sgm_piece_inside(kSgm16Piece, ph, x, n) == inside);
          owner[x] = inside ? xs : -1;
          (inside ? whole : single)++;
        }
        for (int x = 0; x < n; x++) {
          CHECK(owner[x] != -2);
          if (owner[x] >= 0) {  // the eight pixels of a piece agree on it, and it is aligned
            for (int k = 0; k < kSgm16Piece; k++) CHECK(owner[owner[x] + k] == owner[x]);
          } else {  // single pixels lie in the first or the last seven of the line only
            CHECK(x < 7 || x > n - 8);
          }
        }
        std::printf("phase addr=%llu n=%d ph=%d\n", (unsigned long long)a, n, ph);
      }
    }
    CHECK(whole > 0 && single > 0);
  }
  // 5. the general piece arithmetic: 4's assertions, the piece size a variable
  for (const int piece : {kSgmPiece, kSgm16Piece}) {
    const int elem = 16 / piece;  // bytes per pixel
    int whole = 0, single = 0;
    for (uint64_t a = 4096; a < 4096 + 16; a += elem) {
      const int ph = sgm_piece_phase(piece, (uintptr_t)a);
      CHECK(ph == (int)((a / elem) % piece));
      for (int n = 1; n <= 40; n++) {
        int owner[40];
        for (int x = 0; x < n; x++) {
          const int j = sgm_piece_elem(piece, ph, x), xs = x - j;
          CHECK(j >= 0 && j < piece);
          CHECK(((int64_t)a + elem * (int64_t)xs) % 16 == 0);
          const bool inside = xs >= 0 && xs + piece - 1 < n;
          CHECK(sgm_piece_inside(piece, ph, x, n) == inside);
          owner[x] = inside ? xs : -1;
          (inside ? whole : single)++;
        }
        for (int x = 0; x < n; x++) {
          if (owner[x] >= 0) {
            for (int k = 0; k < piece; k++) CHECK(owner[owner[x] + k] == owner[x]);
          } else {
            CHECK(x < piece - 1 || x > n - piece);
          }
        }
      }
    }
    CHECK(whole > 0 && single > 0);
    for (int N : {1, 2})
      for (uint64_t da = 0; da < 16; da += elem)
        for (uint64_t ds = 0; ds < 9; ds++) {
          const bool ok = sgm_piece_vec_ok(piece, N, 4096, 1000 + ds, 8192 + da, 1000);
          CHECK(ok == (da == 0 && (N == 1 || ds % piece == 0)));
        }
  }
  if (g_bad) std::printf("%d checks failed\n", g_bad);
  return g_bad ? 1 : 0;
}
