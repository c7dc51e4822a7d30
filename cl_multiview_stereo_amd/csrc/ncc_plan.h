// The NCC sweep's launch planner: every host-side decision of the fused
// per-pixel sweep (which kernel form runs for which reference views, the runs
// they merge into, the shift tables, the LDS bytes) as plain C++ with no HIP
// headers, so it builds with g++ and runs without a GPU
// (tests/host/ncc_plan_check.cpp prints its decisions).  ncc.hip and
// ncc_mfma.hip map an NccLaunch to a kernel instantiation and launch it.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

namespace mvs {
namespace ncc {

constexpr int kMaxNbr = 16;
constexpr int kMaxRef = 8;  // reference views per launch (the fused sweep takes a run of them)
struct NccArgs {
  int W, H, D, nref;
  int tiles_x, ntiles, tiles_per_xcd, nch;  // XCD-aware work map over nref x ntiles tiles (see k_ncc_volume)
  int pk_pairs, st_pairs;  // LDS band heights in row pairs; the pair-row stride is the template BW
  int txmax_all;           // (matrix-core runs) the largest band origin shift of any step: tiles with
                           // x0 >= it never hold image column -1 in a band
  int plane32;             // (scalar kernels) a view plane is under 2 GB: band DMA by buffer descriptors
  // per reference view r of the launch: view id, neighbour count, first plan
  // record, neighbour view ids
  int z[kMaxRef], nn[kMaxRef], plan[kMaxRef];
  int view[kMaxRef][kMaxNbr];
};

// Row-parity modes of a launch's bands (k_ncc_volume's PAR; the plan knows it):
//   kParEven  every level's pk and stats rows start on a pair boundary (K = 5
//             with horizontal neighbours: R + tymax even)
//   kParOdd   every pk start is odd and every stats start even (K = 7 with
//             horizontal neighbours: R = 3)
//   kParMixed either, per level (vertical / diagonal neighbours): a run-time test
constexpr int kParMixed = 0, kParEven = 1, kParOdd = 2;

constexpr int kTileH = 8;           // rows of a tile (both kernel families)
constexpr int kRecWords = 32;       // one 128-B plan record (NccRec per wave, NccMRec per step) as int32
constexpr int kMfMergeStride = 257;  // k_ncc_mfma's LDS merge rows: 256 pixels + 1 (16 classes on distinct banks)

// Every knob of the sweep's launcher.  ncc_tuning() is the one place that
// reads them: MVS_NCC_DPW and MVS_NCC_NW once per process, the others per call.
struct NccTuning {
  int dpw = 4, nw = 8;  // MVS_NCC_DPW (1|2|4) levels per wave, MVS_NCC_NW (4|8) waves: the widest scalar form tried
  int nb = 0;           // MVS_NCC_NB: 2 keeps the K = 5 scalar kernels' bands double-buffered
  int mfma = 1;         // MVS_NCC_MFMA: 0 keeps the scalar kernels
  int mfma_v = 1;       // MVS_NCC_MFMA_V: vertical / diagonal lists: 0 scalar, 1 automatic, 22|21|12|11 that form
  int mfma7 = 1;        // MVS_NCC_MFMA7: 0 keeps the scalar kernels at K = 7
  int mfma_dbg = 0;     // MVS_NCC_MFMA_DBG: timing probes (1 no MFMA / finish, 2 no band DMA)
  int run = kMaxRef;    // MVS_NCC_RUN: reference views per launch at most
  int plane32 = 1;      // MVS_NCC_PLANE32: 0 stages the scalar kernels' bands by 64-bit addresses
  // mvs_set_ncc_variant's overrides (0: automatic); any of them keeps the scalar kernels
  int force_nw = 0, force_dpw = 0, force_bw = 0, force_general = 0;
};
NccTuning ncc_tuning(int force_nw, int force_dpw, int force_bw, int force_general);

// The size rules, each defined once: the selection, the run merging and the
// launch all go through them.
// Scalar kernels: nb band buffers of `pairs` (pk + stats) pair rows at `pitch`
// columns of 16 B; fused, the WTA merge area shares them and s_r [64][TH] follows.
size_t scalar_lds_bytes(int nb, int pairs, int pitch, int nw, bool fuse);
// Matrix-core kernels: bands at pitch + 1 (sharing the merge area), -Sr' and
// s_r of the tile, and the level offsets of tmax steps of dc levels.
size_t mfma_lds_bytes(int pitch, int nb, int pairs, int tmax, int dc);
// the scalar band pitch template holding band_w columns: 64, 80, 96, 128, 192, 256
int scalar_pitch(int band_w);
// the matrix-core band pitch template (tail: the last chunk carries dummy levels)
int mfma_pitch(bool vert, bool tail, int K, int band_w);

// One kernel launch: everything it needs, nothing device-side.
struct NccLaunch {
  bool mfma = false;  // family: k_ncc_mfma, else k_ncc_volume
  // template coordinates (scalar: K DPW NW BW PAR NB FUSE; matrix-core: K BW TAIL VERT NDB NB DBG)
  int K = 0, BW = 0, NB = 2;
  int DPW = 0, NW = 0, PAR = 0, FUSE = 0;
  int TAIL = 0, VERT = 0, NDB = 0, DBG = 0;
  int first = 0;               // index of its first reference view in [z0, z1)
  NccArgs args{};              // complete, the work map included
  std::vector<int32_t> table;  // the plan records (matrix-core: words 22, 23 hold the neighbour plane's byte offset)
  int tmax = 0;                // (matrix-core) the most steps of any member view
  size_t lds = 0;              // dynamic LDS bytes
  int last[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // mvs_ncc_last_variant's slots {K, TH, DPW, NW, BW, PAR, FUSE, NB}
};

// The launches of reference views [z0, z1), in order.  False with `err` set on
// an argument error (the launcher's arg_fail messages).
bool plan_ncc_launches(const NccTuning& t, int V, int W, int H, int K, int D, const float* levels, const int* vs,
                       const int* sn, int aw, float bl, int z0, int z1, bool want_volume,
                       std::vector<NccLaunch>& out, std::string& err);

}  // namespace ncc
}  // namespace mvs
