// Bootstrap replicates of the demonstrations (mfg_demos_bootstrap, mfg_replicate_bands; include/mfg_hip.h).
//   k_boot_count   grid (days x replicate blocks x groups) x 256: the walk of k_demos_count over the chunks of one day, with
//                  `rb` weighted tallies instead of one.  A replicate block is rb = 4 replicates (one Philox block per agent
//                  serves all four) or, where four sets of tiles do not fit in LDS next to the rank bytes (width near 64), rb = 1.
//                  The weights of a thread's 32 agent slots are drawn once per (chunk, block of hours) and stay in registers,
//                  four bits per replicate; a pair (previous rank, current rank) is up to rb LDS atomics of w, w = 0 skipped.
//                  Flushed once per block of hours into counts [R, N, H, width] and moves [R, N, H-1, width, width] -- the
//                  caller's arrays when given, else the workspace's --, one global integer atomic per non-zero cell.
//   k_demos_finish (mfg_demos.hip, through launch_demos in its second mode) over the R N "days" r N + n: steps 5 to 7.
//   k_boot_status  ORs the day's bad-value flag into the status of each of its replicates.
//   k_bands        a workgroup per BANDS_CELLS consecutive cells x 256: the R values of each cell in LDS; one thread per cell
//                  sums in the order r = 0 .. R - 1 (mean, then squared deviations), every thread ranks elements.
// Workspace: [bad int32 [N] | counts int32 [R, N, H, width] | moves int32 [R, N, H-1, width, width]], each section rounded up to
// 256 bytes; the sections the call uses are zeroed on the stream before the first launch.
#pragma once
#include "mfg_demos.h"

namespace mfg {

constexpr int BOOT_RB = 4;                 // replicates of one Philox block
constexpr int BANDS_CELLS = 16;            // cells of one workgroup of k_bands: R x 16 floats in LDS (64 KiB at R = 1 024)
constexpr int BANDS_THREADS = 256;

struct BootWs {
  int32_t* bad;
  int32_t* counts;
  int32_t* moves;
  size_t bytes;
};

inline BootWs boot_layout(void* base, int R, int N, int H, int width) {
  char* p = reinterpret_cast<char*>(base);
  BootWs w;
  size_t at = 0;
  w.bad = reinterpret_cast<int32_t*>(p + at), at += demos_up((size_t)N * 4);
  w.counts = reinterpret_cast<int32_t*>(p + at), at += demos_up((size_t)R * N * H * width * 4);
  w.moves = reinterpret_cast<int32_t*>(p + at), at += demos_up((size_t)R * N * (H - 1) * width * width * 4);
  w.bytes = at;
  return w;
}

// The LDS of k_boot_count: rb sets of `hours` transitions' (width + 1)^2 tiles next to the day's rank bytes.
struct BootTiles {
  int rb, hours;
  size_t lds_bytes;
};

inline BootTiles boot_tiles(int H, int C, int width) {
  const int tile = (width + 1) * (width + 1) * 4, ranks = (C + 3) / 4 * 4, room = DEMOS_LDS_BUDGET - ranks;
  BootTiles t;
  t.rb = room / tile >= BOOT_RB ? BOOT_RB : 1;
  t.hours = room / (t.rb * tile) < H - 1 ? room / (t.rb * tile) : H - 1;
  t.lds_bytes = (size_t)t.rb * t.hours * tile + ranks;
  return t;
}

}  // namespace mfg
