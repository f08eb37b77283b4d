// Proper scores of an ensemble forecast (mfg_forecast_score): CRPS per topic, the energy score per histogram and the rank of
// the observation among the members, for the members mfg_forecast_pop wrote -- the reference scores ONE sample path by L1 /
// JSD (evaluate, mfg_ac2.py:595-670; the VAR baseline, var.py:330-416) and has no scorer for a forecast distribution.
// Definitions: Gneiting & Raftery, JASA 2007 (kernel forms, beta = 1).  At most two launches, no host synchronisation:
//   launch 1, k_forecast_score, grid (N H, K): one block of four waves per cell (k, n, l), in two passes over the cell's R
//     member rows (N H d floats apart, d contiguous floats each).
//     Columns: the rows are read into LDS transposed, as k_forecast_reduce does (column c's R values contiguous, columns
//     P2 + 1 floats apart, P2 the power of two >= R, so a wave's transposing writes fall on distinct banks), in chunks of
//     score_chunk(d, R) columns.  One wave per column: the counts #{x < y32}, #{x == y32} (fp32 comparisons, integer sums) and
//     A = sum_r |x_r - y64| in fp64 (lane r mod 64 adds members r, r + 64, ... in that order, the 64 lane values go through
//     the xor butterfly of wave_sum), then the bitonic sort of the column padded with +inf and
//     S = sum_i (2 i - R + 1) x_(i) over the ascending column (lane i mod 64 adds entries i, i + 64, ..., wave_sum; every
//     product is exact: an integer below 2^11 times an fp32 value), which is half of sum_{r,s} |x_r - x_s|:
//     crps = A / R - S / R^2.
//     Energy (skipped without `energy`): the rows are read row-wise in tiles of FS_TILE members, rows score_row_stride(d)
//     floats apart (odd, so lanes that read the same column of different members hit different banks).  Tile ta stays resident while the tiles
//     tb >= ta pass by: every unordered pair r < s is met once.  In a tile pair lane j owns member j of tile tb and wave w the
//     rows a = w, w + 4, ... of tile ta, four rows at a time; ||x_r - x_s|| is sqrt(sum_c (x_rc - x_sc)^2), columns
//     ascending, differences, squares (fused multiply-add) and sqrt in fp64.  Each thread adds its pairs' norms to ONE fp64
//     partial in the order (ta, tb, a) ascending; at the end the 64 lane partials go through wave_sum and the four wave totals are added in wave
//     order: P = sum_{r<s}.  The lanes of wave 0 add ||x_r - y64|| of members lane, lane + 64, ... (tile order), then wave_sum: B.
//     energy = B / R - P / R^2.
//     Thread 0 adds the cell's d CRPS values in column order into the workspace (cell_crps [K, N, H]).
//     A cell with a non-finite member or observation (seen while loading) writes NaN and -1 instead; nothing of it reaches
//     another cell.
//   launch 2, k_forecast_score_summary, grid (H, K), one wave: lane n mod 64 adds cell_crps and energy of start rows n,
//     n + 64, ... in that order, wave_sum, divided by N d and N.
// No floating-point atomics, no synchronisation beyond the workgroup: policy k's outputs depend on its own inputs only, run to
// run and whatever K is.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mfg_hip.h"

namespace mfg {

// members per tile of the energy pass: two tiles of FS_TILE rows at the widest row (d = 64: 65 floats) take 33 280 B
constexpr int FS_TILE = MFG_FORECAST_SCORE_TILE;
// LDS of the column pass: 60 KB, which with the block's static arrays (under 2 KB) stays inside the 64 KB a launch gets
// without opting into more.  A column of R members takes (P2 + 1) floats.
constexpr size_t FS_COL_BUDGET = 60 * 1024;
inline int score_p2(int repeats) {
  int p = 1;
  while (p < repeats) p <<= 1;
  return p;
}
// columns per chunk: as many as the budget holds, at most d (14 at the cap of 1024 repeats)
inline int score_chunk(int d, int repeats) {
  const size_t col = (size_t)(score_p2(repeats) + 1) * sizeof(float);
  const size_t fit = FS_COL_BUDGET / col;
  return (int)(fit < (size_t)d ? fit : (size_t)d);
}
inline int score_row_stride(int d) { return d | 1; }
// dynamic LDS of one block: the larger of the column chunk and (with the energy pass) the two row tiles
inline size_t score_lds_bytes(int d, int repeats, bool want_energy) {
  const size_t cols = (size_t)score_chunk(d, repeats) * (size_t)(score_p2(repeats) + 1) * sizeof(float);
  const size_t tiles = want_energy ? (size_t)2 * FS_TILE * score_row_stride(d) * sizeof(float) : 0;
  return cols > tiles ? cols : tiles;
}

// workspace of mfg_forecast_score: cell_crps [K, N, H] fp64
inline size_t forecast_score_workspace_bytes(int64_t N, int H, int K) { return (size_t)K * (size_t)N * (size_t)H * 8; }

// MFG_ELAUNCH (nothing launched) if the LDS request of the shape were to exceed the budget.  state: NULL, or the [K] activity
// states of a control block (a validation check, mfg_pop_validate.h): policy k's blocks return at once when state[k] != 0
int launch_forecast_score(const float* traj, int64_t N, int H, int d, int K, int repeats, const float* emp32, const double* emp64,
                          double* crps, int32_t* less, int32_t* equal, double* energy, double* summary, double* cell_crps,
                          hipStream_t st, const int32_t* state = nullptr);

}  // namespace mfg
