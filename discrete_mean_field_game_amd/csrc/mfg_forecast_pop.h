// Ensemble forecast (mfg_forecast_pop): R rollouts per start state of K policies, reduced on the device to the expected
// histogram per hour, its spread, order statistics per topic and the error curves against held-out rows -- what the reference
// draws by hand from ONE path in visualize_test (mfg_ac2.py:763, ac_irl.py:1663) and what its VAR baseline returns as a forecast
// with intervals (var.py:294-327).  At most three launches, no host synchronisation:
//   launch 1, k_eval_rollout_pop (mfg_evaluate_pop.h), grid (gx, K): learner k's N R members; member j starts at
//     start32[j mod N] (the start-index table with a row stride of 1 instead of the L of an evaluation) under the Philox keys
//     (seed[k], first_step + t, j): the trajectories of mfg_evaluate_pop over an emp32 whose row 0 is start32.
//   launch 2, k_forecast_reduce, grid (N H, K): one block per cell (k, n, l).  The R member rows of the cell (N H d floats
//     apart, d contiguous floats each) are read row by row into LDS, transposed: column i's R values are contiguous, columns
//     FC_PAD floats apart modulo the power of two, so the transposing writes of a wave fall on distinct banks.  One wave per
//     column: mean and std (ddof = 0, two passes, fp64 from the fp32 values; lane r mod 64 sums members r, r + 64, ... in
//     that order, the 64 lane sums go through the xor butterfly of wave_sum -- an order that depends on R alone), then a
//     bitonic sort of the column padded with +inf to a power of two, from which the Q order statistics are copied: elements
//     of the ensemble, bit exact.  Columns go in chunks of forecast_chunk(d, R) so that a block asks for at most FC_LDS_BUDGET.
//   launch 3 (emp given), k_forecast_curves, grid (H, K): one block per (k, l), a wave per member: the step's L1 and JSD
//     (eval_step_l1_jsd, the body k_eval_metrics_pop runs per trajectory), then mean and std over the N R members in a fixed
//     order (16 waves; lane 0 of wave w adds members w, w + 16, ...; wave totals in wave order).
// No floating-point atomics: learner k's outputs depend on its own inputs only, run to run and whatever K is.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mfg_hip.h"
#include "mfg_evaluate_pop.h"

namespace mfg {

// LDS of one k_forecast_reduce block: 64 KB, the most a launch gets without opting into more and well inside the 160 KB of a
// CU (two blocks per CU stay resident at the cap).  A column of R members takes (P2 + FC_PAD) floats, P2 the power of two >= R.
constexpr size_t FC_LDS_BUDGET = 64 * 1024;
constexpr int FC_PAD = 1;
inline int forecast_p2(int repeats) {
  int p = 1;
  while (p < repeats) p <<= 1;
  return p;
}
// columns per chunk: as many as the budget holds, at most d (>= 15 at the cap of 1024 repeats)
inline int forecast_chunk(int d, int repeats) {
  const size_t col = (size_t)(forecast_p2(repeats) + FC_PAD) * sizeof(float);
  const size_t fit = FC_LDS_BUDGET / col;
  return (int)(fit < (size_t)d ? fit : (size_t)d);
}
inline size_t forecast_lds_bytes(int d, int repeats) {
  return (size_t)forecast_chunk(d, repeats) * (size_t)(forecast_p2(repeats) + FC_PAD) * sizeof(float);
}

// workspace layout of mfg_forecast_pop: [idx tables | per-member per-step (L1, JSD) [K][H][N R][2] fp64 (used when emp is
// given) | pi_traj if not given]
inline size_t forecast_pop_workspace_bytes(int64_t N, int H, int d, int K, int repeats, bool traj_given) {
  const int64_t NR = N * repeats;
  size_t b = (size_t)K * (size_t)eval_pop_idx_stride(NR) * 4 + (size_t)K * (size_t)H * (size_t)NR * 2 * 8;
  if (!traj_given) b += (size_t)K * (size_t)NR * H * d * 4;
  return b;
}

struct ForecastRanks {
  int32_t r[MFG_FORECAST_MAX_RANKS];
};

// MFG_ELAUNCH (nothing launched) if the LDS request of the shape were to exceed the budget
int launch_forecast_reduce(const float* pi_traj, int64_t N, int H, int d, int K, int repeats, const ForecastRanks& ranks, int Q,
                           double* mean, double* std, float* quant, hipStream_t st);
void launch_forecast_curves(const float* pi_traj, const float* emp32, const double* emp64, int64_t N, int H, int d, int64_t NR,
                            int K, double* per_step, double* curves, hipStream_t st);

}  // namespace mfg
