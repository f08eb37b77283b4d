// Population evaluation (mfg_evaluate_pop): the test rollouts and the L1 / JSD metrics of K policies in two launches
// (evaluate / gridsearch, mfg_ac2.py:595-689, ac_irl.py:1495-1590).
//   launch 1, k_eval_rollout_pop, grid (gx, K): learner blockIdx.y's N R test trajectories -- the packed core kernel's body
//     (core_small_body, sampling without TD) on the argument block rebased to the learner by pop_core_args (mfg_population.h),
//     so trajectory j carries the Philox keys (seed[k], first_step + t, j) of a single mfg_rollout over the same start rows.
//     Start row of trajectory j: emp32[j mod N, 0], gathered through a per-learner index table that each block writes for
//     its OWN tiles before it runs the body (the body reads the rows of no other tile).
//   launch 2, k_eval_metrics_pop, grid K: one block per learner, a wave per trajectory (lanes = state entries): L1 per step
//     in fp64 against emp64, JSD per step with k_jsd's formula against emp32, the final row and the mean over the L rows;
//     then mean and population std (ddof = 0) over the learner's N R trajectories, summed in a fixed order.
// No floating-point atomics: a learner's outputs depend on nothing but its own inputs, run to run and whatever K is.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mfg_core.h"
#include "mfg_population.h"

namespace mfg {

// workspace layout of mfg_evaluate_pop: [idx tables | per-trajectory metrics [K][N R][4] fp64 | pi_traj if not given]
inline int64_t eval_pop_idx_stride(int64_t NR) { return (NR * 4 + 255) / 256 * 256 / 4; }
inline size_t eval_pop_workspace_bytes(int64_t N, int L, int d, int K, int repeats, bool traj_given) {
  const int64_t NR = N * repeats;
  size_t b = (size_t)K * (size_t)eval_pop_idx_stride(NR) * 4 + (size_t)K * (size_t)NR * 4 * 8;
  if (!traj_given) b += (size_t)K * (size_t)NR * L * d * 4;
  return b;
}

void launch_eval_metrics_pop(const float* pi_traj, const float* emp32, const double* emp64, int64_t N, int L, int d, int64_t NR,
                             int K, double* per_traj, double* metrics, hipStream_t st);

}  // namespace mfg
