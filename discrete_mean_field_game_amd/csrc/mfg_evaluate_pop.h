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

// One step's L1 and JSD of a generated row against the test row, by one wave (lane = state entry, `on` = lane < d; every lane
// of the wave calls): L1 = sum_i |emp64 - gen| in fp64, JSD with k_jsd's formula against emp32 (zeros -> 1e-100, M from the
// un-normalised vectors, P, Q, M renormalised; mfg_ac2.py:546-563, :631-666).  gp: this lane's entry of the generated row (read when `on`), eo:
// its offset in emp32 / emp64.  ONE definition for k_eval_metrics_pop (per trajectory) and k_forecast_curves (per step).
__device__ __forceinline__ void eval_step_l1_jsd(const float* __restrict__ gp, const float* __restrict__ emp32, const double* __restrict__ emp64,
                                                 int64_t eo, bool on, double& l1, double& jsd) {
  double a = 1.0, c = 1.0, e1 = 0.0;
  if (on) {
    const float g = *gp;
    e1 = fabs(emp64[eo] - (double)g);
    a = emp32[eo];
    c = g;
    if (a == 0.0) a = 1e-100;
    if (c == 0.0) c = 1e-100;
  }
  l1 = wave_sum(e1);
  const double sp = wave_sum(on ? a : 0.0), sq = wave_sum(on ? c : 0.0);
  const double sm = 0.5 * (sp + sq);
  double acc = 0.0;
  if (on) {
    const double m = 0.5 * (a + c) / sm;
    const double pn = a / sp, qn = c / sq;
    acc = pn * log(pn / m) + qn * log(qn / m);
  }
  jsd = 0.5 * wave_sum(acc);
}

// state: NULL, or the [K] activity states of a control block (a validation check, mfg_pop_validate.h): learner k's block returns
// at once when state[k] != 0
void launch_eval_metrics_pop(const float* pi_traj, const float* emp32, const double* emp64, int64_t N, int L, int d, int64_t NR,
                             int K, double* per_traj, double* metrics, hipStream_t st, const int32_t* state = nullptr);

}  // namespace mfg
