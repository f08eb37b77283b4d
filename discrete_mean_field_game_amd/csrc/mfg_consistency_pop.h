// Backward-equation check of K policies (mfg_consistency_given / mfg_consistency_pop): the scoring half of the reference's
// synthetic sweep (evaluate_synthetic / evaluate_synthetic_JSD, mfg_synthetic.py:741-899, looped over 200 learners by its
// __main__, :902-925), reduced on the device.
//   launch 1 of mfg_consistency_pop, k_eval_rollout_pop (mfg_evaluate_pop.h), grid (gx, K): learner k's N R members, member j
//     from start32[j mod N] under the Philox keys (seed[k], first_step + t, j), with P_out set: the actions land in
//     [K, N R, T, d, d] (generate_trajectory's action matrices, :566-592 of mfg_ac2.py as mfg_synthetic inherits it).
//   k_consistency_backward, one wave per trajectory: the reverse-time scan V^n = r^n + P^n V^{n+1}, r^n_i = -1/2 |P^n_i|^2,
//     V^T = 0 (:768-774) and per hour sum_ij |P_ij - value_ij| (:776-790) and sum_i JSD(P_i, implied row i) (:858-880) with
//     k_backward_value's formulas.  P^n is read ONCE, 64 consecutive floats per wave load, into the wave's LDS tile; row i is
//     then worked on by consistency_lanes(d) lanes (three at d = 21, four at d = 15: 63 / 60 of 64 lanes busy against the 21 / 15
//     of k_backward_value), lane s of the row taking columns s, s + L, ...; the row's lane partials are added in lane order,
//     rows through the xor butterfly of wave_sum: an order that depends on d alone.  V goes to HBM only when asked for.
//   k_consistency_reduce, grid K: mean and std (ddof = 0, np.mean / np.std at :800-801, :887-888) over the group's M T values
//     in two passes: thread t adds values t, t + BLOCK, ... in that order, the 64 lane sums go through wave_sum, the wave
//     totals are added in wave order.
// No floating-point atomics: group k's outputs depend on group k's inputs only, run to run and whatever K is.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mfg_hip.h"
#include "mfg_evaluate_pop.h"

namespace mfg {

// lanes per row of the backward kernel: as many as fit d rows into a wave, at most d (a lane without a column has no work)
inline __host__ __device__ int consistency_lanes(int d) {
  const int l = WAVE / d;
  return l < d ? l : d;
}
// LDS of one wave: the fp32 tile of P^n [d, d] rounded up to whole doubles, then V^{n+1} and V^n [d] fp64
inline __host__ __device__ size_t consistency_wave_lds(int d) { return ((size_t)d * d * 4 + 7) / 8 * 8 + (size_t)2 * d * 8; }
// waves per block: WAVES while a block stays within the 64 KB a launch gets without opting into more (d <= 62), else two
// (d = 64: 2 x 17 408 B)
constexpr size_t CONSISTENCY_LDS_BUDGET = 64 * 1024;
inline int consistency_waves(int d) { return (size_t)WAVES * consistency_wave_lds(d) <= CONSISTENCY_LDS_BUDGET ? WAVES : 2; }
// blocks per CU the backward launch is capped at (more trajectories than that many waves are strided over)
constexpr int CONSISTENCY_BLOCKS_PER_CU = 8;

// workspace of mfg_consistency_given: the per-step (l1, jsd) [K, M, T, 2] fp64 when `steps` is not given
inline size_t consistency_given_workspace_bytes(int K, int64_t M, int T, bool steps_given) {
  return steps_given ? 0 : (size_t)K * (size_t)M * (size_t)T * 2 * 8;
}
// workspace layout of mfg_consistency_pop: [idx tables | per-step values if `steps` is not given | pi_traj if not given |
// actions if not given]
inline size_t consistency_pop_workspace_bytes(int64_t N, int H, int d, int K, int repeats, bool steps_given, bool actions_given,
                                              bool traj_given) {
  const int64_t NR = N * repeats;
  size_t b = (size_t)K * (size_t)eval_pop_idx_stride(NR) * 4 + consistency_given_workspace_bytes(K, NR, H - 1, steps_given);
  if (!traj_given) b += ((size_t)K * (size_t)NR * H * d * 4 + 7) / 8 * 8;
  if (!actions_given) b += (size_t)K * (size_t)NR * (H - 1) * d * d * 4;
  return b;
}

// the two launches on given actions P [B, T, d, d] (B = K M): steps [B, T, 2] is written always, V [B, T+1, d] when not NULL
void launch_consistency_backward(const float* P, int64_t B, int T, int d, double* V, double* steps, int num_cus, hipStream_t st);
void launch_consistency_reduce(const double* steps, int K, int64_t MT, double* metrics, hipStream_t st);

}  // namespace mfg
