// Population launches (mfg_train_episodes_pop / mfg_train_rollouts_pop): K independent learners served by every launch of an
// episode.  A population launch is K single launches laid side by side: grid (gx, K) -- gx the grid the single call takes for
// one learner's Bk trajectories -- and blockIdx.y (blockIdx.z for kernels whose single form already has a 2-D grid) is the
// learner.  Every kernel first rebases its argument block to learner k (pointers moved by k x their per-learner stride, the
// per-learner scalars read from device arrays [K]) and then runs the body of the single kernel unchanged, so the summation
// trees and the Philox keys (trajectory ids traj_offset .. traj_offset + Bk - 1 under the learner's seed) are those of a
// single-learner call: the same bits.  The kernels are in mfg_population.hip, the episode loops in mfg_kernels.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mfg_core.h"

struct GradArgs;
struct ReduceApply;

namespace mfg {

struct PopArgs {
  int K;
  int64_t F;        // critic features of one learner (w stride; G stride F + 3)
  int64_t s_pi0;    // floats between the learners' start / current states of the core launch (0: the shared start-state table)
  int64_t s_gpi;    // floats between the learners' states read by the gradient kernels (pi_traj or the step's states)
  int64_t s_traj;   // pi_traj floats
  int64_t s_state;  // [Bk, d] state buffers (pi_next_out, draw output)
  int64_t s_n;      // reward / delta / g elements
  int64_t s_acc;    // reward_acc doubles (the episodes of the call)
  int64_t s_ws;     // workspace bytes of one learner's slice
  const uint64_t* seed;
  const double *shift, *alpha_scale, *lr_c, *lr_a;  // [K]
  double sc, sa;  // learning-rate multipliers of the episode (lr_schedule): learner k's rates are lr_c[k] sc, lr_a[k] sa
};

// launchers (mfg_population.hip); grids as the single launches of one learner, times K
int launch_core_small_pop(const CoreArgs& a, const PopArgs& p, bool fast, int num_cus, hipStream_t st);
void launch_draw_start_pop(int grid, const float* mat, int64_t num_start, int64_t B, int d, uint32_t step, uint64_t traj_offset,
                           float* out, const PopArgs& p, hipStream_t st);
void launch_grad_mfma_small_pop(int D, unsigned blocks, const GradArgs& a, const PopArgs& p, hipStream_t st);
void launch_grad_partial_pop(unsigned nsb, unsigned nob, size_t lds, const GradArgs& a, const PopArgs& p, hipStream_t st);
void launch_grad_mfma_pop(int npf, unsigned nsb, unsigned ny, size_t lds, const GradArgs& a, int tpw, const PopArgs& p,
                          hipStream_t st);
void launch_reduce_partials_pop(unsigned nob, const double* partial, int64_t nsb, int64_t FO, double* G, const ReduceApply& ap,
                                const PopArgs& p, hipStream_t st);

}  // namespace mfg
