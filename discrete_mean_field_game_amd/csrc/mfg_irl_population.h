// IRL populations (mfg_train_episodes_irl_pop / mfg_train_rollouts_irl_pop): K independent forward learners of AC_IRL.train served
// by every launch of an episode, as mfg_population.h does for the in-kernel rewards.  Grid (the single call's grid for Bk, K),
// learner = blockIdx.y; each kernel rebases its argument block to learner k and runs the single kernel's body unchanged:
//   k_core_irl_pop        the packed core kernel, IRL variants (STEP 0: the rollout with P, STEP 1 / 2: an env step)
//   k_reward_net_mfma_pop the matrix-core reward network (plain over a rollout's pi_traj, or SUMS with the TD error)
//   k_reduce_rows_apply_pop  the row reduction that closes a step-mode episode
// The rollout flow's batch sums are the gradient population kernels of mfg_population.h with the reward folded in.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mfg_core.h"

namespace mfg {

// the core kernel's per-learner strides (elements of the pointee; *_b: bytes) and scalars
struct IrlCorePop {
  int K;
  int64_t s_pi0;      // current states (0: the shared start-state table, drawn in the kernel)
  int64_t s_state;    // [Bk,d] buffers: pi_start_out, pi_next_out
  int64_t s_theta_b;  // bytes between the learners' theta in (8: theta [K]; the slice: a theta slot of the workspace)
  int64_t F;          // w / w_out stride
  int64_t s_traj;     // pi_traj
  int64_t s_n;        // delta / g
  int64_t s_P;        // P_out
  int64_t s_acc;      // reward_acc
  int64_t s_ws;       // bytes of one learner's workspace slice (step_rows, theta_out)
  const uint64_t* seed;
  const double *shift, *alpha_scale, *lr_c, *lr_a;  // [K]
  double sc, sa;      // the episode's learning-rate multipliers (lr_schedule)
};

// the reward network's per-learner strides: states / actions / outputs, the learner's key, and its weights (per_learner_net:
// learner k's tensor t at base_t + k numel_t, numel_t from the geometry, or at base_t + k s_net when s_net > 0; 0: shared).
// Key of learner k: key[slot] when given, else rn_seed[k] ^ ((call_base[k] + call_j) 0x9E3779B97F4A7C15) when call_base is
// given (per-learner reward-call counters), else rn_seed[k] ^ key_ctr.  Grid rows: n_y slots, slot -> learner[slot] when
// learner is given (0 / NULL: K rows, slot = learner).
struct RnPop {
  int K;
  int per_learner_net;
  int64_t s_state, s_action, s_n, s_next, s_w;  // elements
  int64_t s_ws;                                  // bytes (part_rows, col_f: in the learner's workspace slice)
  const uint64_t* rn_seed;
  uint64_t key_ctr;
  int64_t s_net;                                 // elements between two learners' weights (0: numel_t per tensor)
  const uint64_t* call_base;                     // [K] device (NULL: the shared key_ctr)
  uint64_t call_j;
  const uint64_t* key;                           // [n_y] device, by slot (NULL: from rn_seed)
  const int32_t* learner;                        // [n_y] device (NULL: slot = learner)
  int n_y;
};

int launch_core_irl_pop(const CoreArgs& a, const IrlCorePop& p, bool fast, int num_cus, hipStream_t st);
void launch_reduce_rows_apply_pop(const double* rows, int nrows, int64_t FO, double* G, double count, double* w,
                                  const double* theta_in, int64_t s_theta_in_b, double* theta_out, double* reward_acc,
                                  const IrlCorePop& p, hipStream_t st);

// true: K learners' networks of this geometry (fc3_w of every learner 8-byte aligned) run the matrix-core kernel
// (net_stride > 0: learner k's tensors at base + k net_stride; 0: the numel_t strides)
bool reward_net_pop_ready(int d, const mfg_reward_net_t* net, int per_learner_net, int K, int64_t net_stride = 0);
// the population form of reward_net_forward_sums for the matrix-core kernel (reward_net_pop_ready said yes); sums: the SUMS
// variant with the TD error (*rows_out = partial rows per learner), NULL: the plain forward
int reward_net_forward_pop(const float* state, const float* action, int64_t B, int d, const mfg_reward_net_t* net,
                           uint64_t sample_offset, float* reward, const RnSums* sums, int* rows_out, const RnPop& p, hipStream_t st,
                           int state_T);

}  // namespace mfg
