// Population launches: K independent learners served by every launch of one call (mfg_train_episodes_pop /
// mfg_train_rollouts_pop, their IRL forms mfg_train_*_irl_pop and mfg_evaluate_pop).  A population launch is K single
// launches laid side by side: grid (gx, K) -- gx the grid the single call takes for one learner's Bk trajectories -- and
// blockIdx.y (blockIdx.z for kernels whose single form already has a 2-D grid) is the learner.  Every kernel first rebases its
// argument block to learner k (pointers moved by k x their per-learner stride, the per-learner scalars read from device arrays
// [K]) and then runs the body of the single kernel unchanged, so the summation trees and the Philox keys (trajectory ids
// traj_offset .. traj_offset + Bk - 1 under the learner's seed) are those of a single-learner call: the same bits.  The
// kernels are in mfg_population.hip, mfg_population_ctl.hip and mfg_evaluate_pop.hip, the episode loops in mfg_kernels.hip.
//
// Retiring learners (mfg_ctx_set_pop_control, include/mfg_hip.h): with a control block every training launch carries the learners'
// activity state [K] (PopArgs::state) and runs the _ctl form of each wrapper, which returns before the single kernel's body when
// its learner's state is not 0 -- block-uniform, ahead of every barrier -- so a learner that stopped early or diverged leaves the
// launches at once while the others run on; a launch without a block runs the plain form, which has no such test.  k_pop_retire, one wave per learner, moves the states between two episodes; nothing is read back by the host.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mfg_core.h"

struct GradArgs;
struct ReduceApply;

namespace mfg {

// per-learner strides (elements of the pointee; *_b / s_ws: bytes) and scalars of every population launch (the fields of the
// IRL and evaluation forms last: the others keep their offsets in the kernel arguments)
struct PopArgs {
  int K;
  int L;             // evaluation: rows of the start table between two start rows (a test file's rows; 1 for a forecast's [N, d])
  int64_t F;         // critic features of one learner (w stride; G stride F + 3)
  int64_t s_pi0;     // floats between the learners' start / current states of the core launch (0: the shared start-state table)
  int64_t s_gpi;     // floats between the learners' states read by the gradient kernels (pi_traj or the step's states)
  int64_t s_traj;    // pi_traj floats
  int64_t s_state;   // [Bk, d] state buffers (pi_next_out, pi_start_out, draw output)
  int64_t s_n;       // reward / delta / g elements
  int64_t s_acc;     // reward_acc doubles (the episodes of the call)
  int64_t s_ws;      // workspace bytes of one learner's slice
  const uint64_t* seed;
  const double *shift, *alpha_scale, *lr_c, *lr_a;  // [K] (lr_c / lr_a: training only)
  double sc, sa;     // learning-rate multipliers of the episode (lr_schedule): learner k's rates are lr_c[k] sc, lr_a[k] sa
  int64_t s_P;       // IRL: P_out floats
  int64_t s_theta_b; // IRL: bytes between the learners' theta of a STEP core launch and of the closing row reduction (a theta
                     // slot of the workspace slice, or 8: theta [K])
  int64_t N;         // evaluation: test files
  int64_t s_idx;     // evaluation: int32 entries between the learners' start-index tables (padded to 256 bytes)
  int32_t* idx;      // evaluation: [K][s_idx] start-index tables (workspace)
  const int32_t* state;  // control block: [K] 0 active, 1 stopped, 2 failed (NULL: no control block, every learner runs)
  unsigned* status;      // control block: [K] per-learner status words (the core kernel's range report of learner k)
};

// true: learner k of a launch with a control block has been retired (the _ctl wrappers, which the launchers run exactly when
// p.state is set, return before the body; the plain wrappers never read it)
__device__ __forceinline__ bool pop_retired(const PopArgs& p, int k) { return p.state[k] != 0; }

// p moved by k x `stride` elements / bytes; a null pointer stays null
template <class P>
__device__ __forceinline__ P* pop_at(P* p, int64_t stride, int k) {
  return p ? p + stride * k : p;
}
template <class P>
__device__ __forceinline__ P* pop_bytes(P* p, int64_t bytes, int k) {
  using C = std::conditional_t<std::is_const_v<P>, const char, char>;
  return p ? reinterpret_cast<P*>(reinterpret_cast<C*>(p) + bytes * k) : p;
}

// The core kernel's argument block of learner k.  The unions of CoreArgs are rebased as the variant reads them: part_rows
// (SUMS) or step_G / step_rows (STEP 1), P_in or pi_start_out (STEP 2); the deferred-update fields belong to STEP 1 alone.
// Fields a variant never reads stay as they are: a rebased pointer is one more value the kernel keeps live (measured: with
// reward_out rebased in the STEP forms too, k_core_pop<false, 21, false, 1> spilled 4 more bytes per lane; with P_out and a
// byte-strided theta in the SUMS forms, the per-step population episodes took 1 % longer).
// CTL: the launch carries a control block (status is set, as mfg_ctx_set_pop_control demands).
template <bool SUMS, int STEP, bool CTL = false>
__device__ __forceinline__ CoreArgs pop_core_args(const CoreArgs& a, const PopArgs& p, int k) {
  CoreArgs b = a;
  b.pi0 = pop_at(a.pi0, p.s_pi0, k);
  if constexpr (STEP == 0) b.theta = a.theta + k;  // (theta [K]; the STEP forms read a slot of the learner's workspace slice)
  else b.theta = pop_bytes(a.theta, p.s_theta_b, k);
  b.w = pop_at(a.w, p.F, k);
  b.shift = p.shift[k];
  b.alpha_scale = p.alpha_scale[k];
  b.seed = p.seed[k];
  if constexpr (CTL) b.status = p.status + k;  // (an out-of-range theta is booked to the learner, not to the context)
  b.pi_traj = pop_at(a.pi_traj, p.s_traj, k);
  b.pi_next_out = pop_at(a.pi_next_out, p.s_state, k);
  if constexpr (STEP == 0) b.reward_out = pop_at(a.reward_out, p.s_n, k);  // (the STEP forms take an external reward)
  b.delta = pop_at(a.delta, p.s_n, k);
  b.g = pop_at(a.g, p.s_n, k);
  if constexpr (!SUMS) b.P_out = pop_at(a.P_out, p.s_P, k);  // (SUMS: in-kernel reward, no actions written)
  if constexpr (SUMS) b.part_rows = pop_bytes(a.part_rows, p.s_ws, k);
  if constexpr (STEP == 2) b.pi_start_out = pop_at(a.pi_start_out, p.s_state, k);
  if constexpr (STEP == 1) {
    b.step_G = pop_at(a.step_G, p.F + 3, k);
    b.step_rows = pop_bytes(a.step_rows, p.s_ws, k);
    b.w_out = pop_at(a.w_out, p.F, k);
    b.theta_out = pop_bytes(a.theta_out, p.s_ws, k);
    b.pend_reward_acc = pop_at(a.pend_reward_acc, p.s_acc, k);
    b.pend_lr_c = p.lr_c[k] * p.sc;
    b.pend_lr_a = p.lr_a[k] * p.sa;
  }
  return b;
}

// launchers (mfg_population.hip, mfg_population_ctl.hip, mfg_evaluate_pop.hip); grids as the single launches of one learner, times K.  launch_core_pop:
// training (sampling + TD); the variant follows the arguments as in launch_core_small: part_rows -> SUMS, step_nrows > 0 ->
// STEP 1, < 0 -> STEP 2.  launch_eval_rollout_pop: sampling without TD (mfg_evaluate_pop.h).
int launch_core_pop(const CoreArgs& a, const PopArgs& p, bool fast, int num_cus, hipStream_t st);
int launch_core_pop_ctl(const CoreArgs& a, const PopArgs& p, bool fast, int num_cus, hipStream_t st);  // (its p.state half: mfg_population_ctl.hip)
int launch_eval_rollout_pop(const CoreArgs& a, const PopArgs& p, bool fast, int num_cus, hipStream_t st);
void launch_draw_start_pop(int grid, const float* mat, int64_t num_start, int64_t B, int d, uint32_t step, uint64_t traj_offset,
                           float* out, const PopArgs& p, hipStream_t st);
void launch_grad_mfma_small_pop(int D, unsigned blocks, const GradArgs& a, const PopArgs& p, hipStream_t st);
void launch_grad_partial_pop(unsigned nsb, unsigned nob, size_t lds, const GradArgs& a, const PopArgs& p, hipStream_t st);
void launch_grad_mfma_pop(int npf, unsigned nsb, unsigned ny, size_t lds, const GradArgs& a, int tpw, const PopArgs& p,
                          hipStream_t st);
void launch_reduce_partials_pop(unsigned nob, const double* partial, int64_t nsb, int64_t FO, double* G, const ReduceApply& ap,
                                const PopArgs& p, hipStream_t st);
// the row reduction + update that closes a step-mode IRL episode: learner k's theta in at theta_in + k p.s_theta_b bytes
void launch_reduce_rows_apply_pop(const double* rows, int nrows, int64_t FO, double* G, double count, double* w,
                                  const double* theta_in, double* theta_out, double* reward_acc, double* slots, const PopArgs& p,
                                  hipStream_t st);

// The resident form of the step-mode episodes (mfg_pop_resident.hip, mfg_train_episodes_pop_resident): what one launch of
// k_pop_resident needs beyond CoreArgs (shape, gamma, reward_kind, traj_offset, htab, status, reward / delta / g and the rows
// in part_rows; pi0, theta, w, first_step and pi_next_out are set by the kernel) and PopArgs (strides and per-learner arrays;
// sc / sa unused).  The learning-rate multipliers of the launch's episodes come from the host (lr_schedule: libm's log), by
// value: hence at most MFG_POP_RESIDENT_EPISODES episodes per launch.
struct PopResidentArgs {
  const float* mat_pi0;  // [num_start, d] start-state table
  int64_t num_start;
  float *pi_io, *pi_scratch;  // [K, Bk, d]
  double *theta, *w, *G;      // [K], [K, F], [K, F + 3]
  double* reward_acc;         // [K, s_acc] moved to the launch's first episode, or NULL
  int T, episodes;            // env steps per episode; episodes of this launch
  uint32_t first_step;        // Philox step of the launch's first episode
  double sc[MFG_POP_RESIDENT_EPISODES], sa[MFG_POP_RESIDENT_EPISODES];
};
// d = 21 / 15 only (MFG_EUNSUPPORTED otherwise); grid (1, K)
int launch_pop_resident(const CoreArgs& a, const PopArgs& p, const PopResidentArgs& r, bool fast, hipStream_t st);

// the step between two episodes of a call with a control block (k_pop_retire): the non-finite scan of theta and w, in mixed
// precision the range predicate of report_sep_range and the learner's status word -> state 2; after_episode: episodes_run += 1,
// |theta - theta_prev| < stop_criteria -> state 1, theta_prev = theta (0, before the first episode: the checks and theta_prev)
void launch_pop_retire(const mfg_pop_control_t& c, const double* theta, const double* w, int64_t F, const double* shift, bool mixed,
                       bool after_episode, hipStream_t st);

}  // namespace mfg
