// Population-based training inside a population training call (mfg_ctx_set_pop_evolve, include/mfg_hip.h): behind every
// `every`-th held-out check the call enqueues two launches that rank the active learners by the check's value, let the worst
// take over the parameters of one of the best and perturb their learning rates.  Nothing is read back by the host.
//   k_pop_evolve_rank, grid ceil(K / 256) x 256 threads: rank by counting.  Thread t of block b owns the key of learner
//   256 b + t; the K keys stream through LDS in tiles of 256 (2 KB; the slot of a learner that is not active holds NaN) and
//   a thread counts the active keys that precede its own.  The thread of learner 0 also counts all active keys and writes
//   active[0].  O(K^2) comparisons, no atomics.  No thread returns before the last barrier: a thread without a learner, or
//   with a retired one, counts along and stores nothing.
//   k_pop_evolve_apply, grid K, one wave per learner (as k_pop_validate_select): a learner whose state is not 0 returns before
//   it reads anything (wave-uniform); a receiver's 64 lanes copy the donor's w and best_w (lanes strided over F), lane 0 the
//   scalars, the rates and the log entries.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mfg_hip.h"
#include "mfg_pop_validate.h"

namespace mfg {

constexpr uint32_t EVOLVE_DRAW_ELEM = 0xFFFFFFFEu;  // (outside the action draws' element ids and START_DRAW_ELEM)

// the arrays of the call and of its other two blocks that a step reads or writes
struct PopEvolveArgs {
  const int32_t* state;   // the control block's [K] states, or NULL (every learner is active)
  double* theta_prev;     // the control block's, or NULL
  const double* metrics;  // [K,8] of the check, in the validation workspace
  const double* summary;  // [K,L,2] of the check, or NULL
  double* theta;          // [K]
  double* w;              // [K,F]
  int64_t F;
  int32_t step;           // s
};

// metrics / summary are those of the check the step follows; s < e.max_steps (checked by the caller).
void launch_pop_evolve(const mfg_pop_evolve_t& e, const mfg_pop_validate_t& v, const PopEvolveArgs& a, hipStream_t st);

}  // namespace mfg
