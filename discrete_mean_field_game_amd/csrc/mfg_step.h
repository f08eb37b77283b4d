// The given-P env step (a3 + a4: pi' = pi P and the in-kernel reward), mfg_step.hip: the k_step_* kernels and the rule that
// chooses between them.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mfg {

// B >= 1, 1 <= d <= MFG_MAX_D, reward_kind an MFG_REWARD_* value (MFG_REWARD_EXTERNAL: `reward` is not written and may be
// NULL): checked by the caller.  Returns MFG_OK or the code recorded for mfg_last_error().
int launch_step_given_P(const float* pi, const float* P, int64_t B, int d, int reward_kind, float* pi_next, float* reward,
                        hipStream_t st);

}  // namespace mfg
