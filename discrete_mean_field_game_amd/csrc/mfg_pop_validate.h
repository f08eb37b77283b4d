// Held-out validation inside a population training call (mfg_ctx_set_pop_validate, include/mfg_hip.h): every `period`
// episodes the call enqueues the launches of mfg_evaluate_pop on the learners' current theta, with with_score those of
// mfg_forecast_score on the members just rolled out, and k_pop_validate_select, which keeps the curve row, the best iterate
// and the patience counter of each learner on the device.  Nothing is read back by the host.
//   k_pop_validate_select, grid K, one wave per learner (as k_pop_retire): lane 0 forms the row -- the eight metrics, and the
//   hour means of the score summary added in hour order in fp64 --, writes it while the curve has room, and decides; on an
//   improvement all 64 lanes copy the learner's w (lanes strided over F) and lane 0 stores theta and the counters.  A learner
//   whose state is not 0 returns before it reads anything.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mfg_hip.h"
#include "mfg_evaluate_pop.h"
#include "mfg_forecast_score.h"

namespace mfg {

// workspace of a validation block (byte offsets, each a multiple of 256):
// [mfg_evaluate_pop's workspace with the members inside | metrics [K,8] | with_score: crps [K,N,L,d] fp64 | less, equal
//  [K,N,L,d] int32 | energy [K,N,L] | summary [K,L,2] | mfg_forecast_score's workspace]
struct PopValidateLayout {
  size_t eval_bytes, metrics, crps, less, equal, energy, summary, score_ws, score_ws_bytes, bytes;
};
inline PopValidateLayout pop_validate_layout(int64_t N, int L, int d, int K, int repeats, bool with_score) {
  const auto up = [](size_t b) { return (b + 255) / 256 * 256; };
  PopValidateLayout o{};
  o.eval_bytes = eval_pop_workspace_bytes(N, L, d, K, repeats, false);
  o.metrics = up(o.eval_bytes);
  o.bytes = o.metrics + up((size_t)K * 8 * 8);
  if (with_score) {
    const size_t cells = (size_t)K * (size_t)N * (size_t)L;
    o.crps = o.bytes;
    o.less = o.crps + up(cells * d * 8);
    o.equal = o.less + up(cells * d * 4);
    o.energy = o.equal + up(cells * d * 4);
    o.summary = o.energy + up(cells * 8);
    o.score_ws = o.summary + up((size_t)K * L * 2 * 8);
    o.score_ws_bytes = forecast_score_workspace_bytes(N, L, K);
    o.bytes = o.score_ws + up(o.score_ws_bytes);
  }
  return o;
}

// Learner k's ten-column row of a check, r[0 .. 9]: the eight metrics, and the hour means of the score summary added in hour
// order in fp64 (NaN without a summary).  ONE definition for k_pop_validate_select, which writes the row, and for the evolve
// step (mfg_pop_evolve.h), which ranks the learners by one of its columns: the same bits in both.
__device__ __forceinline__ void pop_validate_row(const mfg_pop_validate_t& v, const double* __restrict__ metrics,
                                                 const double* __restrict__ summary, int k, double* r) {
#pragma unroll
  for (int q = 0; q < 8; ++q) r[q] = metrics[(int64_t)k * 8 + q];
  r[8] = r[9] = NAN;
  if (summary) {
    double s0 = 0.0, s1 = 0.0;
    for (int l = 1; l < v.L; ++l) {  // (hour 0 is the start row: every member equals the observation there)
      s0 += summary[((int64_t)k * v.L + l) * 2];
      s1 += summary[((int64_t)k * v.L + l) * 2 + 1];
    }
    r[8] = s0 / (double)(v.L - 1);
    r[9] = s1 / (double)(v.L - 1);
  }
}

// state: the control block's [K] activity states, or NULL (every learner is active; patience is then 0).  metrics [K,8];
// summary [K,L,2] or NULL (columns 8, 9 are NaN); theta [K], w [K,F]: the call's parameters at the check.
void launch_pop_validate_select(const mfg_pop_validate_t& v, int32_t* state, const double* metrics, const double* summary,
                                const double* theta, const double* w, int64_t F, hipStream_t st);

}  // namespace mfg
