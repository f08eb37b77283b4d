// The decision step of a held-out check inside a population training call (mfg_pop_validate.h) and the host-only workspace
// query of the validation block.
#include "mfg_pop_validate.h"

namespace mfg {

constexpr int PV_WAVE = 64;
constexpr int PV_COLS = MFG_POP_VALIDATE_COLUMNS;

// ---- one wave, learner blockIdx.x ----
__global__ __launch_bounds__(PV_WAVE) void k_pop_validate_select(mfg_pop_validate_t v, int32_t* __restrict__ state,
                                                                 const double* __restrict__ metrics,
                                                                 const double* __restrict__ summary,
                                                                 const double* __restrict__ theta, const double* __restrict__ w,
                                                                 int64_t F) {
  const int k = blockIdx.x, lane = threadIdx.x;
  if (state && state[k] != 0) return;  // (wave-uniform: none of the learner's arrays is touched)
  const int row = v.checks[k];
  double val = NAN;
  if (lane == 0) {
    double r[PV_COLS];
    pop_validate_row(v, metrics, summary, k, r);
    if (row >= 0 && row < v.max_checks) {
      double* out = v.curve + ((int64_t)k * v.max_checks + row) * PV_COLS;
#pragma unroll
      for (int q = 0; q < PV_COLS; ++q) out[q] = r[q];
    }
    v.checks[k] = row + 1;
#pragma unroll
    for (int q = 0; q < PV_COLS; ++q)
      if (q == v.column) val = r[q];
  }
  // strictly smaller: the earliest minimum wins; a NaN or infinite value never becomes the best
  const bool better = __any(lane == 0 && isfinite(val) && val < v.best_value[k]);
  if (better) {
    for (int64_t j = lane; j < F; j += PV_WAVE) v.best_w[F * k + j] = w[F * k + j];
    if (lane == 0) {
      v.best_value[k] = val;
      v.best_check[k] = row;
      v.best_theta[k] = theta[k];
      v.since_best[k] = 0;
    }
  } else if (lane == 0) {
    const int s = v.since_best[k] + 1;
    v.since_best[k] = s;
    if (state && v.patience > 0 && s >= v.patience) state[k] = 1;  // (stopped, as the early stop of k_pop_retire)
  }
}

void launch_pop_validate_select(const mfg_pop_validate_t& v, int32_t* state, const double* metrics, const double* summary,
                                const double* theta, const double* w, int64_t F, hipStream_t st) {
  hipLaunchKernelGGL(k_pop_validate_select, dim3((unsigned)v.K), dim3(PV_WAVE), 0, st, v, state, metrics, summary, theta, w, F);
}

}  // namespace mfg

using namespace mfg;

extern "C" size_t mfg_pop_validate_workspace_bytes(int64_t N, int L, int d, int K, int repeats, int with_score) {
  if (N < 1 || L < 1 || d < 1 || K < 1 || repeats < 1) return 0;
  return pop_validate_layout(N, L, d, K, repeats, with_score != 0).bytes;
}
