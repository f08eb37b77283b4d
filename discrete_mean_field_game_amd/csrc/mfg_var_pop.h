// The VAR baseline as a population (mfg_var_fit_pop, include/mfg_hip.h): K independent vector autoregressions, each with its own
// lag, ridge and day lists, in three launches.
//   k_var_gram      grid (16x16 tiles, K): G = Z'Z + lambda I (lower triangle) and Z'Y, one element per thread, t ascending.  The
//                   rows of Z are read straight from the day table through the model's day list; Z is never materialised.
//   k_var_solve     one workgroup per model: right-looking Cholesky in 16-wide panels on the model's slice of the workspace
//                   (the diagonal block in LDS, the panel a row per thread, the trailing update an element per thread); the d
//                   right-hand sides are d more rows of the same matrix, so the forward substitution is the panel solve and the
//                   trailing update; then the back substitution panel by panel.  Only this workgroup touches the slice:
//                   __syncthreads orders it.
//   k_var_forecast  one workgroup per model: the non-finite scan, the fitted rows with the in-sample sums, the S-step recursion
//                   (sequential in s; a dot product is 16 strided partial sums added in order), the per-step L1 / JSD on one
//                   wave (xor butterfly), the per-day values, their mean and std.
// A model's slice: [64 bytes: the pivot word | W (m + d) x m fp64, row-major: rows < m the lower triangle of G, then L; rows
// m + j the column j of Z'Y, then of L^-1 Z'Y].  Every word that is read was written by this call: the contents are scratch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mfg_hip.h"

namespace mfg {

constexpr int VAR_MAX_M = MFG_VAR_MAX_REGRESSORS;
constexpr int VAR_MAX_D = 64, VAR_MAX_H = 64, VAR_MAX_DAYS = 64;
constexpr int VAR_PANEL = 16;
constexpr size_t VAR_HEAD_BYTES = 64;

inline size_t var_model_bytes(int m, int d) { return (VAR_HEAD_BYTES + (size_t)(m + d) * (size_t)m * 8 + 255) / 256 * 256; }

// ---- device functions shared with the RNN baseline (mfg_rnn_pop.hip): the day clamp and the L1 / JSD of one row
// a day index is clamped into the table before it addresses anything: k_var_forecast reports the model, nothing is read outside
__device__ __forceinline__ int var_day(int idx, int D) { return idx < 0 ? 0 : (idx >= D ? D - 1 : idx); }

__device__ __forceinline__ double var_wave_sum(double x) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) x += __shfl_xor(x, off);
  return x;
}

// one wave (k_var_forecast: wave 0; the RNN kernels: a row per wave): ||yo - yh||_1 and JSD(yo, yh) of one row (var.py:175-192), every sum an xor butterfly over the 64 lanes
__device__ __forceinline__ void var_row_metrics(const double* yo, const double* yh, int d, double& l1, double& jsd) {
  const int j = threadIdx.x & 63;
  const bool on = j < d;
  const double P = on ? yo[j] : 0.0, Q = on ? yh[j] : 0.0;
  l1 = var_wave_sum(on ? fabs(P - Q) : 0.0);
  const double Pf = on ? (P <= 0.0 ? 1e-100 : P) : 0.0, Qf = on ? (Q <= 0.0 ? 1e-100 : Q) : 0.0;
  const double Mf = 0.5 * (Pf + Qf);
  const double sP = var_wave_sum(Pf), sQ = var_wave_sum(Qf), sM = var_wave_sum(Mf);
  double term = 0.0;
  if (on) {
    const double pk = Pf / sP, qk = Qf / sQ, mk = Mf / sM;
    term = pk * log(pk / mk) + qk * log(qk / mk);
  }
  jsd = 0.5 * var_wave_sum(term);
}

// m_max: the largest regressor count of the K models (sizes the tile grid of k_var_gram)
void launch_var_fit(const mfg_var_fit_t& f, int m_max, hipStream_t st);

}  // namespace mfg
