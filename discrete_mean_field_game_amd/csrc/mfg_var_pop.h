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

// m_max: the largest regressor count of the K models (sizes the tile grid of k_var_gram)
void launch_var_fit(const mfg_var_fit_t& f, int m_max, hipStream_t st);

}  // namespace mfg
