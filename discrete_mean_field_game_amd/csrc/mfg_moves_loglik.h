// Dirichlet-multinomial likelihood of K policies on counted moves (mfg_moves_loglik_pop; include/mfg_hip.h).
//   k_ml_rows   a thread per row (data set s, day n, transition h, topic i): the multinomial coefficient of the row,
//               lgamma(n_i + 1) - sum_j lgamma(m_j + 1), summed in column order -- it does not depend on the policy, so it is
//               formed once per call, not once per policy.  NaN marks a row with a negative move or a non-finite state.
//   k_ml_cells  grid (transitions, policy chunks) x 256: a lane per (policy, row i), 64 / d policies to a wavefront (three at
//               d = 21, four at d = 15: 63 and 60 of 64 lanes at work).  The lane walks the d cells of its row in column
//               order: softplus, T and D of the cell (ml_td), the running A, n_i and gradient sums; then T and D of (A, n_i).
//               The rows of a policy meet in LDS (5 KiB) and are added by the lane of row 0 in the order i = 0 .. d - 1: the
//               same additions wherever the policy sits.  Writes ll [K,N,H-1], grad [K,N,H-1,3] and the transition's flags.
//   k_ml_days   a thread per (policy, day): ll_day, grad_day and status from the per-transition values, h = 0 .. H - 2 in order.
// Workspace: [coef fp64 [S, N, H-1, d] | flags int32 [K, N, H-1]], each section rounded up to 256 bytes; every word the call
// reads is written by the call first.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace mfg {

constexpr int ML_THREADS = 256;
constexpr int ML_WAVES = ML_THREADS / 64;
constexpr int ML_MAX_D = 64;
constexpr int ML_SMALL_M = 8;              // T and D of m <= 8 are the finite sums themselves
constexpr int ML_SERIES_MIN = 16;          // the asymptotic series are used at a >= 16 (short recurrence below)
constexpr double ML_PRODUCT_MAX = 1e30;    // the product of 8 factors below this stays finite

inline size_t ml_up(size_t bytes) { return (bytes + 255) / 256 * 256; }

struct MlWs {
  double* coef;
  int32_t* flags;
  size_t bytes;
};

inline MlWs ml_layout(void* base, int policies, int sets, int N, int H, int d) {
  char* p = reinterpret_cast<char*>(base);
  MlWs w;
  size_t at = 0;
  w.coef = reinterpret_cast<double*>(p + at), at += ml_up((size_t)sets * N * (H - 1) * d * 8);
  w.flags = reinterpret_cast<int32_t*>(p + at), at += ml_up((size_t)policies * N * (H - 1) * 4);
  w.bytes = at;
  return w;
}

}  // namespace mfg
