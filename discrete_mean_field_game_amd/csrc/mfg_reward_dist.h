// Reward distributions and mean actions (mfg_row_distribution, mfg_action_mean_pop; contract in include/mfg_hip.h): the numbers
// behind the reference's reward-distribution and action-heatmap figures (ac_irl.py:1046-1375), for K learners at once.
//   k_row_distribution, grid (R): one block per row.  Pass 1 finds a non-finite value, min and max (fp32, exact); pass 2 the
//     mean; pass 3 the variance and the histogram (LDS counts, unsigned LDS atomics: integers, so the order does not matter);
//     then the KDE: thread t owns grid points t, t + BLOCK, ... and adds the N terms of each in ascending n, the values staged
//     through LDS as fp64 in tiles of RD_TILE.  Sums over n: thread t adds values t, t + BLOCK, ... in that order, the BLOCK
//     thread sums are folded by a binary tree in LDS -- an order that depends on N alone.
//   k_action_mean_partial, grid (chunks, K) and k_action_mean_fold, grid (ceil(d d / AM_FOLD_E), K): see action_mean_chunks.
// No floating-point atomics anywhere: a row's / learner's outputs depend on its own inputs only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mfg_hip.h"

namespace mfg {

constexpr int RD_BLOCK = 256;
constexpr int RD_TILE = 1024;  // values per LDS tile of the KDE (8 KB as fp64)

// Chunks of k_action_mean_partial: AM_ROWS matrices each (the fp64 partial row written per chunk is then 1/16 of the bytes
// read) up to AM_MAX_CHUNKS chunks, longer chunks beyond.  A function of N alone.
constexpr int AM_ROWS = 32;
constexpr int AM_MAX_CHUNKS = 1024;
constexpr int AM_FLIGHT = 8;  // loads a thread of the two kernels keeps in flight
// k_action_mean_fold: a block is AM_FOLD_S runs of chunks x AM_FOLD_E elements (128 contiguous bytes per run and chunk)
constexpr int AM_FOLD_E = 16;
constexpr int AM_FOLD_S = RD_BLOCK / AM_FOLD_E;
inline int action_mean_chunks(int64_t N) {
  const int64_t c = (N + AM_ROWS - 1) / AM_ROWS;
  return (int)(c < AM_MAX_CHUNKS ? c : AM_MAX_CHUNKS);
}
inline int64_t action_mean_rows(int64_t N) {
  const int64_t c = action_mean_chunks(N);
  return (N + c - 1) / c;
}
inline size_t action_mean_workspace_bytes(int K, int64_t N, int d) {
  return (size_t)K * (size_t)action_mean_chunks(N) * (size_t)d * (size_t)d * sizeof(double);
}

struct RowDistArgs {
  const float* values;
  int64_t N, stride;
  int bins, use_range, G;
  double lo, hi, x_lo, x_hi;
  double bw_factor;  // N^(-1/5) squared, as gaussian_kde forms it (host pow: the same for every row)
  double* moments;
  int64_t* counts;
  double* edges;
  double* density;
  int32_t* status;
};

void launch_row_distribution(const RowDistArgs& a, int R, hipStream_t st);
void launch_action_mean(const float* action, int64_t s_action, int K, int64_t N, int d, double* mean, double* partials,
                        hipStream_t st);

}  // namespace mfg
