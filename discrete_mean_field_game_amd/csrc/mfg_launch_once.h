// Launchers of the launch-once kernels (mfg_launch_once.hip) that more than one caller runs; the kernels with a C entry
// point of their own need no declaration here.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mfg_population.h"

namespace mfg {

// (w, theta) += lr G / count in place (k_apply_update), and out of place (k_apply_update_oop)
void launch_apply_update(const double* G, int d, double lr_c, double lr_a, double* w, double* theta, double* reward_acc,
                         hipStream_t st);
void launch_apply_update_oop(const double* G, int d, double lr_c, double lr_a, const double* w_in, const double* theta_in,
                             double* w_out, double* theta_out, double* reward_acc, hipStream_t st);

// the start-state draw (k_draw_start): idx[b] and / or the gathered rows out[b]
void launch_draw_start(const float* mat, int64_t num_start, int64_t B, int d, uint64_t seed, uint32_t step, uint64_t traj_offset,
                       int32_t* idx, float* out, hipStream_t st);

// the row reduction + update that closes a step-mode episode (population: learner k's theta_in at k pop->s_theta_b bytes);
// slots: the two theta slots of the workspace's control block (population: learner k's at k pop->s_ws bytes), left zero
void launch_reduce_rows_apply(const double* rows, int nrows, int64_t FO, double* G, double lr_c, double lr_a, double count,
                              double* w, const double* theta_in, double* theta_out, double* reward_acc, double* slots,
                              hipStream_t st, const PopArgs* pop);

}  // namespace mfg
