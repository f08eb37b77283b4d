// Batch sums of the actor-critic update and the critic values of a whole rollout (mfg_batch_sums.hip).  The two share the
// workspace of a call: [control block | partial rows of the sums | V of the large-d rollouts].
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "mfg_grad.h"
#include "mfg_population.h"

namespace mfg {

constexpr size_t MFG_WS_CONTROL_BYTES = 64;  // control block at the START of the workspace (completion counter), kept zero:
                                              // a fixed place, whatever N a call is made with; partial rows follow it
constexpr int MFG_GRAD_FUSE_MAX_ROWS = 32;   // in-kernel finalisation up to this many partial rows

struct ApplyArgs {
  double lr_c, lr_a;
  double *w, *theta, *reward_acc;
};

// Large-d rollouts evaluate the critic values of all states in one matrix-core pass after the rollout (k_value_mfma): room
// for V[B (T+1)] <= 2 N doubles behind the partial rows of the gradient sums.
bool value_batch_ok(int d);
size_t value_buffer_bytes(int64_t N, int d);

// samples staged per iteration, partial rows (<= the workspace cap) and output blocks of the batch sums over N samples
void grad_geometry(int64_t N, int d, int* chunk, int64_t* nsb, int* nob);

// G = [sum delta phi | sum delta g | sum r | N] over N = B T samples.  `apply` (optional): also perform the parameter
// update; *applied tells whether it was done in-kernel.  pop: the population form (mfg_population.h).
int launch_grad(const float* pi, int64_t stride_b, const double* delta, const double* g, const float* reward, int64_t N, int T,
                int d, double* G, int accumulate, void* ws, size_t ws_bytes, hipStream_t st, const ApplyArgs* apply = nullptr,
                bool* applied = nullptr, bool add_reward = false, const PopArgs* pop = nullptr);

// the fixed-order row reduction (+ update) on its own, over rows that another kernel left (k_reduce_partials)
void launch_reduce_partials(const double* partial, int64_t nsb, int64_t FO, int accumulate, double* G, const ReduceApply& ap,
                            hipStream_t st);

// After a TD rollout that skipped the in-kernel values (large d): V of all B (T+1) states, then delta.
int launch_values_and_delta(const float* pi_traj, int64_t B, int T, int d, const double* w, const float* reward, double gamma,
                            int discount_pow, double* delta, void* ws, size_t ws_bytes, hipStream_t st);

}  // namespace mfg
