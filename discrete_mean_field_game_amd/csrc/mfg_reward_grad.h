// Input gradients of the reward network for the listed learners of a population (mfg_rn_input_grad_t, contract in
// include/mfg_hip.h): the block rides on mfg_reward_net_forward_pop, which calls rn_input_grad_check before it launches
// anything and launch_rn_input_grad behind its reward launch.
//   k_rn_input_grad<D>, grid (N, list slots), 256 threads: one block per (sample, slot).  The forward pass of
//     k_rn_train_sample (mfg_reward_train.hip) at the matrix-core geometry (k1 = 5, f2 = 2, k2 = 3, D = 15 / 21 at compile
//     time) with every activation in LDS, then the chain to the INPUTS, which the training kernel does not have: tanh' ->
//     FC4^T (split into dh3 and grad_state) -> FC3^T (thread i owns FC3 inputs i, i + 256, ...: the n3 weight rows are read
//     coalesced) -> ReLU -> transposed 3x3 convolution over the two channels -> ReLU -> transposed 5x5 convolution.  Both
//     transposed convolutions read zero-padded LDS images of the upstream derivative with the taps flipped.  About 20 KB of
//     LDS per block at D = 21.
//   k_rn_grad_mean_partial, grid (chunks, slots) and k_rn_grad_mean_fold, grid (ceil(2 E / 256), slots), E = d + d d: the
//     fp64 means of the gradient and of gradient x input over mfg_action_mean_pop's chunking of N (action_mean_chunks,
//     mfg_reward_dist.h).  One thread per element adds its chunk in ascending n, one thread per element adds the chunk totals
//     in chunk order: no atomics, an order that depends on N alone.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mfg_hip.h"
#include "mfg_reward_dist.h"

namespace mfg {

constexpr int RG_BLOCK = 256;
constexpr int RG_MAXN3 = 16, RG_MAXN4 = 32;

// workspace of a block: per-sample arrays [K,N,E] fp32 (learner k's at k N E: independent of the list) | chunk totals
// [K,chunks,2,E] fp64
struct RnGradLayout {
  size_t samples, partials, bytes;
};
inline RnGradLayout rn_input_grad_layout(int K, int64_t N, int d) {
  const size_t E = (size_t)d + (size_t)d * (size_t)d;
  RnGradLayout L;
  L.samples = 0;
  L.partials = ((size_t)K * (size_t)N * E * sizeof(float) + 7) & ~(size_t)7;
  L.bytes = L.partials + (size_t)K * (size_t)action_mean_chunks(N) * 2 * E * sizeof(double);
  return L;
}

// what mfg_reward_net_forward_pop hands over: its inputs, the network its launch was set up with, its uploaded list
struct RnGradCall {
  const float *state, *action;
  int64_t s_state, s_action, N;
  int d, K, n;
  mfg_reward_net_t net;          // the launch's (with a geometry table: row 0's base and the table's maxima)
  int per_learner_net;
  int64_t s_net;
  const mfg_rn_geom_t* geom;     // [K] device or NULL
  const uint64_t* key;           // [n] device, by slot
  const int32_t* learner;        // [n] device
  uint64_t sample_offset;
};

// the block of the calling thread's bound context; NULL without a context or a block (mfg_kernels.hip)
const mfg_rn_input_grad_t* bound_rn_input_grad();
// MFG_OK, or the refusal of a block that does not fit the call (error recorded); nothing is launched or written
int rn_input_grad_check(const mfg_rn_input_grad_t& b, int K, int64_t N, int d);
// the three launches, on st
int launch_rn_input_grad(const mfg_rn_input_grad_t& b, const RnGradCall& c, hipStream_t st);

}  // namespace mfg
