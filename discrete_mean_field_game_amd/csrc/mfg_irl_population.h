// IRL populations (mfg_train_episodes_irl_pop / mfg_train_rollouts_irl_pop): K independent forward learners of AC_IRL.train served
// by every launch of an episode, as mfg_population.h describes.  The core kernel and the closing row reduction are the population
// kernels of mfg_population.hip; this header declares the argument block of the reward network's population form
// (k_reward_net_mfma_pop, mfg_reward_net.hip, launched by reward_net_forward_sums with an RnPop): grid (the single call's grid for
// Bk, K), learner = blockIdx.y, plain over a rollout's pi_traj or SUMS with the TD error.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mfg_core.h"

namespace mfg {

// the reward network's per-learner strides: states / actions / outputs, the learner's key, and its weights (per_learner_net:
// learner k's tensor t at base_t + k numel_t, numel_t from the geometry, or at base_t + k s_net when s_net > 0; 0: shared).
// Key of learner k: key[slot] when given, else rn_seed[k] ^ ((call_base[k] + call_j) 0x9E3779B97F4A7C15) when call_base is
// given (per-learner reward-call counters), else rn_seed[k] ^ key_ctr.  Grid rows: n_y slots, slot -> learner[slot] when
// learner is given (0 / NULL: K rows, slot = learner).
struct RnPop {
  int K;
  int per_learner_net;
  int64_t s_state, s_action, s_n, s_next, s_w;  // elements
  int64_t s_ws;                                  // bytes (part_rows, col_f: in the learner's workspace slice)
  const uint64_t* rn_seed;
  uint64_t key_ctr;                              // (no host call sets it any more: the training calls always give call_base)
  int64_t s_net;                                 // elements between two learners' weights (0: numel_t per tensor)
  const uint64_t* call_base;                     // [K] device (NULL: the shared key_ctr)
  uint64_t call_j;
  const uint64_t* key;                           // [n_y] device, by slot (NULL: from rn_seed)
  const int32_t* learner;                        // [n_y] device (NULL: slot = learner)
  int n_y;
  const mfg_rn_geom_t* geom;                     // [K] device (NULL: the launch's n3 / n4 / keep_prob for every learner)
  const int32_t* state;                          // [K] device, training flows with a control block (mfg_population.h): the
                                                 // blocks of a learner whose state is not 0 return at once (NULL: all run)
};

// Per-learner geometry (the optional table, include/mfg_hip.h): learner k's entry is read by its blocks -- block-uniform,
// one 16-byte scalar load -- before they run the single kernel's body with its n3 / n4 / keep_prob (/ l1l2).  Learner k's ten
// tensors are one flat row, at the offsets of rt_layout(d, 5, 2, 3, n3_k, n4_k) from row_base + k net_stride; the launch's own
// n3 / n4 are the table's maxima and size the dynamic LDS and the workspace slices only.
typedef const __attribute__((address_space(4))) mfg_rn_geom_t* RnGeomConst;  // read-only global memory: a scalar load
__device__ __forceinline__ mfg_rn_geom_t rn_geom_entry(const mfg_rn_geom_t* geom, int k) {
  RnGeomConst g = (RnGeomConst)geom + k;
  mfg_rn_geom_t e;
  e.n3 = g->n3; e.n4 = g->n4; e.keep_prob = g->keep_prob; e.l1l2 = g->l1l2;
  return e;
}

// the checks a geometry table adds, before anything is launched (0, or the MFG_E* code with the message in `why`): both copies
// given, one row per learner with room for the longest, every entry inside the matrix-core kernel's limits.  n3_max / n4_max /
// np_max: the largest n3, n4 and parameter count of the table.
int rn_geom_check(const mfg_rn_geom_t* geom_host, const mfg_rn_geom_t* geom_dev, int K, int d, int k1, int f2, int k2,
                  int per_learner_net, int64_t net_stride, int* n3_max, int* n4_max, int64_t* np_max, const char** why);
// ... and the network the launches of such a population are set up with: conv1_w = the base of row 0, the other pointers at the
// offsets of the LARGEST geometry (n3 / n4 = the table's maxima: LDS and workspace sizes), keep_prob 1; sets the error on refusal
int rn_pop_nets_struct(const mfg_reward_net_t* net, const mfg_rn_geom_t* geom_host, const mfg_rn_geom_t* geom_dev, int K, int d,
                       int per_learner_net, int64_t net_stride, mfg_reward_net_t* out);

// true: K learners' networks of this geometry (fc3_w of every learner 8-byte aligned) run the matrix-core kernel
// (net_stride > 0: learner k's tensors at base + k net_stride; 0: the numel_t strides)
bool reward_net_pop_ready(int d, const mfg_reward_net_t* net, int per_learner_net, int K, int64_t net_stride = 0);

}  // namespace mfg
