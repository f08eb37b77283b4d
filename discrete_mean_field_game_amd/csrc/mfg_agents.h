// Finite-population members (mfg_agents_step_pop, mfg_forecast_agents_pop; contract in include/mfg_hip.h): a member is a
// population of A agents whose state is the integer histogram counts [d]; in one step every agent of topic i draws its next
// topic from row P[i,:] of the member's action, so the histogram carries the sampling noise of order 1 / sqrt(A) that the
// mean-field step pi' = P^T pi leaves out (the N-player game behind the mean-field limit).
//   k_agents_step, grid (B, K), one workgroup per member, no workspace:
//     phase 1: the thresholds t_ic = floor(S_ic / S_i,d-1 2^32) of the sequential fp64 row sums S_ic, clamped to [0, 2^32].
//       Thread i adds up row i in column order (adds only) and leaves every S_ic in LDS, column-major so that the d threads
//       hit d banks; all threads divide; thread i takes the running maxima.  (A wave per row, every lane repeating the row's
//       d adds on broadcast values, made the forecast's 15 launches take 8.7 instead of 4.5 ms at A = 1 000: the thresholds
//       then cost more than the agents.)  A row with agents and a sum that is not finite or <= 0, or a count outside [0, A],
//       fails the member.  LDS gets the
//       running maxima u_c = max(t_0 .. t_c) that lie below 2^32, as 32-bit words, and their number: "the first column with
//       w < t_c" is the first with w < u_c, u ascends, so the column is the NUMBER of u_c <= w (and t = 2^32 needs no 33rd
//       bit: a word that passes every stored threshold lands in the first column whose threshold is 2^32).
//     phase 2: the rows' agents in chunks of 256 (64 Philox blocks, a lane per block, its words x, y, z, w the agents 4 q ..
//       4 q + 3), the chunks of all rows dealt to the four waves in turn.  A lane places its four agents by four branch-free
//       binary searches side by side over the row's thresholds in LDS (log2 d steps of one read, one compare, one select;
//       a row's thresholds are consecutive words, so lanes that read different ones hit different banks) and counts each
//       with one LDS integer atomic on moves[i,c]: integers, so the order does not matter.  An earlier form counted a column at
//       a time with compare-ballot-popcount over the wave (d x 4 64-bit compares per chunk and thrice as much scalar work): it
//       ran the d = 21 forecast's step at 0.40x this one's rate (profiles/forecast_agents.txt).
//     phase 3: counts'_c = sum_i moves[i,c], the histogram row (float)((double)counts' / (double)A), the copies of moves and P.
//   k_agents_init (the forecast's row 0): the start counts, their histogram row and the sampler's input row of every member.
// The forecast alternates the population sampling kernel (launch_eval_rollout_pop, T = 1, over all K N R members, reading the
// members' current rows) with k_agents_step: 2 (H - 1) launches whatever K is, then mfg_forecast_pop's reduction and curves.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mfg_hip.h"
#include "mfg_evaluate_pop.h"

namespace mfg {

// One launch of k_agents_step.  Strided arrays: member (k, b)'s row starts at base + k s_k + b s_m elements.
struct AgentsArgs {
  const int32_t* counts;  // [d] per member
  int64_t cs_k, cs_m;
  const float* P;         // [K, B, d, d]
  int32_t* counts_next;   // [d] per member
  int64_t ns_k, ns_m;
  float* pi_next;         // [d] per member, or NULL
  int64_t ps_k, ps_m;
  float* pi_cur;          // [K, B, d] or NULL: as pi_next, but left alone for a failed member (the sampler's next input)
  int32_t* moves;         // [K, B, d, d] or NULL
  float* P_copy;          // [d, d] per member, or NULL: the member's action, copied
  int64_t as_k, as_m;
  const uint64_t* seed;   // [K]
  int64_t B;
  int d, agents;
  uint32_t step;
  uint64_t traj_offset;
};

// LDS of one k_agents_step block: the fp64 row sums [d, d] (then the moves, int32, in their place), the rows' last sums [d]
// fp64, the thresholds [d, d] and the rows' agents and threshold counts [d], 32 bits each (49 KB at d = 64, 5.5 KB at d = 21)
inline size_t agents_lds_bytes(int d) { return (size_t)d * d * 12 + (size_t)d * 16; }

void launch_agents_step(const AgentsArgs& a, int K, hipStream_t st);
void launch_agents_init(const int32_t* counts0, int64_t N, int64_t NR, int H, int d, int K, int agents, int32_t* counts_traj,
                        float* pi_traj, float* pi_cur, hipStream_t st);

// workspace layout of mfg_forecast_agents_pop: [idx tables | per-member per-step (L1, JSD) [K][H][N R][2] fp64 | the members'
// current rows [K][N R][d] fp32 | the step's actions [K][N R][d][d] fp32 | pi_traj if not given | counts_traj if not given],
// every part padded to 8 bytes
inline size_t agents_pad8(size_t b) { return (b + 7) / 8 * 8; }
inline size_t forecast_agents_workspace_bytes(int64_t N, int H, int d, int K, int repeats, bool traj_given, bool counts_given) {
  const size_t NR = (size_t)N * (size_t)repeats, Ks = (size_t)K;
  size_t b = Ks * (size_t)eval_pop_idx_stride((int64_t)NR) * 4 + Ks * (size_t)H * NR * 2 * 8;
  b += agents_pad8(Ks * NR * d * 4) + agents_pad8(Ks * NR * d * d * 4);
  if (!traj_given) b += agents_pad8(Ks * NR * H * d * 4);
  if (!counts_given) b += agents_pad8(Ks * NR * H * d * 4);
  return b;
}

}  // namespace mfg
