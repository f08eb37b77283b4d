// The two kernels of a population-based-training step inside a population training call (mfg_pop_evolve.h).
#include "mfg_pop_evolve.h"

#include "mfg_device.h"

namespace mfg {

constexpr int PE_WAVE = 64;
constexpr int PE_TILE = 256;  // threads of a rank block = keys of an LDS tile (256 x 8 bytes = 2 KB)

// learner k's value at the check: column v.column of the row k_pop_validate_select formed; a non-finite value counts as +inf
// (the key (value not finite, value, k) of include/mfg_hip.h with one comparison less)
__device__ __forceinline__ double evolve_key(const mfg_pop_validate_t& v, const double* metrics, const double* summary, int k) {
  double r[MFG_POP_VALIDATE_COLUMNS];
  pop_validate_row(v, metrics, summary, k, r);
  double val = NAN;
#pragma unroll
  for (int q = 0; q < MFG_POP_VALIDATE_COLUMNS; ++q)
    if (q == v.column) val = r[q];
  return isfinite(val) ? val : INFINITY;
}

// ---- rank by counting: thread t of block b owns learner 256 b + t ----
// A tile holds 256 keys; the slot of a learner that is not active (or past K) holds NaN, which precedes nothing and equals
// nothing, so the count loop needs no bound check per key: it runs over the tile's keys in groups of 16 (the last group may
// reach into the NaN slots), fully unrolled and without a branch, so that the LDS reads of a group are in flight together.
// With one load, one wait and two branches per key the loop cost 123 us at K = 1 024; this form 36 us, bound by the three
// fp64 compares per key (profiles/pop_evolve.txt).
__global__ __launch_bounds__(PE_TILE) void k_pop_evolve_rank(mfg_pop_evolve_t e, mfg_pop_validate_t v, PopEvolveArgs a) {
  __shared__ double s_key[PE_TILE];
  const int tid = threadIdx.x, K = e.K;
  const int k = blockIdx.x * PE_TILE + tid;
  const bool mine = k < K && (!a.state || a.state[k] == 0);
  const double my = mine ? evolve_key(v, a.metrics, a.summary, k) : INFINITY;
  int before = 0, total = 0;
  // (no return inside: every thread of the block reaches every barrier, with or without a learner of its own)
  for (int t0 = 0; t0 < K; t0 += PE_TILE) {
    const int j = t0 + tid;
    const bool act = j < K && (!a.state || a.state[j] == 0);
    s_key[tid] = act ? evolve_key(v, a.metrics, a.summary, j) : NAN;
    __syncthreads();
    const int n = K - t0 < PE_TILE ? K - t0 : PE_TILE;
    for (int i0 = 0; i0 < n; i0 += 16) {
#pragma unroll
      for (int u = 0; u < 16; ++u) {  // (every lane reads the same word: an LDS broadcast)
        const double kj = s_key[i0 + u];
        const int lt = kj < my, eq = kj == my, lower = t0 + i0 + u < k;  // (bit operations, not && / ||: no branch per key)
        total += (kj == kj) ? 1 : 0;
        before += lt | (eq & lower);
      }
    }
    __syncthreads();
  }
  if (mine) {  // before < total <= K
    e.rank[(int64_t)k * e.max_steps + a.step] = before;
    e.order[before] = k;
  }
  if (k == 0) e.active[0] = total;
}

// min(max(x, lo), hi)
__device__ __forceinline__ double evolve_clamp(double x, double lo, double hi) { return fmin(fmax(x, lo), hi); }

// ---- exploit and explore: one wave, learner blockIdx.x ----
__global__ __launch_bounds__(PE_WAVE) void k_pop_evolve_apply(mfg_pop_evolve_t e, mfg_pop_validate_t v, PopEvolveArgs a) {
  const int k = blockIdx.x, lane = threadIdx.x;
  if (a.state && a.state[k] != 0) return;  // (wave-uniform: none of the learner's arrays is touched)
  const int64_t slot = (int64_t)k * e.max_steps + a.step;
  const int A = e.active[0], r = e.rank[slot];
  const int64_t F = a.F;
  int donor = k;
  // every lane forms the same decision from the same words: the branch below is wave-uniform
  if (A >= e.n_top + e.n_bottom && r >= A - e.n_bottom &&
      evolve_key(v, a.metrics, a.summary, e.order[e.n_top - 1]) < INFINITY) {
    u32x4 c;
    c.x = EVOLVE_DRAW_ELEM;
    c.y = (uint32_t)a.step;
    c.z = (uint32_t)k;
    c.w = 0u;
    const u32x4 x = philox4x32_10(c, (uint32_t)e.seed, (uint32_t)(e.seed >> 32));
    donor = e.order[(int)(((uint64_t)x.x * (uint64_t)e.n_top) >> 32)];  // a rank < n_top <= A - n_bottom: never a receiver
    for (int64_t j = lane; j < F; j += PE_WAVE) {
      a.w[F * k + j] = a.w[F * donor + j];
      v.best_w[F * k + j] = v.best_w[F * donor + j];
    }
    if (lane == 0) {
      const double th = a.theta[donor];
      a.theta[k] = th;
      if (a.theta_prev) a.theta_prev[k] = th;
      v.best_value[k] = v.best_value[donor];
      v.best_check[k] = v.best_check[donor];
      v.since_best[k] = v.since_best[donor];
      v.best_theta[k] = v.best_theta[donor];
      double lc = e.lr_critic[donor], la = e.lr_actor[donor];
      if (e.perturb & 1) lc = evolve_clamp(lc * ((x.y >> 31) ? e.factor_up : e.factor_down), e.lr_critic_min, e.lr_critic_max);
      if (e.perturb & 2) la = evolve_clamp(la * ((x.z >> 31) ? e.factor_up : e.factor_down), e.lr_actor_min, e.lr_actor_max);
      e.lr_critic[k] = lc;
      e.lr_actor[k] = la;
    }
  }
  if (lane == 0) {  // (the rates lane 0 just stored, or the learner's own)
    e.parent[slot] = donor;
    e.lr_log[slot * 2] = e.lr_critic[k];
    e.lr_log[slot * 2 + 1] = e.lr_actor[k];
  }
}

void launch_pop_evolve(const mfg_pop_evolve_t& e, const mfg_pop_validate_t& v, const PopEvolveArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(k_pop_evolve_rank, dim3((unsigned)((e.K + PE_TILE - 1) / PE_TILE)), dim3(PE_TILE), 0, st, e, v, a);
  hipLaunchKernelGGL(k_pop_evolve_apply, dim3((unsigned)e.K), dim3(PE_WAVE), 0, st, e, v, a);
}

}  // namespace mfg
