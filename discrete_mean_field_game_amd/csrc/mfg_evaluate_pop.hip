// Population evaluation kernels (mfg_evaluate_pop.h): the test rollouts of K policies (the packed core kernel's body on an
// argument block rebased per learner) and their L1 / JSD metrics, reduced per learner in a fixed order.
#include "mfg_core.h"
#include "mfg_evaluate_pop.h"

namespace mfg {

// ---- launch 1: the N R test rollouts of learner blockIdx.y ----
// (strict precision: two waves per SIMD -- at the single kernel's three the body spills 12 .. 296 bytes per lane, and an
//  evaluation launch is far too small to need the occupancy)
template <bool FAST, int D>
__global__ __launch_bounds__(BLOCK, FAST ? MFG_CORE_SMALL_WAVES : 2) void k_eval_rollout_pop(CoreArgs a, PopArgs p) {
  const int k = blockIdx.y;
  // a check inside a training call with a control block (mfg_pop_validate.h): a retired learner's blocks return at once
  // (block-uniform, ahead of every barrier); mfg_evaluate_pop itself passes no states
  if (p.state && pop_retired(p, k)) return;
  const int d = D ? D : a.d;
  const int TB = WAVES * (WAVE / d);
  int32_t* idx = p.idx + p.s_idx * k;
  // start rows of this block's tiles (blockIdx.x + m gridDim.x): the only entries core_small_body reads, its prefetch of the
  // next tile included.  Trajectory j starts at row (j mod N) L of emp32 viewed as [N L, d], i.e. emp32[j mod N, 0] (a
  // forecast, mfg_forecast_pop.h, passes its start rows [N, d] with L = 1).
  for (int64_t b0 = (int64_t)blockIdx.x * TB; b0 < a.B; b0 += (int64_t)gridDim.x * TB) {
    const int64_t b = b0 + threadIdx.x;
    if (threadIdx.x < TB && b < a.B) idx[b] = (int32_t)((b % p.N) * p.L);
  }
  __threadfence();  // (written by other waves of the block than the ones that read them; each learner's table has lines of its own)
  __syncthreads();
  CoreArgs c = pop_core_args<false, 0>(a, p, k);
  c.start_idx = idx;
  if (p.state) c.status = p.status + k;  // (as the _ctl training forms: an out-of-range theta is booked to the learner)
  core_small_body<true, false, FAST, D, false, 0>(c);
}

template <bool FAST, int D>
static void go_eval(const CoreArgs& a, const PopArgs& p, int num_cus, size_t lds, hipStream_t st) {
  const int grid = core_small_grid<k_eval_rollout_pop<FAST, D>>(a, lds, num_cus);
  hipLaunchKernelGGL((k_eval_rollout_pop<FAST, D>), dim3((unsigned)grid, (unsigned)p.K), dim3(BLOCK), lds, st, a, p);
}

int launch_eval_rollout_pop(const CoreArgs& a, const PopArgs& p, bool fast, int num_cus, hipStream_t st) {
  const int d = a.d;
  if (d > WAVE) return MFG_EUNSUPPORTED;
  const size_t lds = core_small_lds(d, false, true);
  if (d == 21) {
    if (fast) go_eval<true, 21>(a, p, num_cus, lds, st);
    else go_eval<false, 21>(a, p, num_cus, lds, st);
  } else if (d == 15) {
    if (fast) go_eval<true, 15>(a, p, num_cus, lds, st);
    else go_eval<false, 15>(a, p, num_cus, lds, st);
  } else {
    if (fast) go_eval<true, 0>(a, p, num_cus, lds, st);
    else go_eval<false, 0>(a, p, num_cus, lds, st);
  }
  return MFG_OK;
}

// ---- launch 2: the eight metrics of learner blockIdx.x (mfg_ac2.py:631-666) ----
// Wave wv walks trajectories j = wv, wv + WAVES, ...; lane i holds state entry i (d <= 64).  Per step: L1 = sum_i |emp64 -
// gen| in fp64, JSD with k_jsd's formula (zeros -> 1e-100, M from the un-normalised vectors, P, Q, M renormalised).  Lane 0
// keeps the trajectory's four values (final row, mean over the L rows), writes them to per_traj and reads them back itself for
// the second pass of the standard deviation.  Wave totals are combined in wave order: a fixed summation order.
__global__ __launch_bounds__(BLOCK) void k_eval_metrics_pop(const float* __restrict__ gen_all, const float* __restrict__ emp32,
                                                            const double* __restrict__ emp64, int64_t N, int L, int d, int64_t NR,
                                                            double* __restrict__ per_traj_all, double* __restrict__ metrics,
                                                            const int32_t* __restrict__ state) {
  __shared__ double part[WAVES][4];
  __shared__ double mean_s[4];
  const int k = blockIdx.x;
  if (state && state[k] != 0) return;  // (a retired learner of a validation check: its row of metrics is left alone)
  const int lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x / WAVE;
  const float* gen = gen_all + (int64_t)k * NR * L * d;
  double* per_traj = per_traj_all + (int64_t)k * NR * 4;
  const bool on = lane < d;
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  for (int64_t j = wv; j < NR; j += WAVES) {
    const int64_t n = j % N;
    double l1_sum = 0.0, jsd_sum = 0.0, l1 = 0.0, jsd = 0.0;
    for (int l = 0; l < L; ++l) {
      const int64_t eo = (n * L + l) * d + lane;
      eval_step_l1_jsd(gen + (j * L + l) * d + lane, emp32, emp64, eo, on, l1, jsd);
      l1_sum += l1;
      jsd_sum += jsd;
    }
    const double v[4] = {l1, l1_sum / L, jsd, jsd_sum / L};
    if (lane == 0) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        per_traj[j * 4 + q] = v[q];
        s[q] += v[q];
      }
    }
  }
  if (lane == 0)
    for (int q = 0; q < 4; ++q) part[wv][q] = s[q];
  __syncthreads();
  if (threadIdx.x < 4) {
    double t = 0.0;
    for (int w = 0; w < WAVES; ++w) t += part[w][threadIdx.x];
    mean_s[threadIdx.x] = t / (double)NR;
  }
  __syncthreads();
  double ss[4] = {0.0, 0.0, 0.0, 0.0};
  if (lane == 0) {
    for (int64_t j = wv; j < NR; j += WAVES)
      for (int q = 0; q < 4; ++q) {
        const double dv = per_traj[j * 4 + q] - mean_s[q];
        ss[q] += dv * dv;
      }
  }
  __syncthreads();  // (part is reused)
  if (lane == 0)
    for (int q = 0; q < 4; ++q) part[wv][q] = ss[q];
  __syncthreads();
  if (threadIdx.x < 4) {
    double t = 0.0;
    for (int w = 0; w < WAVES; ++w) t += part[w][threadIdx.x];
    metrics[(int64_t)k * 8 + 2 * threadIdx.x] = mean_s[threadIdx.x];
    metrics[(int64_t)k * 8 + 2 * threadIdx.x + 1] = sqrt(t / (double)NR);
  }
}

void launch_eval_metrics_pop(const float* pi_traj, const float* emp32, const double* emp64, int64_t N, int L, int d, int64_t NR,
                             int K, double* per_traj, double* metrics, hipStream_t st, const int32_t* state) {
  hipLaunchKernelGGL(k_eval_metrics_pop, dim3((unsigned)K), dim3(BLOCK), 0, st, pi_traj, emp32, emp64, N, L, d, NR, per_traj,
                     metrics, state);
}

}  // namespace mfg
