// Ensemble forecast kernels (mfg_forecast_pop.h): the reduction of R members per cell to mean, std and order statistics, and
// the per-step error curves.  The rollouts themselves are launch_eval_rollout_pop's (mfg_evaluate_pop.hip).
#include "mfg_core.h"
#include "mfg_forecast_pop.h"

namespace mfg {

struct ForecastReduceArgs {
  const float* traj;  // [K, N R, H, d]
  int64_t N;
  int H, d, R, P2, C, Q;  // P2: power of two >= R; C: columns per chunk (forecast_chunk)
  ForecastRanks ranks;
  double *mean, *std;  // [K, N, H, d]
  float* quant;        // [K, N, H, Q, d]
};

// ---- launch 2: mean, std and Q order statistics of cell (k, n, l) = (blockIdx.y, blockIdx.x / H, blockIdx.x mod H) ----
// LDS image: column c of the chunk at fc_col + c (P2 + FC_PAD), member r at [r], +inf at [R, P2).  Thread e of the load loop
// takes entry (r, c) = (e / C, e mod C): consecutive lanes read consecutive floats of one member row and write LDS words
// P2 + FC_PAD apart -- bank (c + r) mod 32 with FC_PAD = 1, distinct within a row.
// A column belongs to ONE wave from the moments to the copy of the order statistics; the barriers inside the sort only order
// that wave's own LDS writes and reads (every wave runs every step, idle ones with nothing to do, so they are uniform).
__global__ __launch_bounds__(BLOCK) void k_forecast_reduce(ForecastReduceArgs a) {
  extern __shared__ float fc_col[];
  const int k = blockIdx.y;
  const int64_t cell = blockIdx.x;
  const int64_t n = cell / a.H;
  const int l = (int)(cell - n * a.H);
  const int lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x / WAVE;
  const int R = a.R, P2 = a.P2, d = a.d, Q = a.Q, stride = P2 + FC_PAD;
  // member r of the cell is trajectory j = r N + n of learner k
  const float* __restrict__ base = a.traj + (((int64_t)k * a.N * R + n) * a.H + l) * d;
  const int64_t mstride = a.N * a.H * d;
  const int64_t ocell = (int64_t)k * a.N * a.H + cell;
  int rk = 0;  // lane q < Q copies order statistic ranks[q]
#pragma unroll
  for (int q = 0; q < MFG_FORECAST_MAX_RANKS; ++q)
    if (lane == q) rk = a.ranks.r[q];
  for (int c0 = 0; c0 < d; c0 += a.C) {
    const int C = min(a.C, d - c0);
    for (int e = threadIdx.x; e < R * C; e += BLOCK) {
      const int r = e / C, c = e - r * C;
      fc_col[c * stride + r] = base[r * mstride + c0 + c];
    }
    if (Q > 0 && P2 > R) {
      const int pad = P2 - R;
      for (int e = threadIdx.x; e < pad * C; e += BLOCK) {
        const int c = e / pad, p = e - c * pad;
        fc_col[c * stride + R + p] = INFINITY;
      }
    }
    __syncthreads();
    for (int cb = 0; cb < C; cb += WAVES) {
      const int ci = cb + wv;
      const bool active = ci < C;
      float* col = fc_col + (active ? ci : 0) * stride;
      if (active) {
        // two passes in fp64 over the members in member order (ahead of the sort, which reorders them)
        double s = 0.0;
        for (int r = lane; r < R; r += WAVE) s += (double)col[r];
        const double mean = wave_sum(s) / (double)R;
        double ss = 0.0;
        for (int r = lane; r < R; r += WAVE) {
          const double dv = (double)col[r] - mean;
          ss += dv * dv;
        }
        const double var = wave_sum(ss) / (double)R;
        if (lane == 0) {
          a.mean[ocell * d + c0 + ci] = mean;
          a.std[ocell * d + c0 + ci] = sqrt(var);
        }
      }
      if (Q > 0) {
        // bitonic sort, ascending: step (kk, j) compares entries i and i | j, i the t-th index with bit j clear
        for (int kk = 2; kk <= P2; kk <<= 1)
          for (int j = kk >> 1; j > 0; j >>= 1) {
            if (active)
              for (int t = lane; t < (P2 >> 1); t += WAVE) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), p = i | j;
                const float x = col[i], y = col[p];
                if ((i & kk) == 0 ? x > y : x < y) {
                  col[i] = y;
                  col[p] = x;
                }
              }
            __syncthreads();
          }
        if (active && lane < Q) a.quant[(ocell * Q + lane) * d + c0 + ci] = col[rk];
      }
    }
    __syncthreads();  // (the next chunk's load overwrites the columns)
  }
}

int launch_forecast_reduce(const float* pi_traj, int64_t N, int H, int d, int K, int repeats, const ForecastRanks& ranks, int Q,
                           double* mean, double* std, float* quant, hipStream_t st) {
  ForecastReduceArgs a{};
  a.traj = pi_traj;
  a.N = N;
  a.H = H;
  a.d = d;
  a.R = repeats;
  a.P2 = forecast_p2(repeats);
  a.C = forecast_chunk(d, repeats);
  a.Q = Q;
  a.ranks = ranks;
  a.mean = mean;
  a.std = std;
  a.quant = quant;
  const size_t lds = forecast_lds_bytes(d, repeats);
  if (a.C < 1 || lds > FC_LDS_BUDGET) return MFG_ELAUNCH;  // (never within MFG_FORECAST_MAX_REPEATS: a column takes 4 100 B there)
  hipLaunchKernelGGL(k_forecast_reduce, dim3((unsigned)(N * H), (unsigned)K), dim3(BLOCK), lds, st, a);
  return MFG_OK;
}

// ---- launch 3: mean and std over the N R members of the step's L1 and JSD, block (l, k) ----
// k_eval_metrics_pop's scheme on one step, with FC_CURVE_WAVES waves (a block has all N R members of its step to itself, and
// the launch has only K H blocks: 16 waves per block took the curves from 0.66 to 0.34 ms at K = 16, N = 6, R = 256): wave wv
// walks members j = wv, wv + FC_CURVE_WAVES, ..., lane 0 keeps the member's two values, writes them to per_step and reads them
// back itself for the second pass; wave totals are combined in wave order.
constexpr int FC_CURVE_WAVES = 16;
constexpr int FC_CURVE_BLOCK = FC_CURVE_WAVES * WAVE;
__global__ __launch_bounds__(FC_CURVE_BLOCK) void k_forecast_curves(const float* __restrict__ gen_all,
                                                                    const float* __restrict__ emp32,
                                                                    const double* __restrict__ emp64, int64_t N, int H, int d,
                                                                    int64_t NR, double* __restrict__ per_step_all,
                                                                    double* __restrict__ curves) {
  __shared__ double part[FC_CURVE_WAVES][2];
  __shared__ double mean_s[2];
  const int l = blockIdx.x, k = blockIdx.y;
  const int lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x / WAVE;
  const float* gen = gen_all + (int64_t)k * NR * H * d;
  double* per = per_step_all + ((int64_t)k * H + l) * NR * 2;
  const bool on = lane < d;
  double s[2] = {0.0, 0.0};
  for (int64_t j = wv; j < NR; j += FC_CURVE_WAVES) {
    const int64_t n = j % N;
    double l1, jsd;
    eval_step_l1_jsd(gen + (j * H + l) * d + lane, emp32, emp64, (n * H + l) * d + lane, on, l1, jsd);
    if (lane == 0) {
      per[j * 2] = l1;
      per[j * 2 + 1] = jsd;
      s[0] += l1;
      s[1] += jsd;
    }
  }
  if (lane == 0)
    for (int q = 0; q < 2; ++q) part[wv][q] = s[q];
  __syncthreads();
  if (threadIdx.x < 2) {
    double t = 0.0;
    for (int w = 0; w < FC_CURVE_WAVES; ++w) t += part[w][threadIdx.x];
    mean_s[threadIdx.x] = t / (double)NR;
  }
  __syncthreads();
  double ss[2] = {0.0, 0.0};
  if (lane == 0) {
    for (int64_t j = wv; j < NR; j += FC_CURVE_WAVES)
      for (int q = 0; q < 2; ++q) {
        const double dv = per[j * 2 + q] - mean_s[q];
        ss[q] += dv * dv;
      }
  }
  __syncthreads();  // (part is reused)
  if (lane == 0)
    for (int q = 0; q < 2; ++q) part[wv][q] = ss[q];
  __syncthreads();
  if (threadIdx.x < 2) {
    double t = 0.0;
    for (int w = 0; w < FC_CURVE_WAVES; ++w) t += part[w][threadIdx.x];
    double* out = curves + ((int64_t)k * H + l) * 4 + 2 * threadIdx.x;
    out[0] = mean_s[threadIdx.x];
    out[1] = sqrt(t / (double)NR);
  }
}

void launch_forecast_curves(const float* pi_traj, const float* emp32, const double* emp64, int64_t N, int H, int d, int64_t NR,
                            int K, double* per_step, double* curves, hipStream_t st) {
  hipLaunchKernelGGL(k_forecast_curves, dim3((unsigned)H, (unsigned)K), dim3(FC_CURVE_BLOCK), 0, st, pi_traj, emp32, emp64, N, H, d, NR,
                     per_step, curves);
}

}  // namespace mfg
