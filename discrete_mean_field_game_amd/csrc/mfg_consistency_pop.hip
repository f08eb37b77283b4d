// Backward-equation check kernels (mfg_consistency_pop.h): the reverse-time scan with the two consistency metrics per hour,
// and their reduction per group.  The rollouts of mfg_consistency_pop are launch_eval_rollout_pop's (mfg_evaluate_pop.hip).
#include "mfg_core.h"
#include "mfg_consistency_pop.h"

namespace mfg {

// ---- the scan of trajectory b = one wave (mfg_synthetic.py:768-790, :858-880; formulas of k_backward_value) ----
// LDS of wave wv (consistency_wave_lds(d) bytes): tile [d, d] fp32 = P^n as it lies in HBM, then two [d] fp64 vectors that
// take turns as V^{n+1} and V^n.  Lane = (row i, part s) = (lane / L, lane mod L), L = consistency_lanes(d); lanes >= d L
// have no column (their loops are empty and their terms 0) but take part in every cross-lane step.  A row's L partial sums
// are read from the row's lanes in lane order by each of them (the same bits in all L); sums over rows go through wave_sum.
// Barriers are wave local: a wave reads only what its own lanes wrote.
__global__ __launch_bounds__(BLOCK) void k_consistency_backward(const float* __restrict__ P, int64_t B, int T, int d, int L,
                                                                double* __restrict__ V, double* __restrict__ steps) {
  extern __shared__ __attribute__((aligned(16))) double cs_lds[];
  const int lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x / WAVE, nwv = blockDim.x / WAVE;
  const int dd = d * d;
  char* base = reinterpret_cast<char*>(cs_lds) + (size_t)wv * consistency_wave_lds(d);
  float* tile = reinterpret_cast<float*>(base);
  double* va = reinterpret_cast<double*>(base + ((size_t)dd * 4 + 7) / 8 * 8);
  double* vb = va + d;
  const bool on = lane < d * L;
  const int i = on ? lane / L : 0;
  const int s = on ? lane - i * L : d;  // first column of this lane (d: none)
  const int r0 = on ? i * L : lane;     // first lane of the row
  const bool head = on && s == 0;
  const float* row = tile + i * d;
  const int64_t nw = (int64_t)gridDim.x * nwv;
  for (int64_t b = (int64_t)blockIdx.x * nwv + wv; b < B; b += nw) {
    double* vn1 = va;  // V^{n+1}
    double* vn = vb;   // V^{n}
    __builtin_amdgcn_wave_barrier();
    for (int c = lane; c < d; c += WAVE) {
      vn1[c] = 0.0;
      if (V) V[(b * (T + 1) + T) * d + c] = 0.0;
    }
    for (int n = T - 1; n >= 0; --n) {
      const float* __restrict__ Pn = P + (b * T + n) * (int64_t)dd;
      for (int e = lane; e < dd; e += WAVE) tile[e] = Pn[e];
      __builtin_amdgcn_s_waitcnt(0xc07f);
      __builtin_amdgcn_wave_barrier();
      // V^n_i = -1/2 sum_j P_ij^2 + sum_j P_ij V^{n+1}_j
      double r2 = 0.0, acc = 0.0;
      for (int j = s; j < d; j += L) {
        const double p = (double)row[j];
        r2 = fma(p, p, r2);
        acc = fma(p, vn1[j], acc);
      }
      double R2 = 0.0, A = 0.0;
      for (int u = 0; u < L; ++u) {
        R2 += __shfl(r2, r0 + u, WAVE);
        A += __shfl(acc, r0 + u, WAVE);
      }
      const double vi = fma(-0.5, R2, A);
      if (head) {
        vn[i] = vi;
        if (V) V[(b * (T + 1) + n) * d + i] = vi;
      }
      const double sumV = wave_sum(head ? vi : 0.0);
      __builtin_amdgcn_s_waitcnt(0xc07f);
      __builtin_amdgcn_wave_barrier();
      // implied row i: V^n_j - V^n_i off the diagonal, 1 - (sum V - d V_i) on it
      const double diag = 1.0 - (sumV - (double)d * vi);
      double l1 = 0.0, sp = 0.0, sq = 0.0;
      for (int j = s; j < d; j += L) {
        const double p = (double)row[j];
        const double val = (j == i) ? diag : vn[j] - vi;
        l1 += fabs(p - val);
        sp += (p <= 0.0) ? 1e-100 : p;
        sq += (val <= 0.0) ? 1e-100 : val;
      }
      double SP = 0.0, SQ = 0.0;
      for (int u = 0; u < L; ++u) {
        SP += __shfl(sp, r0 + u, WAVE);
        SQ += __shfl(sq, r0 + u, WAVE);
      }
      const double sm = 0.5 * (SP + SQ);
      double kl = 0.0;
      for (int j = s; j < d; j += L) {
        double p = (double)row[j];
        double q = (j == i) ? diag : vn[j] - vi;
        if (p <= 0.0) p = 1e-100;
        if (q <= 0.0) q = 1e-100;
        const double m = 0.5 * (p + q) / sm;
        const double pn = p / SP, qn = q / SQ;
        kl += pn * log(pn / m) + qn * log(qn / m);
      }
      l1 = wave_sum(l1);
      const double js = wave_sum(0.5 * kl);
      if (lane == 0) {
        steps[(b * T + n) * 2] = l1;
        steps[(b * T + n) * 2 + 1] = js;
      }
      __builtin_amdgcn_wave_barrier();  // (the next hour overwrites the tile and V^{n+1})
      double* t = vn1;
      vn1 = vn;
      vn = t;
    }
  }
}

void launch_consistency_backward(const float* P, int64_t B, int T, int d, double* V, double* steps, int num_cus, hipStream_t st) {
  const int nwv = consistency_waves(d);
  int64_t g = (B + nwv - 1) / nwv;
  const int64_t cap = (int64_t)num_cus * CONSISTENCY_BLOCKS_PER_CU;
  if (g > cap) g = cap;
  hipLaunchKernelGGL(k_consistency_backward, dim3((unsigned)g), dim3(nwv * WAVE), (size_t)nwv * consistency_wave_lds(d), st, P, B, T, d,
                     consistency_lanes(d), V, steps);
}

// ---- mean and std (ddof = 0) of group blockIdx.x's MT values of each metric, two passes in a fixed order ----
__device__ __forceinline__ void consistency_block_sum(double& a, double& b, double (*part)[2]) {
  const int lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x / WAVE;
  a = wave_sum(a);
  b = wave_sum(b);
  __syncthreads();  // (part is reused)
  if (lane == 0) {
    part[wv][0] = a;
    part[wv][1] = b;
  }
  __syncthreads();
  a = b = 0.0;
  for (int w = 0; w < WAVES; ++w) {
    a += part[w][0];
    b += part[w][1];
  }
}

__global__ __launch_bounds__(BLOCK) void k_consistency_reduce(const double* __restrict__ steps_all, int64_t MT,
                                                              double* __restrict__ metrics) {
  __shared__ double part[WAVES][2];
  const int k = blockIdx.x;
  const double2* __restrict__ st = reinterpret_cast<const double2*>(steps_all) + (int64_t)k * MT;
  double s0 = 0.0, s1 = 0.0;
  for (int64_t e = threadIdx.x; e < MT; e += BLOCK) {
    const double2 v = st[e];
    s0 += v.x;
    s1 += v.y;
  }
  consistency_block_sum(s0, s1, part);
  const double m0 = s0 / (double)MT, m1 = s1 / (double)MT;
  double q0 = 0.0, q1 = 0.0;
  for (int64_t e = threadIdx.x; e < MT; e += BLOCK) {
    const double2 v = st[e];
    const double d0 = v.x - m0, d1 = v.y - m1;
    q0 += d0 * d0;
    q1 += d1 * d1;
  }
  consistency_block_sum(q0, q1, part);
  if (threadIdx.x == 0) {
    double* out = metrics + (int64_t)k * 4;
    out[0] = m0;
    out[1] = sqrt(q0 / (double)MT);
    out[2] = m1;
    out[3] = sqrt(q1 / (double)MT);
  }
}

void launch_consistency_reduce(const double* steps, int K, int64_t MT, double* metrics, hipStream_t st) {
  hipLaunchKernelGGL(k_consistency_reduce, dim3((unsigned)K), dim3(BLOCK), 0, st, steps, MT, metrics);
}

}  // namespace mfg
