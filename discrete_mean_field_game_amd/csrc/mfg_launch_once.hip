// The launch-once kernels for MI355X (gfx950 / CDNA4, wave64): one elementwise or wave-per-row pass each, none of them on
// the training path's critical loop.  Start states (gather, draw), the policy's alpha, the critic's features and value, the
// Dirichlet normalisation, raw Philox words, the parameter update, the closing row reduction of a step-mode episode, and the
// evaluation metrics (JSD, policy log-density, backward value recursion).  A kernel that only its own C entry point launches
// sits next to that entry point; the others have a launcher in mfg_launch_once.h.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mfg_hip.h"
#include "mfg_core.h"
#include "mfg_host.h"
#include "mfg_launch_once.h"
#include "mfg_population.h"

using namespace mfg;

// ---------------------------------------------------------------------------------------------
// trivial kernels: gather, alpha, features, dirichlet_from_gamma, philox_raw, apply_update
// ---------------------------------------------------------------------------------------------
__global__ void k_gather_start(const float* __restrict__ mat, int64_t num_start, const int32_t* __restrict__ idx, int64_t B,
                               int d, float* __restrict__ out) {
  const int64_t n = B * d;
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t b = e / d;
    const int j = (int)(e - b * d);
    out[e] = mat[start_row(idx[b], num_start) * d + j];
  }
}

// a9: the start-state draw itself (start_draw_row, mfg_device.h) as a launch of its own: idx[b] and / or the gathered rows
// (draw_start_body, mfg_core.h)
__global__ void k_draw_start(const float* __restrict__ mat, int64_t num_start, int64_t B, int d, uint64_t seed, uint32_t step,
                             uint64_t traj_offset, int32_t* __restrict__ idx_out, float* __restrict__ out) {
  draw_start_body(mat, num_start, B, d, seed, step, traj_offset, idx_out, out);
}

__global__ void k_alpha(const float* __restrict__ pi, int64_t B, int d, const double* __restrict__ theta_p,
                        double shift, double* __restrict__ alpha, double* __restrict__ deriv) {
  const double theta = *theta_p;
  const int64_t dd = (int64_t)d * d;
  const int64_t n = B * dd;
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t b = e / dd;
    const int r = (int)(e - b * dd);
    const int i = r / d, j = r - i * d;
    const double x = (double)pi[b * d + j] - (double)pi[b * d + i] - shift;
    double sp, sg;
    softplus_sigmoid(theta * x, sp, sg);
    if (alpha) alpha[e] = sp;
    if (deriv) deriv[e] = x * sg;
  }
}

__global__ void k_features(const float* __restrict__ pi, int64_t B, int d, double* __restrict__ phi) {
  const int64_t dd = (int64_t)d * d;
  const int64_t F = (int64_t)d * (d + 1) / 2 + d + 1;
  const int64_t Q = (int64_t)d * (d + 1) / 2;
  const int64_t n = B * dd;
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t b = e / dd;
    const int r = (int)(e - b * dd);
    const int i = r / d, j = r - i * d;
    const double pi_i = (double)pi[b * d + i], pi_j = (double)pi[b * d + j];
    if (j >= i) phi[b * F + feat_idx(i, j, d)] = pi_i * pi_j;
    if (i == 0) phi[b * F + Q + j] = pi_j;
    if (r == 0) phi[b * F + Q + d] = 1.0;
  }
}

__global__ void k_dirichlet_from_gamma(const float* __restrict__ y, int64_t rows, int d, float* __restrict__ P) {
  // one wavefront per row of gamma variates
  const int lane = threadIdx.x & (WAVE - 1);
  const int64_t wave = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) / WAVE;
  const int64_t nw = (int64_t)gridDim.x * blockDim.x / WAVE;
  for (int64_t r = wave; r < rows; r += nw) {
    double s = 0.0;
    for (int j = lane; j < d; j += WAVE) {
      float v = y[r * d + j];
      if (v == 0.0f) v = ZERO_GAMMA_REPLACEMENT;
      s += (double)v;
    }
    s = wave_sum(s);
    const double inv = 1.0 / s;
    for (int j = lane; j < d; j += WAVE) {
      float v = y[r * d + j];
      if (v == 0.0f) v = ZERO_GAMMA_REPLACEMENT;
      P[r * d + j] = (float)((double)v * inv);
    }
  }
}

__global__ void k_philox_raw(uint64_t seed, uint32_t first, uint32_t c1, uint32_t c2, uint32_t c3, int64_t n,
                             uint32_t* __restrict__ out) {
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
    u32x4 c{first + (uint32_t)e, c1, c2, c3};
    const u32x4 r = philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
    out[4 * e + 0] = r.x;
    out[4 * e + 1] = r.y;
    out[4 * e + 2] = r.z;
    out[4 * e + 3] = r.w;
  }
}

__global__ void k_apply_update(const double* __restrict__ G, int64_t F, double lr_c, double lr_a, double* __restrict__ w,
                               double* __restrict__ theta, double* __restrict__ reward_acc) {
  const double count = G[F + 2];
  if (!(count > 0.0)) return;
  const double inv = 1.0 / count;
  if (reward_acc && blockIdx.x == 0 && threadIdx.x == 0) *reward_acc += G[F + 1] * inv;
  for (int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; k < F; k += (int64_t)gridDim.x * blockDim.x)
    w[k] = updated_param(w[k], lr_c, G[k], inv);
  if (blockIdx.x == 0 && threadIdx.x == 0) *theta = updated_param(*theta, lr_a, G[F], inv);
}

// the same update out of place: (w_out, theta_out) = (w_in, theta_in) + lr G / count -- the large-d form of the deferred
// update of mfg_train_rollout_deferred (at d <= 64 the rollout kernel applies it while staging its weights)
__global__ void k_apply_update_oop(const double* __restrict__ G, int64_t F, double lr_c, double lr_a, const double* __restrict__ w_in,
                                   const double* __restrict__ theta_in, double* __restrict__ w_out, double* __restrict__ theta_out,
                                   double* __restrict__ reward_acc) {
  const double count = G[F + 2];
  const bool on = count > 0.0;
  const double inv = on ? 1.0 / count : 0.0;
  if (on && reward_acc && blockIdx.x == 0 && threadIdx.x == 0) *reward_acc += G[F + 1] * inv;
  for (int64_t k = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; k < F; k += (int64_t)gridDim.x * blockDim.x)
    w_out[k] = on ? updated_param(w_in[k], lr_c, G[k], inv) : w_in[k];
  if (blockIdx.x == 0 && threadIdx.x == 0) *theta_out = on ? updated_param(*theta_in, lr_a, G[F], inv) : *theta_in;
}

// ---------------------------------------------------------------------------------------------
// a11: JSD, one wavefront per pair of rows
// ---------------------------------------------------------------------------------------------
__global__ void k_jsd(const float* __restrict__ p, const float* __restrict__ q, int64_t B, int d, double* __restrict__ out) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int64_t wave = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) / WAVE;
  const int64_t nw = (int64_t)gridDim.x * blockDim.x / WAVE;
  for (int64_t b = wave; b < B; b += nw) {
    // zeros -> 1e-100, M = (P+Q)/2 from the un-normalised vectors, entropy() renormalises P, Q and M
    double sp = 0, sq = 0;
    for (int j = lane; j < d; j += WAVE) {
      double a = p[b * d + j], c = q[b * d + j];
      if (a == 0.0) a = 1e-100;
      if (c == 0.0) c = 1e-100;
      sp += a;
      sq += c;
    }
    sp = wave_sum(sp);
    sq = wave_sum(sq);
    const double sm = 0.5 * (sp + sq);
    double acc = 0;
    for (int j = lane; j < d; j += WAVE) {
      double a = p[b * d + j], c = q[b * d + j];
      if (a == 0.0) a = 1e-100;
      if (c == 0.0) c = 1e-100;
      const double m = 0.5 * (a + c) / sm;
      const double pn = a / sp, qn = c / sq;
      acc += pn * log(pn / m) + qn * log(qn / m);
    }
    acc = wave_sum(acc);
    if (lane == 0) out[b] = 0.5 * acc;
  }
}

// ---------------------------------------------------------------------------------------------
// f1 (importance weights of the max-ent IRL loss, ac_irl.py:270-289 calc_pdf_action / :324-379 calc_z): log-density of
// the product-Dirichlet policy, one wavefront per (sample n, policy k):
//   log q_k(P_n | pi_n) = sum_i [ lgamma(sum_j a_ij) - sum_j lgamma(a_ij) + sum_j (a_ij - 1) ln P_ij ],
//   a_ij = max(alpha_floor, alpha_scale * ln(1 + exp(theta_k (pi_j - pi_i - shift)))).
// Log space replaces the reference's divide-by-normaliser trick (pdf / c before the products).  fp64 throughout.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void k_policy_logpdf(const float* __restrict__ pi, const float* __restrict__ P, int64_t N,
                                                         int d, const double* __restrict__ thetas, int K, double shift,
                                                         double alpha_scale, double alpha_floor, double p_floor,
                                                         double* __restrict__ out) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int64_t wave = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) / WAVE;
  const int64_t nw = (int64_t)gridDim.x * blockDim.x / WAVE;
  const int dd = d * d;
  for (int64_t u = wave; u < N * K; u += nw) {
    const int64_t n = u / K;
    const int k = (int)(u - n * K);
    const double th = thetas[k];
    const float* pn = pi + n * d;
    const float* Pn = P + n * (int64_t)dd;
    double acc = 0.0;
    for (int e = lane; e < dd; e += WAVE) {
      const int i = e / d, j = e - i * d;
      double sp, sg;
      softplus_sigmoid(th * ((double)pn[j] - (double)pn[i] - shift), sp, sg);
      double al = alpha_scale * sp;
      if (al < alpha_floor) al = alpha_floor;
      double pv = (double)Pn[e];
      if (pv < p_floor) pv = p_floor;
      acc += (al - 1.0) * log(pv) - lgamma(al);
    }
    for (int i = lane; i < d; i += WAVE) {
      double A = 0.0;
      for (int j = 0; j < d; ++j) {
        double sp, sg;
        softplus_sigmoid(th * ((double)pn[j] - (double)pn[i] - shift), sp, sg);
        double al = alpha_scale * sp;
        if (al < alpha_floor) al = alpha_floor;
        A += al;
      }
      acc += lgamma(A);
    }
    acc = wave_sum(acc);
    if (lane == 0) out[u] = acc;
  }
}

// ---------------------------------------------------------------------------------------------
// f3: backward value recursion of mfg_synthetic (mfg_synthetic.py:768-774) and the two consistency metrics
// of evaluate_synthetic (:776-790, sum_ij |P_ij - value_ij|) / evaluate_synthetic_JSD (:858-880, sum_i JSD(P_i,
// implied row i) with entries <= 0 -> 1e-100).  One wavefront per trajectory, lane = row i, reverse-time scan
// with V^{n+1} in LDS.  Evaluation-only: rows are read strided (L2 resident), fp64 throughout.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void k_backward_value(const float* __restrict__ P, int64_t B, int T, int d,
                                                          double* __restrict__ V, double* __restrict__ diff_l1,
                                                          double* __restrict__ diff_jsd) {
  extern __shared__ __attribute__((aligned(16))) double smd[];
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), wv = tid / WAVE;
  double* vn1 = smd + wv * 2 * d;  // V^{n+1}
  double* vn = vn1 + d;            // V^{n}
  const int64_t nw = (int64_t)gridDim.x * WAVES;
  for (int64_t b = (int64_t)blockIdx.x * WAVES + wv; b < B; b += nw) {
    __builtin_amdgcn_wave_barrier();
    for (int i = lane; i < d; i += WAVE) {
      vn1[i] = 0.0;
      V[(b * (T + 1) + T) * d + i] = 0.0;
    }
    __builtin_amdgcn_s_waitcnt(0xc07f);
    __builtin_amdgcn_wave_barrier();
    for (int n = T - 1; n >= 0; --n) {
      const float* Pn = P + (b * T + n) * (int64_t)d * d;
      double sumV = 0.0;
      for (int i = lane; i < d; i += WAVE) {
        const float* row = Pn + (int64_t)i * d;
        double r2 = 0.0, acc = 0.0;
        for (int j = 0; j < d; ++j) {
          const double p = (double)row[j];
          r2 = fma(p, p, r2);
          acc = fma(p, vn1[j], acc);
        }
        const double v = fma(-0.5, r2, acc);
        vn[i] = v;
        V[(b * (T + 1) + n) * d + i] = v;
        sumV += v;
      }
      sumV = wave_sum(sumV);
      __builtin_amdgcn_s_waitcnt(0xc07f);
      __builtin_amdgcn_wave_barrier();
      double l1 = 0.0, js = 0.0;
      for (int i = lane; i < d; i += WAVE) {
        const float* row = Pn + (int64_t)i * d;
        const double vi = vn[i];
        const double diag = 1.0 - (sumV - (double)d * vi);
        double sp = 0.0, sq = 0.0;
        for (int j = 0; j < d; ++j) {
          const double p = (double)row[j];
          const double val = (j == i) ? diag : vn[j] - vi;
          l1 += fabs(p - val);
          sp += (p <= 0.0) ? 1e-100 : p;
          sq += (val <= 0.0) ? 1e-100 : val;
        }
        if (diff_jsd) {
          const double sm = 0.5 * (sp + sq);
          double kl = 0.0;
          for (int j = 0; j < d; ++j) {
            double p = (double)row[j];
            double q = (j == i) ? diag : vn[j] - vi;
            if (p <= 0.0) p = 1e-100;
            if (q <= 0.0) q = 1e-100;
            const double m = 0.5 * (p + q) / sm;
            const double pn = p / sp, qn = q / sq;
            kl += pn * log(pn / m) + qn * log(qn / m);
          }
          js += 0.5 * kl;
        }
      }
      l1 = wave_sum(l1);
      if (diff_jsd) js = wave_sum(js);
      if (lane == 0) {
        diff_l1[b * T + n] = l1;
        if (diff_jsd) diff_jsd[b * T + n] = js;
      }
      __builtin_amdgcn_wave_barrier();
      for (int i = lane; i < d; i += WAVE) vn1[i] = vn[i];
      __builtin_amdgcn_s_waitcnt(0xc07f);
      __builtin_amdgcn_wave_barrier();
    }
  }
}

// ---------------------------------------------------------------------------------------------
// a5: V(pi) = phi(pi).w, one wavefront per trajectory, lanes own columns c, rows i <= c.
// w rows are contiguous in k for fixed i, so the loads are coalesced (L2 resident).
// ---------------------------------------------------------------------------------------------
__global__ void k_value(const float* __restrict__ pi, const double* __restrict__ w, int64_t B, int d,
                        double* __restrict__ out) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int64_t wave = (blockIdx.x * (int64_t)blockDim.x + threadIdx.x) / WAVE;
  const int64_t nw = (int64_t)gridDim.x * blockDim.x / WAVE;
  for (int64_t b = wave; b < B; b += nw) {
    const double v = value_wave(pi + b * d, w, d, lane);
    if (lane == 0) out[b] = v;
  }
}

// The row reduction + update of the IRL env step as a launch of its own (after an episode's LAST step; the other steps' reductions
// ride in the next step kernel, k_core_small<.., STEP>): a wave per column, rows_column_sum -- the same order, the same bits.
__global__ __launch_bounds__(BLOCK) void k_reduce_rows_apply(const double* __restrict__ rows, int nrows, int64_t FO, double* __restrict__ G,
                                                            double lr_c, double lr_a, double count, double* __restrict__ w,
                                                            const double* theta_in, double* theta_out,
                                                            double* __restrict__ reward_acc, double* slots) {
  reduce_rows_apply_body(rows, nrows, FO, G, lr_c, lr_a, count, w, theta_in, theta_out, reward_acc, slots);
}

// ---------------------------------------------------------------------------------------------
// host side: launchers of the kernels with more than one caller
// ---------------------------------------------------------------------------------------------
namespace mfg {

// the update as a launch of its own (where no kernel applied it while it formed G)
void launch_apply_update(const double* G, int d, double lr_c, double lr_a, double* w, double* theta, double* reward_acc,
                         hipStream_t st) {
  const int64_t F = mfg_num_features(d);
  hipLaunchKernelGGL(k_apply_update, dim3((unsigned)((F + 255) / 256)), dim3(256), 0, st, G, F, lr_c, lr_a, w, theta, reward_acc);
}

void launch_apply_update_oop(const double* G, int d, double lr_c, double lr_a, const double* w_in, const double* theta_in,
                             double* w_out, double* theta_out, double* reward_acc, hipStream_t st) {
  const int64_t F = mfg_num_features(d);
  hipLaunchKernelGGL(k_apply_update_oop, dim3((unsigned)((F + 255) / 256)), dim3(256), 0, st, G, F, lr_c, lr_a, w_in, theta_in, w_out,
                     theta_out, reward_acc);
}

void launch_draw_start(const float* mat, int64_t num_start, int64_t B, int d, uint64_t seed, uint32_t step, uint64_t traj_offset,
                       int32_t* idx, float* out, hipStream_t st) {
  hipLaunchKernelGGL(k_draw_start, dim3(grid_for(out ? B * d : B, 256, 8)), dim3(256), 0, st, mat, num_start, B, d, seed, step,
                     traj_offset, idx, out);
}

void launch_reduce_rows_apply(const double* rows, int nrows, int64_t FO, double* G, double lr_c, double lr_a, double count,
                              double* w, const double* theta_in, double* theta_out, double* reward_acc, double* slots,
                              hipStream_t st, const PopArgs* pop) {
  if (pop) launch_reduce_rows_apply_pop(rows, nrows, FO, G, count, w, theta_in, theta_out, reward_acc, slots, *pop, st);
  else hipLaunchKernelGGL(k_reduce_rows_apply, dim3((unsigned)((FO + WAVES - 1) / WAVES)), dim3(BLOCK), 0, st, rows, nrows, FO,
                          G, lr_c, lr_a, count, w, theta_in, theta_out, reward_acc, slots);
}

}  // namespace mfg

// ---------------------------------------------------------------------------------------------
// C ABI: the entry points whose kernel nothing else launches
// ---------------------------------------------------------------------------------------------
extern "C" {

int mfg_gather_start(const float* mat_pi0, int64_t num_start, const int32_t* idx, int64_t B, int d, float* pi0,
                     mfg_stream_t stream) {
  CHECK_BD();
  REQUIRE(mat_pi0 && idx && pi0 && num_start > 0, "null pointer / empty table");
  hipLaunchKernelGGL(k_gather_start, dim3(grid_for(B * d, 256, 8)), dim3(256), 0, S(stream), mat_pi0, num_start, idx, B,
                     d, pi0);
  return check_launch("gather_start");
}

int mfg_alpha(const float* pi, int64_t B, int d, const double* theta, double shift, double* alpha, double* alpha_deriv,
              mfg_stream_t stream) {
  CHECK_BD();
  REQUIRE(pi && theta && (alpha || alpha_deriv), "null pointer");
  hipLaunchKernelGGL(k_alpha, dim3(grid_for(B * d * d, 256, 8)), dim3(256), 0, S(stream), pi, B, d, theta, shift, alpha,
                     alpha_deriv);
  return check_launch("alpha");
}

int mfg_dirichlet_from_gamma(const float* y, int64_t B, int d, float* P, mfg_stream_t stream) {
  CHECK_BD();
  REQUIRE(y && P, "null pointer");
  hipLaunchKernelGGL(k_dirichlet_from_gamma, dim3(grid_for(B * d, WAVES, 8)), dim3(BLOCK), 0, S(stream), y, B * d, d, P);
  return check_launch("dirichlet_from_gamma");
}

int mfg_philox_raw(uint64_t seed, uint32_t first_ctr, uint32_t c1, uint32_t c2, uint32_t c3, int64_t n, uint32_t* out,
                   mfg_stream_t stream) {
  REQUIRE(n >= 0 && (out || n == 0), "null pointer");
  if (n == 0) return MFG_OK;
  hipLaunchKernelGGL(k_philox_raw, dim3(grid_for(n, 256, 8)), dim3(256), 0, S(stream), seed, first_ctr, c1, c2, c3, n, out);
  return check_launch("philox_raw");
}

int mfg_value(const float* pi, const double* w, int64_t B, int d, double* value, mfg_stream_t stream) {
  CHECK_BD();
  REQUIRE(pi && w && value, "null pointer");
  hipLaunchKernelGGL(k_value, dim3(grid_for(B, WAVES, 8)), dim3(BLOCK), 0, S(stream), pi, w, B, d, value);
  return check_launch("value");
}

int mfg_features(const float* pi, int64_t B, int d, double* phi, mfg_stream_t stream) {
  CHECK_BD();
  REQUIRE(pi && phi, "null pointer");
  hipLaunchKernelGGL(k_features, dim3(grid_for(B * d * d, 256, 8)), dim3(256), 0, S(stream), pi, B, d, phi);
  return check_launch("features");
}

int mfg_backward_value(const float* P, int64_t B, int T, int d, double* V, double* diff_l1, double* diff_jsd,
                       mfg_stream_t stream) {
  CHECK_BD();
  REQUIRE(T >= 1, "T < 1");
  REQUIRE(P && V && diff_l1, "null pointer");
  hipLaunchKernelGGL(k_backward_value, dim3(grid_for(B, WAVES, 8)), dim3(BLOCK), (size_t)WAVES * 2 * d * 8, S(stream), P,
                     B, T, d, V, diff_l1, diff_jsd);
  return check_launch("backward_value");
}

int mfg_jsd(const float* p, const float* q, int64_t B, int d, double* out, mfg_stream_t stream) {
  REQUIRE(B >= 0 && d >= 1, "bad shape");
  if (B == 0) return MFG_OK;
  REQUIRE(p && q && out, "null pointer");
  hipLaunchKernelGGL(k_jsd, dim3(grid_for(B, WAVES, 8)), dim3(BLOCK), 0, S(stream), p, q, B, d, out);
  return check_launch("jsd");
}

int mfg_policy_logpdf(const float* pi, const float* P, int64_t N, int d, const double* thetas, int K, double shift,
                      double alpha_scale, double alpha_floor, double p_floor, double* out, mfg_stream_t stream) {
  const int64_t B = N;
  CHECK_BD();
  REQUIRE(pi && P && thetas && out && K >= 1, "null pointer / K < 1");
  hipLaunchKernelGGL(k_policy_logpdf, dim3(grid_for(N * K, WAVES, 8)), dim3(BLOCK), 0, S(stream), pi, P, N, d, thetas, K,
                     shift, alpha_scale, alpha_floor, p_floor, out);
  return check_launch("policy_logpdf");
}

}  // extern "C"
