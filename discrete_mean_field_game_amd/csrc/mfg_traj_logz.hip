// Importance log-weights of a trajectory store on the device (gfx950): ln z of the max-ent IRL loss as the reference wrote it,
//     z_j = [ 1/n_pol  sum_p q_p(tau_j) ]^-1,   q_p(tau) = Pr(s_1) prod_t q_{theta_p}(a_t; s_t)
// (reference ac_irl.py:292-321 calc_z's formula, :324-379 its TF graph; consumed by the weighted loss that ac_irl.py:404-406
// leaves commented out).  The reference multiplies 15 d Dirichlet densities in linear space over a hand-picked normaliser
// c = 2e11, which overflows; here everything stays in log space and in fp64:
//     log_z[k, row] = ln n_pol - logsumexp_p( sum_t ln q_{theta[k,p]}(a_t; s_t) - log_start ).
// ln q is the formula of k_policy_logpdf (mfg_launch_once.hip) with its alpha_floor / p_floor clamps and its device helpers.
//
// One launch, no host read: block (x = listed row, y = learner), one wavefront per policy (a loop when there are more
// policies than waves).  The per-policy sums of a round meet in LDS and one thread folds them into a running logsumexp in
// policy order -- a fixed association, so a learner's row has the same bits whatever K and the row list are.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <vector>

#include "../../include/mfg_hip.h"
#include "mfg_core.h"

namespace mfg {

struct TzArgs {
  const float *state, *action;  // [(K,) capacity, steps, d] / [(K,) capacity, steps, d, d]
  int64_t capacity;
  int64_t learner_rows;         // rows between two learners' stores (0: one store shared by all)
  const int32_t* rows;          // [n_rows] device
  int steps, d, n_pol;
  const double *thetas, *shift;  // [K, n_pol], [K]
  double alpha_scale, alpha_floor, p_floor, log_start;
  double* log_z;                // [K, capacity]
};

// sum_t ln q_theta(a_t; s_t) of one trajectory by one wavefront (every lane returns the total)
__device__ __forceinline__ double traj_logpdf_wave(const float* st, const float* ac, int steps, int d, double th, double shift,
                                                   double alpha_scale, double alpha_floor, double p_floor, int lane) {
  const int dd = d * d;
  double acc = 0.0;
  for (int t = 0; t < steps; ++t) {
    const float* pn = st + (int64_t)t * d;
    const float* Pn = ac + (int64_t)t * dd;
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
  }
  return wave_sum(acc);
}

__global__ __launch_bounds__(BLOCK) void k_traj_log_z_pop(TzArgs a) {
  __shared__ double s_lq[WAVES];
  const int lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x / WAVE;
  const int k = blockIdx.y;
  const int64_t row = a.rows[blockIdx.x];
  const int64_t srow = a.learner_rows * k + row;
  const float* st = a.state + srow * a.steps * a.d;
  const float* ac = a.action + srow * a.steps * a.d * a.d;
  const double shift = a.shift[k];
  const double* th = a.thetas + (int64_t)k * a.n_pol;
  // running logsumexp over the policies, in policy order (thread 0)
  double m = -INFINITY, s = 0.0;
  for (int p0 = 0; p0 < a.n_pol; p0 += WAVES) {
    const int p = p0 + wv;
    if (p < a.n_pol) {
      const double lq = traj_logpdf_wave(st, ac, a.steps, a.d, th[p], shift, a.alpha_scale, a.alpha_floor, a.p_floor, lane);
      if (lane == 0) s_lq[wv] = lq - a.log_start;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      const int np = a.n_pol - p0 < WAVES ? a.n_pol - p0 : WAVES;
      for (int u = 0; u < np; ++u) {
        const double x = s_lq[u];
        if (x != x) {          // (a NaN density stays visible)
          m = x;
          s = x;
        } else if (x > m) {    // (m = -inf: s = 0, nothing to rescale; x = +inf keeps m = +inf to the end)
          s = (m == -INFINITY ? 0.0 : s * exp(m - x)) + 1.0;
          m = x;
        } else if (x > -INFINITY && m < INFINITY) {
          s += exp(x - m);
        }
      }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    // every q_p = 0 (an exact zero in P with p_floor = 0): logsumexp = -inf and ln z = +inf, as Dirichlet.prob gives
    const double lse = (m == -INFINITY || m == INFINITY) ? m : m + log(s);
    a.log_z[(int64_t)k * a.capacity + row] = log((double)a.n_pol) - lse;
  }
}

}  // namespace mfg

using namespace mfg;

extern "C" int mfg_traj_log_z_pop(const float* state, const float* action, int64_t capacity, const int32_t* rows_host, int n_rows,
                                  int steps, int d, const double* thetas, int n_pol, const double* shift, int K,
                                  int per_learner_store, double alpha_scale, double alpha_floor, double p_floor, double log_start,
                                  double* log_z, void* scratch, size_t scratch_bytes, mfg_stream_t stream) {
  if (!state || !action || !rows_host || !thetas || !shift || !log_z || !scratch || capacity < 1 || n_rows < 0 ||
      n_rows > capacity || steps < 1 || d < 1 || d > MFG_MAX_D || n_pol < 1 || K < 1 || K > MFG_POP_MAX_K)
    return set_error(MFG_EINVAL, "traj_log_z_pop: null pointer / bad count");
  std::vector<char> seen((size_t)capacity, 0);
  for (int r = 0; r < n_rows; ++r) {
    if (rows_host[r] < 0 || rows_host[r] >= capacity) return set_error(MFG_EINVAL, "traj_log_z_pop: store row negative / beyond the store");
    if (seen[(size_t)rows_host[r]]) return set_error(MFG_EINVAL, "traj_log_z_pop: a store row twice in the list");
    seen[(size_t)rows_host[r]] = 1;
  }
  if (scratch_bytes < (size_t)n_rows * sizeof(int32_t))
    return set_error(MFG_EWORKSPACE, "traj_log_z_pop: scratch holds fewer than 4 n_rows bytes");
  if (n_rows == 0) return MFG_OK;
  // the row list is uploaded once; the caller may reuse rows_host on return, so the stream is drained before the launch
  hipStream_t st = (hipStream_t)stream;
  if (hipMemcpyAsync(scratch, rows_host, (size_t)n_rows * sizeof(int32_t), hipMemcpyHostToDevice, st) != hipSuccess ||
      hipStreamSynchronize(st) != hipSuccess)
    return set_error(MFG_ELAUNCH, "traj_log_z_pop: row upload failed");
  TzArgs a{};
  a.state = state; a.action = action;
  a.capacity = capacity;
  a.learner_rows = per_learner_store ? capacity : 0;
  a.rows = (const int32_t*)scratch;
  a.steps = steps; a.d = d; a.n_pol = n_pol;
  a.thetas = thetas; a.shift = shift;
  a.alpha_scale = alpha_scale; a.alpha_floor = alpha_floor; a.p_floor = p_floor; a.log_start = log_start;
  a.log_z = log_z;
  hipLaunchKernelGGL(k_traj_log_z_pop, dim3((unsigned)n_rows, (unsigned)K), dim3(BLOCK), 0, st, a);
  return hipGetLastError() == hipSuccess ? MFG_OK : set_error(MFG_ELAUNCH, "traj_log_z_pop: launch failed");
}
