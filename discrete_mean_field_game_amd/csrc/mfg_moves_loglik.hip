// The kernels of mfg_moves_loglik_pop and its entry points (mfg_moves_loglik.h, include/mfg_hip.h).
#include <math.h>

#include "mfg_moves_loglik.h"
#include "mfg_device.h"
#include "mfg_host.h"

namespace mfg {

// Stirling's correction of ln Gamma: ln Gamma(z) = (z - 1/2) ln z - z + ln(2 pi) / 2 + ml_stirling(z); z >= 16: the first
// omitted term is below 2e-16
__device__ __forceinline__ double ml_stirling(double z) {
  const double r = 1.0 / z, w = r * r;
  return r * (1.0 / 12.0 - w * (1.0 / 360.0 - w * (1.0 / 1260.0 - w * (1.0 / 1680.0 - w * (1.0 / 1188.0)))));
}

// the tail of digamma: psi(z) = ln z - 1 / (2 z) - ml_psi_tail(z); z >= 16 (the series of digamma_pos, one term shorter)
__device__ __forceinline__ double ml_psi_tail(double z) {
  const double r = 1.0 / z, w = r * r;
  return w * (1.0 / 12.0 - w * (1.0 / 120.0 - w * (1.0 / 252.0 - w * (1.0 / 240.0 - w * (1.0 / 132.0 - w * (691.0 / 32760.0))))));
}

// T(a, m) = sum_{t < m} ln(a + t) and D(a, m) = sum_{t < m} 1 / (a + t), m >= 0, without the difference of two ln Gamma or two
// digamma values.  The first s terms are the finite sums themselves, as q = prod (a + t) and q' = dq / da (all terms
// positive): T = ln q, D = q' / q; s = m for m <= 8, else the terms that bring a to 16.  The other m - s terms are the two
// ends' asymptotic series combined before anything is rounded, through L = log1p(m / a):
//   T = (a - 1/2) L + m (ln(a + m) - 1) + [stirling(a + m) - stirling(a)]
//   D = L + m / (2 a (a + m)) + [tail(a) - tail(a + m)]
// (the bracketed differences are of values below 1 / (12 a): their rounding does not show).  m = 0: q = 1, q' = 0, so T = D = 0
// exactly.  a = 0 with m > 0: T = ln 0 = -inf (D is the caller's to mark).
__device__ __forceinline__ void ml_td(double a, int64_t m, double& T, double& D) {
  int s = 0;
  if (m > 0) {
    if (m <= ML_SMALL_M && a < ML_PRODUCT_MAX) s = (int)m;
    else if (a < (double)ML_SERIES_MIN) s = ML_SERIES_MIN - (int)a < m ? ML_SERIES_MIN - (int)a : (int)m;
  }
  double q = 1.0, qp = 0.0;
  for (int t = 0; t < s; ++t) {
    const double xk = a + (double)t;
    qp = fma(qp, xk, q);
    q = q * xk;
  }
  T = log(q);
  D = qp / q;
  if (m > s) {
    const double b = a + (double)s, mm = (double)(m - s), z = b + mm;
    const double L = log1p(mm / b);
    T += (b - 0.5) * L + mm * (log(z) - 1.0) + (ml_stirling(z) - ml_stirling(b));
    D += L + mm / (2.0 * b * z) + (ml_psi_tail(b) - ml_psi_tail(z));
  }
}

__device__ __forceinline__ bool ml_finite(double x) { return fabs(x) <= 1.7976931348623157e308; }
__device__ __forceinline__ double ml_canon(double x) { return x != x ? (double)NAN : x; }

// a thread per row (s, n, h, i): coef = lgamma(n_i + 1) - sum_j lgamma(m_j + 1), j in column order; NaN for a row with a
// negative move or a non-finite state entry i of hour h
__global__ __launch_bounds__(ML_THREADS) void k_ml_rows(mfg_moves_loglik_t f, double* __restrict__ coef, int64_t rows) {
  const int64_t r = (int64_t)blockIdx.x * ML_THREADS + threadIdx.x;
  if (r >= rows) return;
  const int d = f.d, width = f.width, H = f.H;
  const int i = (int)(r % d);
  const int64_t t = r / d, per_set = (int64_t)f.N * (H - 1);
  const int64_t s = t / per_set, u = t - s * per_set, n = u / (H - 1), h = u - n * (H - 1);
  const int32_t* row = f.moves + s * f.moves_stride + ((u * width) + i) * (int64_t)width;
  const float st = f.state[s * f.state_stride + (n * H + h) * d + i];
  bool bad = !(fabsf(st) <= 3.4028234663852886e38f);
  int64_t tot = 0;
  double c = 0.0;
  for (int j = 0; j < d; ++j) {
    const int32_t m = row[j];
    bad = bad || m < 0;
    tot += m;
    if (m > 1) c -= lgamma((double)m + 1.0);
  }
  if (tot > 1) c += lgamma((double)tot + 1.0);
  coef[r] = bad ? (double)NAN : c;
}

// flag bits of a transition / a day (include/mfg_hip.h)
constexpr int ML_BAD_DATA = 1, ML_ZERO_ALPHA = 2, ML_BAD_POLICY = 4, ML_BAD_SET = 8;

// blockIdx.x: the transition u = n (H - 1) + h; blockIdx.y: the chunk of ML_WAVES * (64 / d) policies; a wavefront holds 64 / d
// policies, lane = slot * d + i (the lanes behind them idle).  The rows of a policy meet in LDS and are added by the lane of
// row 0 in the order i = 0 .. d - 1: the same additions wherever the policy sits.
__global__ __launch_bounds__(ML_THREADS) void k_ml_cells(mfg_moves_loglik_t f, const double* __restrict__ coef,
                                                         int32_t* __restrict__ flags) {
  __shared__ double rows[4][ML_THREADS];
  __shared__ int row_flag[ML_THREADS];
  const int d = f.d, width = f.width, H = f.H, K = f.policies;
  const int tid = threadIdx.x, lane = tid & 63, slots = 64 / d, slot = lane / d;
  const int i = lane - slot * d;
  const int k = (blockIdx.y * ML_WAVES + (tid >> 6)) * slots + slot;
  const int64_t u = blockIdx.x, trans = (int64_t)f.N * (H - 1);
  const int64_t n = u / (H - 1), h = u - n * (H - 1);
  const bool live = slot < slots && k < K;                 // (a lane behind the last policy computes nothing and writes nothing)
  double theta = 0.0, shift = 0.0, scale = 1.0;
  int64_t s = 0;
  int policy = 0;
  if (live) {
    theta = f.theta[k], shift = f.shift[k], scale = f.alpha_scale[k];
    s = f.set_index ? f.set_index[k] : 0;
    if (!(ml_finite(theta) && ml_finite(shift) && ml_finite(scale) && scale > 0.0)) policy |= ML_BAD_POLICY;
    if (s < 0 || s >= f.sets) policy |= ML_BAD_SET;
  }
  double ll = 0.0, g0 = 0.0, g1 = 0.0, g2 = 0.0;
  int flag = policy;
  if (live && policy == 0) {
    const float* pi = f.state + s * f.state_stride + (n * H + h) * d;
    const int32_t* row = f.moves + s * f.moves_stride + ((u * width) + i) * (int64_t)width;
    const double c = coef[(s * trans + u) * d + i];
    const double pii = (double)pi[i];
    double A = 0.0, sumT = 0.0, dth = 0.0, dsh = 0.0, dla = 0.0, Ath = 0.0, Ash = 0.0;
    int64_t tot = 0;
    bool zero = false;
    for (int j = 0; j < d; ++j) {
      const int64_t m = row[j];
      const double x = (double)pi[j] - pii - shift;
      double sp, sg;
      softplus_sigmoid(theta * x, sp, sg);
      const double a = scale * sp;
      const double ath = scale * sg * x, ash = -(scale * sg * theta);
      A += a, Ath += ath, Ash += ash;
      if (m > 0) {
        double T, D;
        ml_td(a, m, T, D);
        zero = zero || a == 0.0;
        tot += m;
        sumT += T;
        dth = fma(D, ath, dth), dsh = fma(D, ash, dsh), dla = fma(D, a, dla);
      }
    }
    if (c != c) {
      flag |= ML_BAD_DATA;
      ll = g0 = g1 = g2 = (double)NAN;
    } else if (zero) {
      flag |= ML_ZERO_ALPHA;
      ll = -(double)INFINITY;
      g0 = g1 = g2 = (double)NAN;
    } else if (tot > 0) {
      double T, D;
      ml_td(A, tot, T, D);
      ll = c + sumT - T;
      g0 = dth - D * Ath, g1 = dsh - D * Ash, g2 = dla - D * A;
    }
  }
  rows[0][tid] = ll, rows[1][tid] = g0, rows[2][tid] = g1, rows[3][tid] = g2;
  row_flag[tid] = flag;
  __syncthreads();
  if (live && i == 0) {
    for (int r = 1; r < d; ++r) {                          // (tid + r stays inside the policy's d lanes)
      ll = __dadd_rn(ll, rows[0][tid + r]);
      flag |= row_flag[tid + r];
      if (f.grad) g0 = __dadd_rn(g0, rows[1][tid + r]), g1 = __dadd_rn(g1, rows[2][tid + r]), g2 = __dadd_rn(g2, rows[3][tid + r]);
    }
    const int64_t o = (int64_t)k * trans + u;
    if (flag & (ML_BAD_POLICY | ML_BAD_SET | ML_BAD_DATA)) ll = g0 = g1 = g2 = (double)NAN;
    else if (flag & ML_ZERO_ALPHA) g0 = g1 = g2 = (double)NAN;       // (ll: -inf plus finite rows)
    f.ll[o] = ml_canon(ll);
    flags[o] = flag;
    if (f.grad) f.grad[3 * o] = ml_canon(g0), f.grad[3 * o + 1] = ml_canon(g1), f.grad[3 * o + 2] = ml_canon(g2);
  }
}

// a thread per (k, n): the transitions in the order h = 0 .. H - 2, each addition rounded on its own
__global__ __launch_bounds__(ML_THREADS) void k_ml_days(mfg_moves_loglik_t f, const int32_t* __restrict__ flags, int64_t days) {
  const int64_t r = (int64_t)blockIdx.x * ML_THREADS + threadIdx.x;
  if (r >= days) return;
  const int T = f.H - 1;
  double ll = 0.0, g0 = 0.0, g1 = 0.0, g2 = 0.0;
  int flag = 0;
  for (int h = 0; h < T; ++h) {
    const int64_t o = r * T + h;
    ll = __dadd_rn(ll, f.ll[o]);
    flag |= flags[o];
    if (f.grad) g0 = __dadd_rn(g0, f.grad[3 * o]), g1 = __dadd_rn(g1, f.grad[3 * o + 1]), g2 = __dadd_rn(g2, f.grad[3 * o + 2]);
  }
  f.ll_day[r] = ml_canon(ll);
  f.status[r] = flag;
  if (f.grad_day) f.grad_day[3 * r] = ml_canon(g0), f.grad_day[3 * r + 1] = ml_canon(g1), f.grad_day[3 * r + 2] = ml_canon(g2);
}

static void launch_moves_loglik(const mfg_moves_loglik_t& f, hipStream_t st) {
  const MlWs w = ml_layout(f.workspace, f.policies, f.sets, f.N, f.H, f.d);
  const int64_t trans = (int64_t)f.N * (f.H - 1), rows = (int64_t)f.sets * trans * f.d, days = (int64_t)f.policies * f.N;
  hipLaunchKernelGGL(k_ml_rows, dim3((unsigned)((rows + ML_THREADS - 1) / ML_THREADS)), dim3(ML_THREADS), 0, st, f, w.coef, rows);
  const int per_block = ML_WAVES * (64 / f.d);
  const dim3 grid((unsigned)trans, (unsigned)((f.policies + per_block - 1) / per_block));
  hipLaunchKernelGGL(k_ml_cells, grid, dim3(ML_THREADS), 0, st, f, w.coef, w.flags);
  hipLaunchKernelGGL(k_ml_days, dim3((unsigned)((days + ML_THREADS - 1) / ML_THREADS)), dim3(ML_THREADS), 0, st, f, w.flags, days);
}

}  // namespace mfg

using namespace mfg;

static bool ml_shape_ok(int policies, int sets, int N, int H, int d) {
  return policies >= 1 && policies <= MFG_POP_MAX_K && sets >= 1 && N >= 1 && H >= 2 && d >= 1 && d <= ML_MAX_D &&
         (int64_t)N * (H - 1) <= INT32_MAX && (int64_t)sets * N * (H - 1) * d <= ((int64_t)INT32_MAX - ML_THREADS) * ML_THREADS;
}

extern "C" size_t mfg_moves_loglik_workspace_bytes(int policies, int sets, int N, int H, int d) {
  if (!ml_shape_ok(policies, sets, N, H, d)) return 0;
  return ml_layout(nullptr, policies, sets, N, H, d).bytes;
}

extern "C" int mfg_moves_loglik_pop(const mfg_moves_loglik_t* loglik) {
  REQUIRE(loglik, "null descriptor");
  const mfg_moves_loglik_t& f = *loglik;
  REQUIRE(f.state && f.moves, "moves_loglik: null state or moves");
  REQUIRE(f.theta && f.shift && f.alpha_scale, "moves_loglik: null theta, shift or alpha_scale");
  REQUIRE(f.ll && f.ll_day && f.status, "moves_loglik: null ll, ll_day or status");
  REQUIRE((f.grad == nullptr) == (f.grad_day == nullptr), "moves_loglik: grad and grad_day are given together or not at all");
  REQUIRE(f.policies >= 1 && f.policies <= MFG_POP_MAX_K, "moves_loglik: policies outside [1, MFG_POP_MAX_K]");
  REQUIRE(f.N >= 1 && f.H >= 2, "moves_loglik: N < 1 or H < 2");
  REQUIRE(f.d >= 1 && f.d <= ML_MAX_D, "moves_loglik: d outside [1, 64]");
  REQUIRE(f.d <= f.width, "moves_loglik: d > width");
  REQUIRE(f.sets >= 1, "moves_loglik: sets < 1");
  REQUIRE((int64_t)f.N * (f.H - 1) <= INT32_MAX, "moves_loglik: N (H - 1) > 2^31 - 1");
  REQUIRE(ml_shape_ok(f.policies, f.sets, f.N, f.H, f.d), "moves_loglik: sets N (H - 1) d too large for one launch");
  if (f.sets > 1) {
    REQUIRE(f.state_stride >= (int64_t)f.N * f.H * f.d, "moves_loglik: state_stride below N H d");
    REQUIRE(f.moves_stride >= (int64_t)f.N * (f.H - 1) * f.width * f.width, "moves_loglik: moves_stride below N (H - 1) width^2");
  }
  REQUIRE(f.workspace && (reinterpret_cast<uintptr_t>(f.workspace) & 7) == 0, "moves_loglik: workspace null or not 8-byte aligned");
  const size_t need = mfg_moves_loglik_workspace_bytes(f.policies, f.sets, f.N, f.H, f.d);
  if (f.workspace_bytes < need)
    return fail(MFG_EWORKSPACE, "moves_loglik workspace: need %lld bytes, have %lld", (long long)need, (long long)f.workspace_bytes);
  launch_moves_loglik(f, S(f.stream));
  return check_launch("moves_loglik");
}
