// The three kernels of mfg_var_fit_pop and its entry points (mfg_var_pop.h, include/mfg_hip.h).
#include <math.h>

#include "mfg_host.h"
#include "mfg_var_pop.h"

namespace mfg {

constexpr int VAR_THREADS = 1024;
constexpr int VAR_PARTS = VAR_THREADS / 64;   // strided partial sums of one dot product
constexpr int VAR_SOLVE_THREADS = 1024;

struct VarModel {
  int p, m, T, n, R, S;
  const int32_t *tr, *te;
  char* slice;
  double* W;
};

__device__ __forceinline__ VarModel var_model(const mfg_var_fit_t& f, const mfg_var_model_t& mo, int k) {
  VarModel v;
  v.p = mo.lag;
  v.m = 1 + mo.lag * f.d;
  v.T = mo.n_train * f.Hd;
  v.n = v.T - v.p;
  v.R = v.m + f.d;
  v.S = mo.n_test * f.Hd;
  v.tr = f.train_idx + (int64_t)k * f.train_stride;
  v.te = f.test_idx + (int64_t)k * f.test_stride;
  v.slice = reinterpret_cast<char*>(f.workspace) + mo.ws_offset;
  v.W = reinterpret_cast<double*>(v.slice + VAR_HEAD_BYTES);
  return v;
}

// row r of the model's extended series: the training days in list order, then the test days
__device__ __forceinline__ const double* var_row(const mfg_var_fit_t& f, const VarModel& v, int r) {
  const int32_t* list = r < v.T ? v.tr : v.te;
  const int rr = r < v.T ? r : r - v.T;
  const int day = rr / f.Hd, hour = rr - day * f.Hd;
  return f.days + ((int64_t)var_day(list[day], f.D) * f.Hd + hour) * f.d;
}

// One operand of a Gram element along t: column j of the training row t - l, or the constant.
struct VarWalk {
  const double* days;
  const int32_t* list;
  const double* base;
  int Hd, d, D, j, n_days, day, hour;
  bool one;
  __device__ __forceinline__ void load() { base = days + (int64_t)var_day(list[day], D) * Hd * d + j; }
  __device__ __forceinline__ void init(const mfg_var_fit_t& f, const int32_t* tr, int n_train, int row0, int col, bool constant) {
    days = f.days, list = tr, Hd = f.Hd, d = f.d, D = f.D, j = col, n_days = n_train, one = constant;
    day = row0 / Hd, hour = row0 - day * Hd;
    load();
  }
  __device__ __forceinline__ double get() const { return one ? 1.0 : base[hour * d]; }
  __device__ __forceinline__ void next() {
    if (++hour == Hd) {
      hour = 0;
      if (++day < n_days) load();
    }
  }
};

// ---- grid (tiles, K), 16 x 16 threads: element (r, c) of W, r < m: G[r][c] for c <= r; r >= m: (Z'Y)[c][r - m]
__global__ __launch_bounds__(256) void k_var_gram(mfg_var_fit_t f, int tiles_c) {
  const int k = blockIdx.y;
  const mfg_var_model_t mo = f.models[k];
  const VarModel v = var_model(f, mo, k);
  const int d = f.d;
  const int r = (int)(blockIdx.x / tiles_c) * 16 + (int)(threadIdx.x >> 4);
  const int c = (int)(blockIdx.x % tiles_c) * 16 + (int)(threadIdx.x & 15);
  if (r >= v.R || c >= v.m || (r < v.m && c > r)) return;
  // operand a: regressor r (lag la >= 1 or the constant), or topic r - m of the row itself (lag 0); operand b: regressor c
  const int ra = r < v.m ? r : 0;
  const int la = r < v.m ? (r == 0 ? 0 : (ra - 1) / d + 1) : 0;
  const int ja = r < v.m ? (r == 0 ? 0 : (ra - 1) % d) : r - v.m;
  const int lb = c == 0 ? 0 : (c - 1) / d + 1, jb = c == 0 ? 0 : (c - 1) % d;
  VarWalk a, b;
  a.init(f, v.tr, mo.n_train, v.p - la, ja, r == 0);
  b.init(f, v.tr, mo.n_train, v.p - lb, jb, c == 0);
  double s = 0.0;
  for (int t = v.p; t < v.T; ++t) {
    s = fma(a.get(), b.get(), s);
    a.next();
    b.next();
  }
  if (r == c) s += mo.ridge;
  v.W[(int64_t)r * v.m + c] = s;
}

// ---- one workgroup, model blockIdx.x
__global__ __launch_bounds__(VAR_SOLVE_THREADS) void k_var_solve(mfg_var_fit_t f) {
  const int k = blockIdx.x, tid = threadIdx.x;
  const mfg_var_model_t mo = f.models[k];
  const VarModel v = var_model(f, mo, k);
  const int d = f.d, m = v.m, R = v.R;
  double* W = v.W;
  double* coef = f.coef + (int64_t)k * f.M * d;
  __shared__ double Ld[VAR_PANEL][VAR_PANEL + 1];
  __shared__ int fail;
  if (tid == 0) fail = 0;
  const int lr = tid >> 4, lc = tid & 15;   // (of the first 256 threads)

  for (int j0 = 0; j0 < m; j0 += VAR_PANEL) {
    const int nb = min(VAR_PANEL, m - j0), j1 = j0 + nb;
    // the diagonal block (a short last block is padded with the identity)
    if (tid < 256) Ld[lr][lc] = (lr < nb && lc <= lr) ? W[(j0 + lr) * m + j0 + lc] : (lr == lc ? 1.0 : 0.0);
    __syncthreads();
    for (int c = 0; c < nb; ++c) {
      if (tid == 0) {
        const double piv = Ld[c][c];
        if (!(piv > 0.0) || !isfinite(piv)) fail = 1;
        Ld[c][c] = sqrt(piv);
      }
      __syncthreads();
      if (tid > c && tid < nb) Ld[tid][c] = Ld[tid][c] / Ld[c][c];
      __syncthreads();
      if (tid < 256 && lr < nb && lc > c && lc <= lr) Ld[lr][lc] = fma(-Ld[lr][c], Ld[lc][c], Ld[lr][lc]);
      __syncthreads();
    }
    if (tid < 256 && lr < nb && lc <= lr) W[(j0 + lr) * m + j0 + lc] = Ld[lr][lc];
    // the panel, a row per thread: x L' = a, columns in order (rows >= m are the right-hand sides: their forward substitution).
    // The row stays in the workspace and is read back through the cache: held in 16 registers under unrolled loops the kernel
    // spilled (780 bytes of scratch per lane at the 128 VGPRs of a 1 024-thread workgroup, 272 at 512 threads).
    for (int i = j1 + tid; i < R; i += VAR_SOLVE_THREADS) {
      double* x = W + i * m + j0;
      for (int c = 0; c < nb; ++c) {
        double s = x[c];
        for (int e = 0; e < c; ++e) s = fma(-x[e], Ld[c][e], s);
        x[c] = s / Ld[c][c];
      }
    }
    __syncthreads();
    // the trailing update, an element per thread (there is one only behind a full panel): the 16 products in column order
    const int nc = m - j1, nr = R - j1;
    for (int e = tid; e < nr * nc; e += VAR_SOLVE_THREADS) {
      const int i = j1 + e / nc, kk = j1 + e % nc;
      if (kk > i) continue;
      const double* li = W + i * m + j0;
      const double* lk = W + kk * m + j0;
      double s = W[i * m + kk];
#pragma unroll
      for (int c = 0; c < VAR_PANEL; ++c) s = fma(-li[c], lk[c], s);
      W[i * m + kk] = s;
    }
    __syncthreads();
  }

  // L' B = Y from the last panel up; Y' sits in the rows m + c of W
  for (int j0 = (m - 1) / VAR_PANEL * VAR_PANEL; j0 >= 0; j0 -= VAR_PANEL) {
    const int nb = min(VAR_PANEL, m - j0);
    if (tid < 256) Ld[lr][lc] = (lr < nb && lc <= lr) ? W[(j0 + lr) * m + j0 + lc] : (lr == lc ? 1.0 : 0.0);
    __syncthreads();
    if (tid < d) {
      for (int r = nb - 1; r >= 0; --r) {
        double s = W[(m + tid) * m + j0 + r];
        for (int e = nb - 1; e > r; --e) s = fma(-Ld[e][r], coef[(j0 + e) * d + tid], s);
        coef[(j0 + r) * d + tid] = s / Ld[r][r];
      }
    }
    __syncthreads();
    for (int e = tid; e < j0 * d; e += VAR_SOLVE_THREADS) {
      const int c = e / j0, i = e % j0;
      double s = W[(m + c) * m + i];
      for (int r = 0; r < nb; ++r) s = fma(-W[(j0 + r) * m + i], coef[(j0 + r) * d + c], s);
      W[(m + c) * m + i] = s;
    }
    __syncthreads();
  }
  for (int e = m * d + tid; e < f.M * d; e += VAR_SOLVE_THREADS) coef[e] = 0.0;
  if (tid == 0) *reinterpret_cast<int32_t*>(v.slice) = fail;
}

// yh[j] = sum_i coef[i][j] z[i] for j < d: thread (q, j) adds the terms i = q, q + 16, ... in ascending order, thread (0, j) the 16
// partial sums in order.  Ends behind a barrier.
__device__ __forceinline__ void var_dot(const double* __restrict__ coef, const double* z, int m, int d,
                                        double (*part)[64], double* yh) {
  const int q = threadIdx.x >> 6, j = threadIdx.x & 63;
  double acc = 0.0;
  if (j < d)
    for (int i = q; i < m; i += VAR_PARTS) acc = fma(coef[i * d + j], z[i], acc);
  part[q][j] = acc;
  __syncthreads();
  if (q == 0 && j < d) {
    double s = part[0][j];
#pragma unroll
    for (int w = 1; w < VAR_PARTS; ++w) s += part[w][j];
    yh[j] = s;
  }
  __syncthreads();
}

// ---- one workgroup, model blockIdx.x
__global__ __launch_bounds__(VAR_THREADS) void k_var_forecast(mfg_var_fit_t f) {
  const int k = blockIdx.x, tid = threadIdx.x;
  const mfg_var_model_t mo = f.models[k];
  const VarModel v = var_model(f, mo, k);
  const int d = f.d, Hd = f.Hd, m = v.m, T = v.T, S = v.S, Nt = mo.n_test;
  double* __restrict__ coef = f.coef + (int64_t)k * f.M * d;
  double* __restrict__ future = f.future ? f.future + (int64_t)k * f.S_max * d : nullptr;
  double* __restrict__ per_day = f.per_day ? f.per_day + (int64_t)k * f.test_stride * 4 : nullptr;
  __shared__ double z[2][VAR_MAX_M];
  __shared__ double part[VAR_PARTS][64];
  __shared__ double yh[64], yo[64];
  __shared__ double pd[VAR_MAX_DAYS][4];
  __shared__ int bad;
  if (tid == 0) bad = 0;
  __syncthreads();

  // the rows the model reads: its day indices and every value of its training and test days
  int mine = 0;
  for (int i = tid; i < mo.n_train; i += VAR_THREADS) mine |= v.tr[i] < 0 || v.tr[i] >= f.D;
  for (int i = tid; i < Nt; i += VAR_THREADS) mine |= v.te[i] < 0 || v.te[i] >= f.D;
  for (int e = tid; e < (T + S) * d; e += VAR_THREADS) {
    const int r = e / d;
    mine |= !isfinite(var_row(f, v, r)[e - r * d]);
  }
  if (mine) atomicOr(&bad, 1);
  __syncthreads();
  const int status = bad ? MFG_VAR_NONFINITE : (*reinterpret_cast<const int32_t*>(v.slice) ? MFG_VAR_PIVOT : 0);
  if (status) {
    for (int e = tid; e < f.M * d; e += VAR_THREADS) coef[e] = NAN;
    if (future)
      for (int e = tid; e < f.S_max * d; e += VAR_THREADS) future[e] = NAN;
    if (per_day)
      for (int e = tid; e < f.test_stride * 4; e += VAR_THREADS) per_day[e] = NAN;
    if (tid < d) f.sse[(int64_t)k * d + tid] = NAN;
    if (tid < 2) f.insample[(int64_t)k * 2 + tid] = NAN;
    if (tid < 8) f.metrics[(int64_t)k * 8 + tid] = NAN;
    if (tid == 0) f.status[k] = status;
    return;
  }

  // the fitted rows: evaluate_train part 2 and the residual sums of squares, t ascending
  double sse = 0.0, l1_sum = 0.0, jsd_sum = 0.0;
  for (int t = v.p; t < T; ++t) {
    for (int i = tid; i < m; i += VAR_THREADS) {
      const int l = i == 0 ? 0 : (i - 1) / d + 1;
      z[0][i] = i == 0 ? 1.0 : var_row(f, v, t - l)[i - 1 - (l - 1) * d];
    }
    if (tid < d) yo[tid] = var_row(f, v, t)[tid];
    __syncthreads();
    var_dot(coef, z[0], m, d, part, yh);
    if (tid < 64) {
      double l1, jsd;
      var_row_metrics(yo, yh, d, l1, jsd);
      l1_sum += l1;
      jsd_sum += jsd;
      if (tid < d) {
        const double e = yo[tid] - yh[tid];
        sse = fma(e, e, sse);
      }
    }
    __syncthreads();
  }
  if (tid < d) f.sse[(int64_t)k * d + tid] = sse;
  if (tid == 0) {
    f.insample[(int64_t)k * 2] = l1_sum / (double)v.n;
    f.insample[(int64_t)k * 2 + 1] = jsd_sum / (double)v.n;
  }

  // the forecast: S rows, sequential
  int cur = 0, hour = 0, day = 0;
  double day_l1 = 0.0, day_jsd = 0.0;
  if (S > 0 && mo.origin == 0) {
    for (int i = tid; i < m; i += VAR_THREADS) {
      const int l = i == 0 ? 0 : (i - 1) / d + 1;
      z[0][i] = i == 0 ? 1.0 : var_row(f, v, T - l)[i - 1 - (l - 1) * d];
    }
  }
  __syncthreads();
  for (int s = 0; s < S; ++s) {
    const bool observed = mo.origin == 1 && hour == 0;   // the rolling origin: hour 0 of a test day is given
    if (tid < d) {
      const double y = var_row(f, v, T + s)[tid];
      yo[tid] = y;
      if (observed) yh[tid] = y;
    }
    __syncthreads();
    if (!observed) var_dot(coef, z[cur], m, d, part, yh);
    if (future && tid < d) future[s * d + tid] = yh[tid];
    if (tid < 64) {
      double l1, jsd;
      var_row_metrics(yo, yh, d, l1, jsd);
      day_l1 += l1;
      day_jsd += jsd;
      if (hour == Hd - 1) {
        if (tid == 0) {
          pd[day][0] = l1;
          pd[day][1] = day_l1 / (double)Hd;
          pd[day][2] = jsd;
          pd[day][3] = day_jsd / (double)Hd;
        }
        day_l1 = day_jsd = 0.0;
      }
    }
    if (observed) {
      // the history of the day: the last p rows of [training series | test days before | this row], all observed
      for (int i = tid; i < m; i += VAR_THREADS) {
        const int l = i == 0 ? 0 : (i - 1) / d + 1;
        z[cur][i] = i == 0 ? 1.0 : var_row(f, v, T + s + 1 - l)[i - 1 - (l - 1) * d];
      }
    } else {
      for (int i = tid; i < m; i += VAR_THREADS) z[cur ^ 1][i] = i == 0 ? 1.0 : (i <= d ? yh[i - 1] : z[cur][i - d]);
      cur ^= 1;
    }
    if (++hour == Hd) hour = 0, ++day;
    __syncthreads();
  }

  if (tid < Nt * 4 && per_day) per_day[tid] = pd[tid >> 2][tid & 3];
  if (per_day)
    for (int e = Nt * 4 + tid; e < f.test_stride * 4; e += VAR_THREADS) per_day[e] = 0.0;
  if (future)
    for (int e = S * d + tid; e < f.S_max * d; e += VAR_THREADS) future[e] = 0.0;
  if (tid < 4) {
    // mean and np.std (ddof 0) over the test days, in day order
    double mean = NAN, sd = NAN;
    if (Nt > 0) {
      double a = 0.0;
      for (int j = 0; j < Nt; ++j) a += pd[j][tid];
      mean = a / (double)Nt;
      double q = 0.0;
      for (int j = 0; j < Nt; ++j) q = fma(pd[j][tid] - mean, pd[j][tid] - mean, q);
      sd = sqrt(q / (double)Nt);
    }
    f.metrics[(int64_t)k * 8 + 2 * tid] = mean;
    f.metrics[(int64_t)k * 8 + 2 * tid + 1] = sd;
  }
  if (tid == 0) f.status[k] = 0;
}

void launch_var_fit(const mfg_var_fit_t& f, int m_max, hipStream_t st) {
  const int tiles_c = (m_max + 15) / 16, tiles_r = (m_max + f.d + 15) / 16;
  hipLaunchKernelGGL(k_var_gram, dim3((unsigned)(tiles_r * tiles_c), (unsigned)f.K), dim3(256), 0, st, f, tiles_c);
  hipLaunchKernelGGL(k_var_solve, dim3((unsigned)f.K), dim3(VAR_SOLVE_THREADS), 0, st, f);
  hipLaunchKernelGGL(k_var_forecast, dim3((unsigned)f.K), dim3(VAR_THREADS), 0, st, f);
}

// NULL when the record is inside the limits of include/mfg_hip.h, else what is wrong with it
static const char* var_model_error(const mfg_var_model_t& mo, int Hd, int d) {
  if (mo.lag < 1) return "lag < 1";
  if (mo.n_train < 1 || mo.n_train > VAR_MAX_DAYS) return "training days outside [1, 64]";
  if (mo.n_test < 0 || mo.n_test > VAR_MAX_DAYS) return "test days outside [0, 64]";
  if (mo.origin != 0 && mo.origin != 1) return "origin not 0 or 1";
  if ((int64_t)mo.lag * d + 1 > VAR_MAX_M) return "1 + lag d > MFG_VAR_MAX_REGRESSORS";
  const int T = mo.n_train * Hd;
  if (T - mo.lag < 1) return "no row to fit: lag >= training rows";
  if (mo.origin == 1 && mo.lag > T + 1) return "rolling origin: lag > training rows + 1";
  if (!(mo.ridge > 0.0) || !std::isfinite(mo.ridge)) return "ridge not finite and > 0";
  return nullptr;
}

}  // namespace mfg

using namespace mfg;

extern "C" size_t mfg_var_fit_workspace_bytes(int K, mfg_var_model_t* models_host, int d) {
  if (K < 1 || !models_host || d < 1 || d > VAR_MAX_D) return 0;
  size_t at = 0;
  for (int k = 0; k < K; ++k) {
    mfg_var_model_t& mo = models_host[k];
    if (mo.lag < 1 || (int64_t)mo.lag * d + 1 > VAR_MAX_M) return 0;
    mo.ws_offset = (int64_t)at;
    at += var_model_bytes(1 + mo.lag * d, d);
  }
  return at;
}

extern "C" int mfg_var_fit_pop(const mfg_var_fit_t* fit) {
  REQUIRE(fit, "null descriptor");
  const mfg_var_fit_t& f = *fit;
  REQUIRE(f.K >= 1 && f.K <= MFG_POP_MAX_K, "population size K outside [1, MFG_POP_MAX_K]");
  REQUIRE(f.D >= 1, "D < 1");
  REQUIRE(f.Hd >= 1 && f.Hd <= VAR_MAX_H, "Hd outside [1, 64]");
  REQUIRE(f.d >= 1 && f.d <= VAR_MAX_D, "d outside [1, 64]");
  REQUIRE(f.train_stride >= 1 && f.test_stride >= 0, "index table strides");
  REQUIRE(f.M >= 1 && f.M <= VAR_MAX_M && f.S_max >= 0, "M outside [1, MFG_VAR_MAX_REGRESSORS] or S_max < 0");
  REQUIRE(f.days && f.models_host && f.models && f.train_idx && f.coef && f.sse && f.insample && f.metrics && f.status &&
              f.workspace && (f.test_idx || f.test_stride == 0),
          "null pointer");
  REQUIRE((reinterpret_cast<uintptr_t>(f.workspace) & 7) == 0, "workspace not 8-byte aligned");
  size_t at = 0;
  int m_max = 0;
  for (int k = 0; k < f.K; ++k) {
    const mfg_var_model_t& mo = f.models_host[k];
    if (const char* what = var_model_error(mo, f.Hd, f.d)) return fail(MFG_EINVAL, "var fit: model %d: %s", k, what);
    const int m = 1 + mo.lag * f.d;
    if (m > f.M) return fail(MFG_EINVAL, "var fit: model %d: %d regressors, coef has M = %d rows", k, m, f.M);
    if (mo.n_train > f.train_stride || mo.n_test > f.test_stride)
      return fail(MFG_EINVAL, "var fit: model %d: more days than the index tables' strides", k);
    if (f.future && mo.n_test * f.Hd > f.S_max) return fail(MFG_EINVAL, "var fit: model %d: %d forecast rows > S_max = %d", k, mo.n_test * f.Hd, f.S_max);
    if (mo.ws_offset != (int64_t)at)
      return fail(MFG_EINVAL, "var fit: model %d: ws_offset is not the layout of mfg_var_fit_workspace_bytes", k);
    at += var_model_bytes(m, f.d);
    m_max = m > m_max ? m : m_max;
  }
  if (f.workspace_bytes < at)
    return fail(MFG_EWORKSPACE, "var fit workspace: need %lld bytes, have %lld", (long long)at, (long long)f.workspace_bytes);
  launch_var_fit(f, m_max, S(f.stream));
  return check_launch("var_fit_pop");
}
