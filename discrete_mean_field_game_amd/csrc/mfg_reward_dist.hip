// Reward distributions and mean actions: kernels, launch rules and entry points (mfg_reward_dist.h, include/mfg_hip.h).
#include "mfg_reward_dist.h"

#include <math.h>

#include "mfg_host.h"

namespace mfg {

// Total of the RD_BLOCK thread values, returned to every thread: a binary tree in LDS, the same order for every call.
__device__ __forceinline__ double block_sum(double v, double* red) {
  const int t = threadIdx.x;
  __syncthreads();  // (the previous total may still be being read)
  red[t] = v;
  __syncthreads();
  for (int s = RD_BLOCK / 2; s > 0; s >>= 1) {
    if (t < s) red[t] += red[t + s];
    __syncthreads();
  }
  return red[0];
}

// np.linspace(start, stop, last + 1)[i]: fl(fl(i step) + start), two roundings (no FMA), and stop itself at the end
__device__ __forceinline__ double lin_point(int i, int last, double start, double stop, double step) {
#pragma clang fp contract(off)
  if (i >= last && last > 0) return stop;
  const double m = (double)i * step;
  return m + start;
}

__global__ __launch_bounds__(RD_BLOCK) void k_row_distribution(RowDistArgs a) {
  __shared__ double red[RD_BLOCK];
  __shared__ float redf[2][RD_BLOCK];
  __shared__ unsigned cnt[MFG_DIST_MAX_BINS];
  __shared__ double tile[RD_TILE];
  const int t = threadIdx.x;
  const int64_t r = blockIdx.x, N = a.N;
  const int bins = a.bins, G = a.G;
  const float* __restrict__ x = a.values + r * a.stride;
  double* mom = a.moments + r * 6;
  int64_t* counts = a.counts + r * bins;
  double* edges = a.edges + r * (bins + 1);
  double* dens = G > 0 ? a.density + r * G : nullptr;
  const double nan = __longlong_as_double(0x7FF8000000000000ll);

  // ---- pass 1: a non-finite value; min and max (fp32: exact)
  float mn = INFINITY, mx = -INFINITY;
  int bad = 0;
  for (int64_t n = t; n < N; n += RD_BLOCK) {
    const float v = x[n];
    bad |= !isfinite(v);
    mn = fminf(mn, v);
    mx = fmaxf(mx, v);
  }
  if (__syncthreads_or(bad)) {
    for (int i = t; i < bins; i += RD_BLOCK) {
      counts[i] = 0;
      edges[i] = nan;
    }
    for (int g = t; g < G; g += RD_BLOCK) dens[g] = nan;
    if (t == 0) {
      edges[bins] = nan;
      for (int q = 0; q < 6; ++q) mom[q] = nan;
      a.status[r] = MFG_DIST_NONFINITE;
    }
    return;
  }
  redf[0][t] = mn;
  redf[1][t] = mx;
  __syncthreads();
  for (int s = RD_BLOCK / 2; s > 0; s >>= 1) {
    if (t < s) {
      redf[0][t] = fminf(redf[0][t], redf[0][t + s]);
      redf[1][t] = fmaxf(redf[1][t], redf[1][t + s]);
    }
    __syncthreads();
  }
  const double xmin = (double)redf[0][0], xmax = (double)redf[1][0];

  // ---- pass 2: the mean
  double s1 = 0.0;
  for (int64_t n = t; n < N; n += RD_BLOCK) s1 += (double)x[n];
  const double mean = block_sum(s1, red) / (double)N;

  // ---- pass 3: the variance and the histogram
  double first = a.use_range ? a.lo : xmin, last = a.use_range ? a.hi : xmax;
  if (first == last) {
    first -= 0.5;
    last += 0.5;
  }
  const double width = last - first, step = width / (double)bins;
  for (int i = t; i < bins; i += RD_BLOCK) cnt[i] = 0u;
  __syncthreads();
  double s2 = 0.0;
  for (int64_t n = t; n < N; n += RD_BLOCK) {
    const double v = (double)x[n];
    const double dv = v - mean;
    s2 += dv * dv;
    if (v >= first && v <= last) {
      // NumPy's guess, then its two corrections against the exact edges
      int i = (int)(((v - first) / width) * (double)bins);
      if (i >= bins) i = bins - 1;
      if (v < lin_point(i, bins, first, last, step)) --i;
      if (i != bins - 1 && v >= lin_point(i + 1, bins, first, last, step)) ++i;
      atomicAdd(&cnt[i], 1u);
    }
  }
  const double var = block_sum(s2, red) / (double)(N - 1);  // (N = 1: 0 / 0, NaN as np.var(ddof=1))
  double kept = 0.0;
  for (int i = t; i < bins; i += RD_BLOCK) {
    const unsigned c = cnt[i];
    kept += (double)c;
    counts[i] = (int64_t)c;
    edges[i] = lin_point(i, bins, first, last, step);
  }
  kept = block_sum(kept, red);  // (integers below 2^31: exact in any order)
  const double c = var * a.bw_factor;
  const bool no_kde = !(N >= 2 && var > 0.0);
  if (t == 0) {
    edges[bins] = last;
    mom[0] = kept;
    mom[1] = xmin;
    mom[2] = xmax;
    mom[3] = mean;
    mom[4] = var;
    mom[5] = c;
    a.status[r] = no_kde ? MFG_DIST_NO_KDE : 0;
  }
  if (G == 0) return;
  if (no_kde) {
    for (int g = t; g < G; g += RD_BLOCK) dens[g] = nan;
    return;
  }

  // ---- the KDE: thread t owns grid points t, t + RD_BLOCK, ...; the values pass through LDS as fp64, tile by tile
  const double two_c = 2.0 * c, denom = (double)N * sqrt(2.0 * M_PI * c);
  const double gstep = G > 1 ? (a.x_hi - a.x_lo) / (double)(G - 1) : 0.0;
  for (int g0 = 0; g0 < G; g0 += RD_BLOCK) {
    const int g = g0 + t;
    const double gx = lin_point(g < G ? g : 0, G - 1, a.x_lo, a.x_hi, gstep);
    double acc = 0.0;
    for (int64_t n0 = 0; n0 < N; n0 += RD_TILE) {
      const int m = (int)(N - n0 < RD_TILE ? N - n0 : RD_TILE);
      __syncthreads();  // (the previous tile is still being read)
      for (int i = t; i < m; i += RD_BLOCK) tile[i] = (double)x[n0 + i];
      __syncthreads();
      for (int i = 0; i < m; ++i) {
        const double dx = gx - tile[i];
        acc += exp(-(dx * dx) / two_c);
      }
    }
    if (g < G) dens[g] = acc / denom;
  }
}

void launch_row_distribution(const RowDistArgs& a, int R, hipStream_t st) {
  hipLaunchKernelGGL(k_row_distribution, dim3((unsigned)R), dim3(RD_BLOCK), 0, st, a);
}

// ---- mean action matrices: block (c, k) adds chunk c of learner k's matrices, element by element ----
__global__ __launch_bounds__(RD_BLOCK) void k_action_mean_partial(const float* __restrict__ action, int64_t s_action, int64_t N,
                                                                  int E, int64_t rows, double* __restrict__ partials) {
  const int c = blockIdx.x, k = blockIdx.y, chunks = gridDim.x;
  const int64_t n0 = (int64_t)c * rows;
  const int64_t n1 = n0 + rows < N ? n0 + rows : N;  // (n0 >= N in the last chunks of a capped grid: an empty sum)
  const float* base = action + (int64_t)k * s_action;
  double* out = partials + ((int64_t)k * chunks + c) * E;
  for (int e = threadIdx.x; e < E; e += RD_BLOCK) {
    const float* p = base + (n0 < n1 ? n0 * E : 0) + e;
    double s = 0.0;
    int64_t n = n0;
    for (; n + AM_FLIGHT <= n1; n += AM_FLIGHT, p += (int64_t)AM_FLIGHT * E) {  // AM_FLIGHT loads in flight, added in row order
      float v[AM_FLIGHT];
#pragma unroll
      for (int j = 0; j < AM_FLIGHT; ++j) v[j] = p[(int64_t)j * E];
#pragma unroll
      for (int j = 0; j < AM_FLIGHT; ++j) s += (double)v[j];
    }
    for (; n < n1; ++n, p += E) s += (double)*p;
    out[e] = s;
  }
}

// block (x, k): elements AM_FOLD_E x .. of learner k.  Thread (s, el) = (t / AM_FOLD_E, t mod AM_FOLD_E) adds the partials of the
// s-th of AM_FOLD_S equal runs of chunks in chunk order, AM_FLIGHT loads in flight; the run totals are added in run order.
__global__ __launch_bounds__(RD_BLOCK) void k_action_mean_fold(const double* __restrict__ partials, int chunks, int E, int64_t N,
                                                               double* __restrict__ mean) {
  __shared__ double part[AM_FOLD_S][AM_FOLD_E];
  const int el = threadIdx.x % AM_FOLD_E, sl = threadIdx.x / AM_FOLD_E, k = blockIdx.y;
  const int e = blockIdx.x * AM_FOLD_E + el;
  const int per = (chunks + AM_FOLD_S - 1) / AM_FOLD_S;
  const int c0 = sl * per, c1 = c0 + per < chunks ? c0 + per : chunks;
  double s = 0.0;
  if (e < E && c0 < c1) {
    const double* p = partials + ((int64_t)k * chunks + c0) * E + e;
    int c = c0;
    for (; c + AM_FLIGHT <= c1; c += AM_FLIGHT, p += (int64_t)AM_FLIGHT * E) {
      double v[AM_FLIGHT];
#pragma unroll
      for (int j = 0; j < AM_FLIGHT; ++j) v[j] = p[(int64_t)j * E];
#pragma unroll
      for (int j = 0; j < AM_FLIGHT; ++j) s += v[j];
    }
    for (; c < c1; ++c, p += E) s += *p;
  }
  part[sl][el] = s;
  __syncthreads();
  if (sl == 0 && e < E) {
    double tot = 0.0;
    for (int q = 0; q < AM_FOLD_S; ++q) tot += part[q][el];
    mean[(int64_t)k * E + e] = tot / (double)N;
  }
}

void launch_action_mean(const float* action, int64_t s_action, int K, int64_t N, int d, double* mean, double* partials,
                        hipStream_t st) {
  const int E = d * d, chunks = action_mean_chunks(N);
  hipLaunchKernelGGL(k_action_mean_partial, dim3((unsigned)chunks, (unsigned)K), dim3(RD_BLOCK), 0, st, action, s_action, N, E,
                     action_mean_rows(N), partials);
  hipLaunchKernelGGL(k_action_mean_fold, dim3((unsigned)((E + AM_FOLD_E - 1) / AM_FOLD_E), (unsigned)K), dim3(RD_BLOCK), 0, st,
                     partials, chunks, E, N, mean);
}

}  // namespace mfg

using namespace mfg;

extern "C" size_t mfg_row_distribution_workspace_bytes(int R, int64_t N, int bins, int G) {
  (void)R, (void)N, (void)bins, (void)G;
  return 0;  // counts, tiles and partial sums live in LDS
}

extern "C" int mfg_row_distribution(const float* values, int R, int64_t N, int64_t stride, int bins, int use_range, double lo,
                                    double hi, int G, double x_lo, double x_hi, double* moments, int64_t* counts, double* edges,
                                    double* density, int32_t* status, void* workspace, size_t workspace_bytes,
                                    mfg_stream_t stream) {
  REQUIRE(R >= 1, "no rows (R < 1)");
  REQUIRE(N >= 1 && N <= 0x7FFFFFFF, "N outside [1, 2^31)");
  REQUIRE(stride >= N, "stride < N");
  REQUIRE(bins >= 1 && bins <= MFG_DIST_MAX_BINS, "bins outside [1, MFG_DIST_MAX_BINS]");
  REQUIRE(G >= 0 && G <= MFG_DIST_MAX_GRID, "G outside [0, MFG_DIST_MAX_GRID]");
  REQUIRE(!use_range || (isfinite(lo) && isfinite(hi) && lo < hi), "histogram range: finite lo < hi needed");
  REQUIRE(G == 0 || (isfinite(x_lo) && isfinite(x_hi)), "KDE grid: finite x_lo, x_hi needed");
  REQUIRE(values && moments && counts && edges && status, "null pointer");
  REQUIRE(G == 0 || density, "density: null pointer with G > 0");
  const size_t need = mfg_row_distribution_workspace_bytes(R, N, bins, G);
  if (workspace_bytes < need || (need > 0 && !workspace))
    return fail(MFG_EWORKSPACE, "row distribution workspace: need %lld bytes, have %lld", (long long)need,
                (long long)workspace_bytes);
  RowDistArgs a{};
  a.values = values;
  a.N = N;
  a.stride = stride;
  a.bins = bins;
  a.use_range = use_range != 0;
  a.G = G;
  a.lo = lo;
  a.hi = hi;
  a.x_lo = x_lo;
  a.x_hi = x_hi;
  const double f = pow((double)N, -1.0 / 5.0);  // scipy.stats.gaussian_kde.scotts_factor for one dimension
  a.bw_factor = f * f;
  a.moments = moments;
  a.counts = counts;
  a.edges = edges;
  a.density = density;
  a.status = status;
  launch_row_distribution(a, R, S(stream));
  return check_launch("row_distribution");
}

extern "C" size_t mfg_action_mean_pop_workspace_bytes(int K, int64_t N, int d) {
  if (K < 1 || N < 1 || d < 1) return 0;
  return action_mean_workspace_bytes(K, N, d);
}

extern "C" int mfg_action_mean_pop(const float* action, int64_t s_action, int K, int64_t N, int d, double* mean, void* workspace,
                                   size_t workspace_bytes, mfg_stream_t stream) {
  REQUIRE(K >= 1 && K <= MFG_POP_MAX_K, "population size K outside [1, MFG_POP_MAX_K]");
  REQUIRE(N >= 1, "no matrices (N < 1)");
  REQUIRE(d >= 1, "d < 1");
  if (d > 64) return fail(MFG_EUNSUPPORTED, "mean action: d=%d > 64 (as for the populations)", d);
  REQUIRE(s_action == 0 || s_action >= N * (int64_t)d * d, "s_action: 0 (shared) or at least N d d");
  REQUIRE(action && mean && workspace, "null pointer");
  const size_t need = action_mean_workspace_bytes(K, N, d);
  if (workspace_bytes < need)
    return fail(MFG_EWORKSPACE, "mean action workspace: need %lld bytes, have %lld", (long long)need,
                (long long)workspace_bytes);
  launch_action_mean(action, s_action, K, N, d, mean, reinterpret_cast<double*>(workspace), S(stream));
  return check_launch("action_mean_pop");
}
