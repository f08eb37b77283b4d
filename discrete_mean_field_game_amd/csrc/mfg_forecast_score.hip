// Proper scores of an ensemble forecast (mfg_forecast_score.h): CRPS, the rank counts and the energy score of one cell per
// workgroup, the per-hour means in a second launch, and the two C entry points.  The bitonic sort and the transposing load are
// k_forecast_reduce's (mfg_forecast_pop.hip), copied so that that unit's code stays as it is.
#include "mfg_forecast_score.h"

#include <math.h>

#include "mfg_host.h"

namespace mfg {

constexpr int FS_WAVE = 64;
constexpr int FS_BLOCK = 256;
constexpr int FS_WAVES = FS_BLOCK / FS_WAVE;
constexpr int FS_MAX_D = 64;
constexpr int FS_ROWS = 4;  // rows of the resident tile a wave takes per pass over a lane's member

// the xor butterfly over the 64 lanes (the order of wave_sum, mfg_device.h); every lane returns the total
template <typename T>
__device__ __forceinline__ T fs_wave_sum(T v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, FS_WAVE);
  return v;
}

__device__ __forceinline__ bool fs_nonfinite(float v) { return (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u; }
__device__ __forceinline__ bool fs_nonfinite(double v) { return ((unsigned)__double2hiint(v) & 0x7ff00000u) == 0x7ff00000u; }

struct ForecastScoreArgs {
  const float* traj;    // [K, N R, H, d]
  const float* emp32;   // [N, H, d]
  const double* emp64;  // [N, H, d]
  int64_t N;
  int H, d, R, P2, C;   // P2: power of two >= R; C: columns per chunk (score_chunk)
  double* crps;         // [K, N, H, d]
  int32_t *less, *equal;
  double* energy;       // [K, N, H] or NULL
  double* cell_crps;    // [K, N, H]
  const int32_t* state; // [K] activity states of a control block (a validation check), or NULL: policy k is skipped when != 0
};

// norms of the pairs (row a of tile ta, member j of tile tb) this thread owns, added to acc in ascending a; `diag`: ta == tb,
// only a < j counts.  Rows and the lane's member are clamped for the reads; what a clamped read gives is not added.
__device__ __forceinline__ void fs_tile_pairs(const float* __restrict__ tA, const float* __restrict__ tB, int na, int nb, int d,
                                              int st, bool diag, int wv, int lane, double& acc) {
  const float* bj = tB + min(lane, nb - 1) * st;
  for (int a0 = wv; a0 < na; a0 += FS_WAVES * FS_ROWS) {
    const float* ar[FS_ROWS];
    double s[FS_ROWS];
#pragma unroll
    for (int q = 0; q < FS_ROWS; ++q) {
      ar[q] = tA + min(a0 + q * FS_WAVES, na - 1) * st;
      s[q] = 0.0;
    }
    for (int c = 0; c < d; ++c) {
      const double b = (double)bj[c];
#pragma unroll
      for (int q = 0; q < FS_ROWS; ++q) {
        const double df = (double)ar[q][c] - b;
        s[q] = fma(df, df, s[q]);
      }
    }
#pragma unroll
    for (int q = 0; q < FS_ROWS; ++q) {
      const int a = a0 + q * FS_WAVES;
      if (a < na && lane < nb && (!diag || lane > a)) acc += sqrt(s[q]);
    }
  }
}

// ---- launch 1: the scores of cell (k, n, l) = (blockIdx.y, blockIdx.x / H, blockIdx.x mod H) ----
__global__ __launch_bounds__(FS_BLOCK) void k_forecast_score(ForecastScoreArgs a) {
  extern __shared__ float fs_lds[];
  __shared__ double s_y64[FS_MAX_D], s_crps[FS_MAX_D], s_part[FS_WAVES];
  __shared__ float s_y32[FS_MAX_D];
  __shared__ int s_less[FS_MAX_D], s_equal[FS_MAX_D];
  const int k = blockIdx.y;
  if (a.state && a.state[k] != 0) return;  // (a retired learner of a validation check; block-uniform, ahead of every barrier)
  const int64_t cell = blockIdx.x;
  const int64_t n = cell / a.H;
  const int l = (int)(cell - n * a.H);
  const int tid = threadIdx.x, lane = tid & (FS_WAVE - 1), wv = tid / FS_WAVE;
  const int R = a.R, P2 = a.P2, d = a.d, stride = P2 + 1;
  // member r of the cell is trajectory j = r N + n of learner k
  const float* __restrict__ base = a.traj + (((int64_t)k * a.N * R + n) * a.H + l) * d;
  const int64_t mstride = a.N * a.H * d;
  const int64_t ocell = (int64_t)k * a.N * a.H + cell;
  int bad = 0;
  if (tid < d) {
    const float y32 = a.emp32[cell * d + tid];
    const double y64 = a.emp64[cell * d + tid];
    s_y32[tid] = y32;
    s_y64[tid] = y64;
    bad = fs_nonfinite(y32) || fs_nonfinite(y64);
  }
  // ---- columns: counts, sum |x - y|, sort, the weighted sum of the ascending column ----
  for (int c0 = 0; c0 < d; c0 += a.C) {
    const int C = min(a.C, d - c0);
    for (int e = tid; e < R * C; e += FS_BLOCK) {
      const int r = e / C, c = e - r * C;
      const float v = base[r * mstride + c0 + c];
      bad |= fs_nonfinite(v);
      fs_lds[c * stride + r] = v;
    }
    if (P2 > R) {
      const int pad = P2 - R;
      for (int e = tid; e < pad * C; e += FS_BLOCK) {
        const int c = e / pad, p = e - c * pad;
        fs_lds[c * stride + R + p] = INFINITY;
      }
    }
    __syncthreads();  // (orders s_y32 / s_y64 too)
    for (int cb = 0; cb < C; cb += FS_WAVES) {
      const int ci = cb + wv;
      const bool active = ci < C;
      float* col = fs_lds + (active ? ci : 0) * stride;
      double A = 0.0;
      int lt = 0, eq = 0;
      if (active) {
        const float y32 = s_y32[c0 + ci];
        const double y64 = s_y64[c0 + ci];
        for (int r = lane; r < R; r += FS_WAVE) {
          const float x = col[r];
          lt += x < y32;
          eq += x == y32;
          A += fabs((double)x - y64);
        }
        A = fs_wave_sum(A);
        lt = fs_wave_sum(lt);
        eq = fs_wave_sum(eq);
      }
      // bitonic sort, ascending: step (kk, j) compares entries i and i | j, i the t-th index with bit j clear
      for (int kk = 2; kk <= P2; kk <<= 1)
        for (int j = kk >> 1; j > 0; j >>= 1) {
          if (active)
            for (int t = lane; t < (P2 >> 1); t += FS_WAVE) {
              const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), p = i | j;
              const float x = col[i], y = col[p];
              if ((i & kk) == 0 ? x > y : x < y) {
                col[i] = y;
                col[p] = x;
              }
            }
          __syncthreads();
        }
      if (active) {
        double S = 0.0;
        for (int i = lane; i < R; i += FS_WAVE) S += (double)(2 * i - R + 1) * (double)col[i];
        S = fs_wave_sum(S);
        if (lane == 0) {
          s_crps[c0 + ci] = A / (double)R - S / ((double)R * (double)R);
          s_less[c0 + ci] = lt;
          s_equal[c0 + ci] = eq;
        }
      }
    }
    __syncthreads();  // (the next chunk's load, or the first tile's, overwrites the columns)
  }
  // ---- energy: every unordered pair of members once, tile ta resident, tiles tb >= ta passing by ----
  double e_cell = 0.0;
  if (a.energy) {
    const int st = d | 1;
    float* tA = fs_lds;
    float* tB = fs_lds + FS_TILE * st;
    const int nt = (R + FS_TILE - 1) / FS_TILE;
    double acc = 0.0, accy = 0.0;
    for (int ta = 0; ta < nt; ++ta) {
      const int na = min(FS_TILE, R - ta * FS_TILE);
      for (int e = tid; e < na * d; e += FS_BLOCK) {
        const int r = e / d, c = e - r * d;
        tA[r * st + c] = base[(ta * FS_TILE + r) * mstride + c];
      }
      __syncthreads();
      if (wv == 0 && lane < na) {
        double s = 0.0;
        for (int c = 0; c < d; ++c) {
          const double df = (double)tA[lane * st + c] - s_y64[c];
          s = fma(df, df, s);
        }
        accy += sqrt(s);
      }
      fs_tile_pairs(tA, tA, na, na, d, st, true, wv, lane, acc);
      for (int tb = ta + 1; tb < nt; ++tb) {
        const int nb = min(FS_TILE, R - tb * FS_TILE);
        __syncthreads();  // (the last tile pair has been read)
        for (int e = tid; e < nb * d; e += FS_BLOCK) {
          const int r = e / d, c = e - r * d;
          tB[r * st + c] = base[(tb * FS_TILE + r) * mstride + c];
        }
        __syncthreads();
        fs_tile_pairs(tA, tB, na, nb, d, st, false, wv, lane, acc);
      }
      __syncthreads();  // (the next resident tile overwrites this one)
    }
    acc = fs_wave_sum(acc);
    accy = fs_wave_sum(accy);
    if (lane == 0) s_part[wv] = acc;
    __syncthreads();
    if (tid == 0) {
      double P = 0.0;
      for (int w = 0; w < FS_WAVES; ++w) P += s_part[w];
      e_cell = accy / (double)R - P / ((double)R * (double)R);
    }
  }
  bad = __syncthreads_or(bad);  // (orders s_crps, s_less, s_equal too)
  if (tid < d) {
    a.crps[ocell * d + tid] = bad ? (double)NAN : s_crps[tid];
    a.less[ocell * d + tid] = bad ? -1 : s_less[tid];
    a.equal[ocell * d + tid] = bad ? -1 : s_equal[tid];
  }
  if (tid == 0) {
    double t = 0.0;
    for (int c = 0; c < d; ++c) t += s_crps[c];
    a.cell_crps[ocell] = bad ? (double)NAN : t;
    if (a.energy) a.energy[ocell] = bad ? (double)NAN : e_cell;
  }
}

// ---- launch 2: summary[k, l] = (mean of crps over (n, c), mean of energy over n), block (l, k), one wave ----
__global__ __launch_bounds__(FS_WAVE) void k_forecast_score_summary(const double* __restrict__ cell_crps,
                                                                    const double* __restrict__ energy, int64_t N, int H, int d,
                                                                    double* __restrict__ summary,
                                                                    const int32_t* __restrict__ state) {
  const int l = blockIdx.x, k = blockIdx.y, lane = threadIdx.x;
  if (state && state[k] != 0) return;
  double s = 0.0, e = 0.0;
  for (int64_t n = lane; n < N; n += FS_WAVE) {
    const int64_t o = ((int64_t)k * N + n) * H + l;
    s += cell_crps[o];
    if (energy) e += energy[o];
  }
  s = fs_wave_sum(s);
  e = fs_wave_sum(e);
  if (lane == 0) {
    double* out = summary + ((int64_t)k * H + l) * 2;
    out[0] = s / ((double)N * (double)d);
    out[1] = energy ? e / (double)N : (double)NAN;
  }
}

int launch_forecast_score(const float* traj, int64_t N, int H, int d, int K, int repeats, const float* emp32, const double* emp64,
                          double* crps, int32_t* less, int32_t* equal, double* energy, double* summary, double* cell_crps,
                          hipStream_t st, const int32_t* state) {
  ForecastScoreArgs a{};
  a.state = state;
  a.traj = traj;
  a.emp32 = emp32;
  a.emp64 = emp64;
  a.N = N;
  a.H = H;
  a.d = d;
  a.R = repeats;
  a.P2 = score_p2(repeats);
  a.C = score_chunk(d, repeats);
  a.crps = crps;
  a.less = less;
  a.equal = equal;
  a.energy = energy;
  a.cell_crps = cell_crps;
  const size_t lds = score_lds_bytes(d, repeats, energy != nullptr);
  if (a.C < 1 || lds > FS_COL_BUDGET) return MFG_ELAUNCH;  // (never within MFG_FORECAST_MAX_REPEATS and d <= 64)
  hipLaunchKernelGGL(k_forecast_score, dim3((unsigned)(N * H), (unsigned)K), dim3(FS_BLOCK), lds, st, a);
  hipLaunchKernelGGL(k_forecast_score_summary, dim3((unsigned)H, (unsigned)K), dim3(FS_WAVE), 0, st, cell_crps, energy, N, H, d,
                     summary, state);
  return MFG_OK;
}

}  // namespace mfg

using namespace mfg;

extern "C" size_t mfg_forecast_score_workspace_bytes(int64_t N, int H, int d, int K, int repeats) {
  if (N < 1 || H < 1 || d < 1 || K < 1 || repeats < 1) return 0;
  return forecast_score_workspace_bytes(N, H, K);
}

extern "C" int mfg_forecast_score(const float* traj, int64_t N, int H, int d, int K, int repeats, const float* emp32,
                                  const double* emp64, double* crps, int32_t* less, int32_t* equal, double* energy,
                                  double* summary, void* workspace, size_t workspace_bytes, mfg_stream_t stream) {
  REQUIRE(K >= 1 && K <= MFG_POP_MAX_K, "population size K outside [1, MFG_POP_MAX_K]");
  REQUIRE(d >= 1, "d < 1");
  if (d > FS_MAX_D) return fail(MFG_EUNSUPPORTED, "forecast score: d=%d > 64 (as for the ensemble forecast)", d);
  REQUIRE(H >= 2, "horizon H < 2");
  REQUIRE(N >= 1, "no start states (N < 1)");
  REQUIRE(repeats >= 1, "repeats < 1");
  REQUIRE(N * (int64_t)H <= 0x7FFFFFFF, "N H too large for the grid");
  REQUIRE(traj && emp32 && emp64 && crps && less && equal && summary && workspace, "null pointer");
  if (repeats > MFG_FORECAST_MAX_REPEATS)
    return fail(MFG_EUNSUPPORTED, "forecast score: repeats=%d > MFG_FORECAST_MAX_REPEATS=%d", repeats, MFG_FORECAST_MAX_REPEATS);
  const size_t need = forecast_score_workspace_bytes(N, H, K);
  if (workspace_bytes < need)
    return fail(MFG_EWORKSPACE, "forecast score workspace: need %lld bytes, have %lld", (long long)need, (long long)workspace_bytes);
  REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, "workspace not 8-byte aligned");
  const int rc = launch_forecast_score(traj, N, H, d, K, repeats, emp32, emp64, crps, less, equal, energy, summary,
                                       reinterpret_cast<double*>(workspace), S(stream));
  if (rc != MFG_OK) return fail(rc, "%s", "forecast score: LDS request beyond the budget");
  return check_launch("forecast_score");
}
