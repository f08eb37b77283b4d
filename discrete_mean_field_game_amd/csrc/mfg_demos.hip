// The four kernels of mfg_demos_from_logs and its entry points (mfg_demos.h, include/mfg_hip.h).
#include <math.h>

#include "mfg_demos.h"
#include "mfg_host.h"

namespace mfg {

// One unit added to tile[key] for every lane with `on`: an LDS atomic per lane.  COMBINE: first two rounds in which the first
// pending lane's cell is taken for every lane that hit it (one LDS atomic of the lane count); popular cells -- the diagonal of
// the largest topics -- go in the rounds, the tail does not loop.  Measured slower than the plain form at the probe's shape
// (profiles/demos_from_logs.txt), so it is not the default.  The whole wave calls this together.
template <bool COMBINE>
__device__ __forceinline__ void demos_add(int32_t* tile, int key, bool on) {
  if (COMBINE) {
    unsigned long long todo = __ballot(on);
#pragma unroll
    for (int round = 0; round < 2; ++round) {
      if (todo == 0) break;
      const int leader = __ffsll(todo) - 1;
      const int k = __builtin_amdgcn_readlane(key, leader);
      const unsigned long long same = __ballot(on && key == k);
      if ((int)(threadIdx.x & 63) == leader) atomicAdd(&tile[k], (int32_t)__popcll(same));
      on = on && key != k;
      todo &= ~same;
    }
  }
  if (on) atomicAdd(&tile[key], 1);
}

template <bool VEC, bool COMBINE>
__global__ __launch_bounds__(DEMOS_THREADS) void k_demos_keys(mfg_demos_t f, DemosWs w, int chunks, int all_hours) {
  extern __shared__ int32_t lds[];
  const int tid = threadIdx.x, C = f.C;
  const int64_t r = blockIdx.x / chunks;                 // the day (hour 0), or day H + hour
  const int64_t u0 = (int64_t)(blockIdx.x % chunks) * MFG_DEMOS_CHUNK;
  for (int c = tid; c < C; c += DEMOS_THREADS) lds[c] = 0;
  __syncthreads();
  const int32_t* row = f.topic + (all_hours ? r : r * f.H) * f.U + u0;
  int32_t v[DEMOS_SLOTS];
  demos_load<VEC>(row, f.U - u0, v);
#pragma unroll
  for (int s = 0; s < DEMOS_SLOTS; ++s) {
    const bool on = v[s] >= 0 && v[s] < C;
    demos_add<COMBINE>(lds, on ? v[s] : 0, on);
  }
  __syncthreads();
  unsigned long long* keys = w.keys + (all_hours ? 0 : r * C);
  for (int c = tid; c < C; c += DEMOS_THREADS)
    if (lds[c] != 0) atomicAdd(&keys[c], (unsigned long long)(uint32_t)lds[c]);
}

__global__ __launch_bounds__(DEMOS_RANK_THREADS) void k_demos_rank(mfg_demos_t f, DemosWs w) {
  __shared__ unsigned long long key[MFG_DEMOS_MAX_C];
  const int tid = threadIdx.x, C = f.C;
  const int64_t n = blockIdx.x;
  if (f.order_mode == MFG_DEMOS_ORDER_GIVEN) {
    const int32_t* given = f.order_given + (f.order_given_rows == 1 ? 0 : n * C);
    for (int c = tid; c < C; c += DEMOS_RANK_THREADS) f.order[n * C + c] = -1;
    __syncthreads();
    bool bad = false;
    for (int c = tid; c < C; c += DEMOS_RANK_THREADS) {
      int g = given[c];
      if (g < -1 || g >= C) bad = true, g = -1;
      w.rank[n * C + c] = g;
      if (g >= 0) f.order[n * C + g] = c;
    }
    if (bad) atomicOr(&f.status[n], MFG_DEMOS_BAD_VALUE);
    return;
  }
  for (int c = tid; c < C; c += DEMOS_RANK_THREADS) key[c] = w.keys[n * C + c];
  __syncthreads();
  const int days = f.order_mode == MFG_DEMOS_ORDER_TOTAL ? f.N : 1;      // (one workgroup in all: it writes every day's row)
  for (int c = tid; c < C; c += DEMOS_RANK_THREADS) {
    const unsigned long long k = key[c];
    int r = 0;
    for (int o = 0; o < C; ++o) r += (key[o] > k || (key[o] == k && o < c)) ? 1 : 0;
    for (int64_t m = n; m < n + days; ++m) w.rank[m * C + c] = r, f.order[m * C + r] = c;
  }
}

// A workgroup owns the chunks g, g + groups, ... of one day.  The hours go in blocks of `hb` transitions whose tiles sit in LDS
// together (all H - 1 when they fit: every hour is then read once; else the first hour of a block is read again): per chunk the
// block's first hour gives the ranks that stay in registers, every further hour one LDS update per agent; the tiles are folded
// and flushed once per block -- one global atomic per non-zero cell, row and (last hour) column of a workgroup, not of a chunk.
template <bool VEC, bool COMBINE>
__global__ __launch_bounds__(DEMOS_THREADS) void k_demos_count(mfg_demos_t f, DemosWs w, int chunks, int groups, int hb, int copies) {
  extern __shared__ int32_t lds[];
  const int tid = threadIdx.x, C = f.C, H = f.H, width = f.width, W1 = width + 1, T = W1 * W1;
  const int64_t n = blockIdx.x / groups;
  const int g = blockIdx.x % groups;
  uint8_t* rk = reinterpret_cast<uint8_t*>(lds + copies * hb * T);
  for (int c = tid; c < C; c += DEMOS_THREADS) {
    const int r = w.rank[n * C + c];
    rk[c] = (uint8_t)((r >= 0 && r < width) ? r : width);
  }
  for (int i = tid; i < copies * hb * T; i += DEMOS_THREADS) lds[i] = 0;
  __syncthreads();
  int32_t* tiles = lds + ((tid >> 6) % copies) * hb * T;
  bool bad = false;
  for (int h0 = 0; h0 < H - 1; h0 += hb) {
    const int nb = H - 1 - h0 < hb ? H - 1 - h0 : hb;                    // transitions h0 + k -> h0 + k + 1, k < nb
    for (int chunk = g; chunk < chunks; chunk += groups) {
      const int64_t u0 = (int64_t)chunk * MFG_DEMOS_CHUNK;
      const int32_t* row = f.topic + (n * H + h0) * f.U + u0;
      int32_t cur[DEMOS_SLOTS];
      uint32_t prev[DEMOS_SLOTS / 4];
      bad = demos_ranks<VEC>(row, f.U - u0, rk, C, width, cur) || bad;
#pragma unroll
      for (int q = 0; q < DEMOS_SLOTS / 4; ++q)
        prev[q] = (uint32_t)cur[4 * q] | (uint32_t)cur[4 * q + 1] << 8 | (uint32_t)cur[4 * q + 2] << 16 | (uint32_t)cur[4 * q + 3] << 24;
      for (int k = 0; k < nb; ++k) {
        row += f.U;
        bad = demos_ranks<VEC>(row, f.U - u0, rk, C, width, cur) || bad;
        int32_t* tile = tiles + k * T;
#pragma unroll
        for (int s = 0; s < DEMOS_SLOTS; ++s) {
          const int p = (prev[s >> 2] >> ((s & 3) * 8)) & 0xFF;
          demos_add<COMBINE>(tile, p * W1 + cur[s], p != width || cur[s] != width);
        }
#pragma unroll
        for (int q = 0; q < DEMOS_SLOTS / 4; ++q)
          prev[q] = (uint32_t)cur[4 * q] | (uint32_t)cur[4 * q + 1] << 8 | (uint32_t)cur[4 * q + 2] << 16 | (uint32_t)cur[4 * q + 3] << 24;
      }
    }
    __syncthreads();
    for (int cell = tid; cell < nb * T; cell += DEMOS_THREADS) {         // fold the copies into the first
      int32_t a = lds[cell];
      for (int k = 1; k < copies; ++k) a += lds[k * hb * T + cell], lds[k * hb * T + cell] = 0;
      lds[cell] = a;
    }
    __syncthreads();
    // tile k is the transition h -> h + 1, h = h0 + k: cell (i, j) a move, row i a count of hour h, column j of the last hour
    for (int cell = tid; cell < nb * T; cell += DEMOS_THREADS) {
      const int32_t a = lds[cell];
      const int k = cell / T, c = cell - k * T, i = c / W1, j = c - i * W1;
      if (a != 0 && i < width && j < width) atomicAdd(&w.moves[((n * (H - 1) + h0 + k) * width + i) * width + j], a);
    }
    for (int r = tid; r < nb * width; r += DEMOS_THREADS) {
      const int k = r / width, i = r - k * width;
      int32_t a = 0;
      for (int j = 0; j < W1; ++j) a += lds[k * T + i * W1 + j];
      if (a != 0) atomicAdd(&w.counts[(n * H + h0 + k) * width + i], a);
    }
    if (h0 + nb == H - 1 && tid < width) {
      int32_t a = 0;
      for (int i = 0; i < W1; ++i) a += lds[(nb - 1) * T + i * W1 + tid];
      if (a != 0) atomicAdd(&w.counts[(n * H + H - 1) * width + tid], a);
    }
    __syncthreads();
    for (int cell = tid; cell < nb * T; cell += DEMOS_THREADS) lds[cell] = 0;
    __syncthreads();
  }
  if (bad) atomicOr(&f.status[n], MFG_DEMOS_BAD_VALUE);
}

__global__ __launch_bounds__(DEMOS_THREADS) void k_demos_finish(mfg_demos_t f, const int32_t* __restrict__ cin,
                                                                const int32_t* __restrict__ moves_in) {
  __shared__ int32_t cnt[DEMOS_MAX_WIDTH], next[DEMOS_MAX_WIDTH], rowtot[DEMOS_MAX_WIDTH], colsum[DEMOS_MAX_WIDTH];
  __shared__ int failed, next_failed;
  const int tid = threadIdx.x, H = f.H, width = f.width, d = f.d;
  const int64_t n = blockIdx.x / H, row = blockIdx.x;        // row = n H + h
  const int h = (int)(row - n * H);
  const bool last = h == H - 1;
  const int32_t* m = last ? nullptr : moves_in + (row - n) * width * width;     // n (H-1) + h = row - n
  if (tid == 0) failed = 0, next_failed = 0;
  __syncthreads();
  if (tid < width) {
    cnt[tid] = cin[row * width + tid];
    next[tid] = last ? 0 : cin[(row + 1) * width + tid];
    if (cnt[tid] < 0) failed = 1;
    if (next[tid] < 0) next_failed = 1;
  }
  if (!last) {
    bool neg = false;
    for (int c = tid; c < width * width; c += DEMOS_THREADS) neg = neg || m[c] < 0;
    if (neg) failed = 1;
    if (tid < width) {
      int32_t a = 0;
      for (int j = 0; j < width; ++j) a += m[tid * width + j];
      rowtot[tid] = a;
    } else if (tid >= 64 && tid < 64 + width) {
      int32_t a = 0;
      for (int i = 0; i < width; ++i) a += m[i * width + (tid - 64)];
      colsum[tid - 64] = a;
    }
  }
  __syncthreads();
  const bool fail_here = failed != 0, fail_next = next_failed != 0;
  int32_t present = 0;
  for (int i = 0; i < width; ++i) present += cnt[i];
  if (tid == 0) {
    if (f.present) f.present[row] = fail_here ? -1 : present;
    const int bits = fail_here ? MFG_DEMOS_FAILED : (present == 0 ? MFG_DEMOS_EMPTY_HOUR : 0);
    if (bits) atomicOr(&f.status[n], bits);
  }
  if (f.topic && f.counts && tid < width) f.counts[row * width + tid] = cnt[tid];
  if (f.state && tid < d)
    f.state[row * d + tid] = (fail_here || present == 0) ? NAN : (float)((double)cnt[tid] / (double)present);
  if (last) return;
  const int64_t step = row - n;
  if (tid < width) {
    if (f.left) f.left[step * width + tid] = fail_here ? -1 : cnt[tid] - rowtot[tid];
    if (f.entered) f.entered[step * width + tid] = (fail_here || fail_next) ? -1 : next[tid] - colsum[tid];
  }
  if (f.topic && f.moves)
    for (int c = tid; c < width * width; c += DEMOS_THREADS) f.moves[step * width * width + c] = m[c];
  if (f.action) {
    const float uniform = (float)(1.0 / (double)d);
    for (int c = tid; c < d * d; c += DEMOS_THREADS) {
      const int i = c / d, j = c - i * d;
      float a;
      if (fail_here) a = NAN;
      else if (rowtot[i] > 0) a = (float)((double)m[i * width + j] / (double)rowtot[i]);
      else if (cnt[i] == 0 && f.empty_row == MFG_DEMOS_EMPTY_UNIFORM) a = uniform;
      else a = i == j ? 1.0f : 0.0f;
      f.action[step * d * d + c] = a;
    }
  }
}

template <bool VEC, bool COMBINE>
static void launch_demos_log(const mfg_demos_t& f, const DemosWs& w, hipStream_t st) {
  const int chunks = (int)((f.U + MFG_DEMOS_CHUNK - 1) / MFG_DEMOS_CHUNK);
  if (f.order_mode != MFG_DEMOS_ORDER_GIVEN) {
    const int all = f.order_mode == MFG_DEMOS_ORDER_TOTAL;
    const int64_t rows = all ? (int64_t)f.N * f.H : f.N;
    hipLaunchKernelGGL((k_demos_keys<VEC, COMBINE>), dim3((unsigned)(rows * chunks)), dim3(DEMOS_THREADS), (size_t)f.C * 4, st, f, w,
                       chunks, all);
  }
  hipLaunchKernelGGL(k_demos_rank, dim3((unsigned)(f.order_mode == MFG_DEMOS_ORDER_TOTAL ? 1 : f.N)), dim3(DEMOS_RANK_THREADS), 0, st,
                     f, w);
  const DemosTiles t = demos_tiles(f.H, f.C, f.width);
  int groups = f.groups > 0 ? f.groups : (2 * num_cus() + f.N - 1) / f.N;      // two workgroups per CU over the days
  groups = groups < chunks ? groups : chunks;
  hipLaunchKernelGGL((k_demos_count<VEC, COMBINE>), dim3((unsigned)((int64_t)f.N * groups)), dim3(DEMOS_THREADS), t.lds_bytes, st, f, w,
                     chunks, groups, t.hours, t.copies);
}

void launch_demos(const mfg_demos_t& f, hipStream_t st) {
  (void)hipMemsetAsync(f.status, 0, (size_t)f.N * 4, st);
  const int32_t *cin = f.counts, *moves_in = f.moves;
  if (f.topic) {
    const DemosWs w = demos_layout(f.workspace, f.N, f.H, f.C, f.width);
    (void)hipMemsetAsync(f.workspace, 0, w.bytes, st);
    const bool vec = f.U % 4 == 0 && (reinterpret_cast<uintptr_t>(f.topic) & 15) == 0;
    const bool combine = f.lds_update == MFG_DEMOS_LDS_COMBINE;
    if (vec && combine) launch_demos_log<true, true>(f, w, st);
    else if (vec) launch_demos_log<true, false>(f, w, st);
    else if (combine) launch_demos_log<false, true>(f, w, st);
    else launch_demos_log<false, false>(f, w, st);
    cin = w.counts, moves_in = w.moves;
  }
  hipLaunchKernelGGL(k_demos_finish, dim3((unsigned)((int64_t)f.N * f.H)), dim3(DEMOS_THREADS), 0, st, f, cin, moves_in);
}

}  // namespace mfg

using namespace mfg;

extern "C" size_t mfg_demos_workspace_bytes(int N, int H, int C, int width) {
  if (N < 1 || H < 2 || C < 1 || C > MFG_DEMOS_MAX_C || width < 1 || width > C || width > DEMOS_MAX_WIDTH) return 0;
  return demos_layout(nullptr, N, H, C, width).bytes;
}

extern "C" int mfg_demos_from_logs(const mfg_demos_t* demos) {
  REQUIRE(demos, "null descriptor");
  const mfg_demos_t& f = *demos;
  REQUIRE(f.status, "demos: null status");
  REQUIRE(f.N >= 1 && f.H >= 2, "demos: N < 1 or H < 2");
  REQUIRE((int64_t)f.N * f.H <= INT32_MAX, "demos: N H > 2^31 - 1");
  REQUIRE(f.d >= 1 && f.d <= f.width, "demos: d < 1 or d > width");
  REQUIRE(f.empty_row == MFG_DEMOS_EMPTY_UNIFORM || f.empty_row == MFG_DEMOS_EMPTY_IDENTITY, "demos: unknown empty_row");
  REQUIRE(f.lds_update == MFG_DEMOS_LDS_COMBINE || f.lds_update == MFG_DEMOS_LDS_PLAIN, "demos: unknown lds_update");
  REQUIRE(f.groups >= 0, "demos: groups < 0");
  if (f.topic) {
    REQUIRE(f.order, "demos: null order");
    REQUIRE(f.U >= 1 && f.U <= INT32_MAX, "demos: U outside [1, 2^31 - 1]");
    REQUIRE(f.C >= 1 && f.C <= MFG_DEMOS_MAX_C, "demos: C outside [1, MFG_DEMOS_MAX_C]");
    REQUIRE(f.width <= f.C, "demos: width > C");
    REQUIRE(f.order_mode == MFG_DEMOS_ORDER_FIRST_HOUR || f.order_mode == MFG_DEMOS_ORDER_TOTAL || f.order_mode == MFG_DEMOS_ORDER_GIVEN,
            "demos: unknown order_mode");
    if (f.order_mode == MFG_DEMOS_ORDER_GIVEN)
      REQUIRE(f.order_given && (f.order_given_rows == 1 || f.order_given_rows == f.N), "demos: a given order needs a table of 1 or N rows");
  } else {
    REQUIRE(f.counts && f.moves, "demos: without a log counts and moves are inputs");
  }
  if (f.width > DEMOS_MAX_WIDTH) return fail(MFG_EUNSUPPORTED, "demos: width=%d > %d", f.width, DEMOS_MAX_WIDTH);
  if (f.topic) {
    const int64_t chunks = (f.U + MFG_DEMOS_CHUNK - 1) / MFG_DEMOS_CHUNK;
    REQUIRE((int64_t)f.N * f.H * chunks <= INT32_MAX, "demos: more than 2^31 - 1 workgroups (N H chunks)");
    REQUIRE(f.workspace && (reinterpret_cast<uintptr_t>(f.workspace) & 7) == 0, "demos: workspace null or not 8-byte aligned");
    const size_t need = mfg_demos_workspace_bytes(f.N, f.H, f.C, f.width);
    if (f.workspace_bytes < need)
      return fail(MFG_EINVAL, "demos workspace: need %lld bytes, have %lld", (long long)need, (long long)f.workspace_bytes);
  }
  launch_demos(f, S(f.stream));
  return check_launch("demos_from_logs");
}
