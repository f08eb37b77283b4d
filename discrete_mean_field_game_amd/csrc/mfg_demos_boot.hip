// The kernels of mfg_demos_bootstrap and mfg_replicate_bands and their entry points (mfg_demos_boot.h, include/mfg_hip.h).
#include <math.h>

#include "mfg_demos_boot.h"
#include "mfg_device.h"
#include "mfg_host.h"

namespace mfg {

// w = #{k < 12 : x >= T[k]}: Poisson(1) by inversion, T[k] = floor(2^32 sum_{j <= k} e^-1 / j!) (MFG_DEMOS_BOOT_TABLE)
__device__ __forceinline__ uint32_t boot_weight(uint32_t x) {
  constexpr uint32_t T[12] = MFG_DEMOS_BOOT_TABLE;
  uint32_t w = 0;
#pragma unroll
  for (int k = 0; k < 12; ++k) w += x >= T[k] ? 1u : 0u;
  return w;
}

__device__ __forceinline__ uint32_t boot_word(const u32x4& x, int i) { return i == 0 ? x.x : i == 1 ? x.y : i == 2 ? x.z : x.w; }

// the agent of slot s of a thread within its chunk (demos_load)
template <bool VEC>
__device__ __forceinline__ int boot_slot_agent(int s) {
  return VEC ? (s >> 2) * (DEMOS_THREADS * 4) + (int)threadIdx.x * 4 + (s & 3) : s * DEMOS_THREADS + (int)threadIdx.x;
}

// A workgroup owns the chunks g, g + groups, ... of one day for the replicates r0 .. r0 + rb - 1 (one quad of the generator, or
// one replicate).  LDS: [rb][hb] tiles of (width + 1)^2, then the day's rank bytes.  Hours in blocks of hb as k_demos_count.
template <bool VEC>
__global__ __launch_bounds__(DEMOS_THREADS) void k_boot_count(mfg_demos_boot_t f, int32_t* __restrict__ bad_flag,
                                                              int32_t* __restrict__ counts, int32_t* __restrict__ moves, int chunks,
                                                              int groups, int rblocks, int rb, int hb) {
  extern __shared__ int32_t lds[];
  const int tid = threadIdx.x, C = f.C, H = f.H, width = f.width, W1 = width + 1, T = W1 * W1, N = f.N;
  const int g = blockIdx.x % groups;
  const int r0 = (int)((blockIdx.x / groups) % rblocks) * rb;
  const int64_t n = blockIdx.x / ((int64_t)groups * rblocks);
  uint8_t* rk = reinterpret_cast<uint8_t*>(lds + rb * hb * T);
  bool bad = false;
  const int32_t* given = f.rank + (f.rank_rows == 1 ? 0 : n * C);
  for (int c = tid; c < C; c += DEMOS_THREADS) {
    const int r = given[c];
    bad = bad || r < -1 || r >= C;
    rk[c] = (uint8_t)((r >= 0 && r < width) ? r : width);
  }
  for (int i = tid; i < rb * hb * T; i += DEMOS_THREADS) lds[i] = 0;
  __syncthreads();
  const uint64_t day_key = f.unit == MFG_DEMOS_UNIT_AGENT ? 0ull : (uint64_t)(f.day_offset + n);
  const uint32_t c1 = (uint32_t)day_key, c2 = (uint32_t)(r0 >> 2), c3 = MFG_DEMOS_BOOT_TAG | ((uint32_t)(day_key >> 32) << 16);
  const uint32_t k0 = (uint32_t)f.seed, k1 = (uint32_t)(f.seed >> 32);
  for (int h0 = 0; h0 < H - 1; h0 += hb) {
    const int nb = H - 1 - h0 < hb ? H - 1 - h0 : hb;                    // transitions h0 + k -> h0 + k + 1, k < nb
    for (int chunk = g; chunk < chunks; chunk += groups) {
      const int64_t u0 = (int64_t)chunk * MFG_DEMOS_CHUNK;
      // the weights of the thread's slots: 4 bits per replicate of the block, two slots to a register
      uint32_t wq[DEMOS_SLOTS / 2];
#pragma unroll
      for (int s = 0; s < DEMOS_SLOTS; ++s) {
        const int64_t u = u0 + boot_slot_agent<VEC>(s);
        uint32_t ws = 0;
        if (u < f.U) {
          u32x4 c;
          c.x = (uint32_t)u, c.y = c1, c.z = c2, c.w = c3;
          const u32x4 x = philox4x32_10(c, k0, k1);
          for (int j = 0; j < rb; ++j)
            if (r0 + j < f.R) ws |= boot_weight(boot_word(x, (r0 + j) & 3)) << (4 * j);
        }
        if (s & 1) wq[s >> 1] |= ws << 16;
        else wq[s >> 1] = ws;
      }
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
        int32_t* tile = lds + k * T;
#pragma unroll
        for (int s = 0; s < DEMOS_SLOTS; ++s) {
          const int p = (prev[s >> 2] >> ((s & 3) * 8)) & 0xFF;
          const uint32_t ws = (wq[s >> 1] >> ((s & 1) * 16)) & 0xFFFFu;
          if ((p != width || cur[s] != width) && ws != 0) {
            const int key = p * W1 + cur[s];
#pragma unroll
            for (int j = 0; j < BOOT_RB; ++j) {                          // (rb = 1: the weights of j >= 1 are 0)
              const int32_t wj = (int32_t)((ws >> (4 * j)) & 15u);
              if (wj != 0) atomicAdd(&tile[j * hb * T + key], wj);
            }
          }
        }
#pragma unroll
        for (int q = 0; q < DEMOS_SLOTS / 4; ++q)
          prev[q] = (uint32_t)cur[4 * q] | (uint32_t)cur[4 * q + 1] << 8 | (uint32_t)cur[4 * q + 2] << 16 | (uint32_t)cur[4 * q + 3] << 24;
      }
    }
    __syncthreads();
    // tile k of replicate j is the transition h -> h + 1, h = h0 + k: cell (i, j) a move, row i a count of hour h, column j of
    // the last hour; "day" r N + n of the finishing pass
    for (int j = 0; j < rb && r0 + j < f.R; ++j) {
      const int32_t* tiles = lds + j * hb * T;
      const int64_t day = (int64_t)(r0 + j) * N + n;
      for (int cell = tid; cell < nb * T; cell += DEMOS_THREADS) {
        const int32_t a = tiles[cell];
        const int k = cell / T, c = cell - k * T, i = c / W1, jj = c - i * W1;
        if (a != 0 && i < width && jj < width) atomicAdd(&moves[((day * (H - 1) + h0 + k) * width + i) * width + jj], a);
      }
      for (int r = tid; r < nb * width; r += DEMOS_THREADS) {
        const int k = r / width, i = r - k * width;
        int32_t a = 0;
        for (int jj = 0; jj < W1; ++jj) a += tiles[k * T + i * W1 + jj];
        if (a != 0) atomicAdd(&counts[(day * H + h0 + k) * width + i], a);
      }
      if (h0 + nb == H - 1 && tid < width) {
        int32_t a = 0;
        for (int i = 0; i < W1; ++i) a += tiles[(nb - 1) * T + i * W1 + tid];
        if (a != 0) atomicAdd(&counts[(day * H + H - 1) * width + tid], a);
      }
    }
    __syncthreads();
    for (int i = tid; i < rb * hb * T; i += DEMOS_THREADS) lds[i] = 0;
    __syncthreads();
  }
  if (bad) atomicOr(&bad_flag[n], MFG_DEMOS_BAD_VALUE);
}

__global__ void k_boot_status(int32_t* __restrict__ status, const int32_t* __restrict__ bad_flag, int N, int64_t rows) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < rows && bad_flag[i % N] != 0) status[i] |= bad_flag[i % N];
}

template <bool VEC>
static void launch_boot_count(const mfg_demos_boot_t& f, const BootWs& w, int32_t* counts, int32_t* moves, hipStream_t st) {
  const int chunks = (int)((f.U + MFG_DEMOS_CHUNK - 1) / MFG_DEMOS_CHUNK);
  const BootTiles t = boot_tiles(f.H, f.C, f.width);
  const int rblocks = (f.R + t.rb - 1) / t.rb;
  const int64_t owners = (int64_t)f.N * rblocks;
  int groups = f.groups > 0 ? f.groups : (int)((2 * num_cus() + owners - 1) / owners);     // two workgroups per CU in all
  groups = groups < chunks ? groups : chunks;
  hipLaunchKernelGGL((k_boot_count<VEC>), dim3((unsigned)(owners * groups)), dim3(DEMOS_THREADS), t.lds_bytes, st, f, w.bad, counts,
                     moves, chunks, groups, rblocks, t.rb, t.hours);
}

static void launch_boot(const mfg_demos_boot_t& f, hipStream_t st) {
  const BootWs w = boot_layout(f.workspace, f.R, f.N, f.H, f.width);
  const int64_t days = (int64_t)f.R * f.N;
  int32_t* counts = f.counts ? f.counts : w.counts;
  int32_t* moves = f.moves ? f.moves : w.moves;
  (void)hipMemsetAsync(w.bad, 0, (size_t)f.N * 4, st);
  (void)hipMemsetAsync(counts, 0, (size_t)days * f.H * f.width * 4, st);
  (void)hipMemsetAsync(moves, 0, (size_t)days * (f.H - 1) * f.width * f.width * 4, st);
  if (f.U % 4 == 0 && (reinterpret_cast<uintptr_t>(f.topic) & 15) == 0) launch_boot_count<true>(f, w, counts, moves, st);
  else launch_boot_count<false>(f, w, counts, moves, st);
  // steps 5 to 7: the second mode of mfg_demos_from_logs over the R N days (it zeroes status first)
  mfg_demos_t m = {};
  m.state = f.state, m.action = f.action, m.counts = counts, m.moves = moves;
  m.present = f.present, m.left = f.left, m.entered = f.entered, m.status = f.status;
  m.N = (int32_t)days, m.H = f.H, m.C = f.C, m.d = f.d, m.width = f.width, m.empty_row = f.empty_row;
  launch_demos(m, st);
  hipLaunchKernelGGL(k_boot_status, dim3((unsigned)((days + 255) / 256)), dim3(256), 0, st, f.status, w.bad, f.N, days);
}

// BANDS_CELLS consecutive cells of x [R, cells]: v[r][c] in LDS (all 64 KiB of it at R = 1 024: no other shared array).
__global__ __launch_bounds__(BANDS_THREADS) void k_bands(mfg_replicate_bands_t b) {
  extern __shared__ float v[];
  const int tid = threadIdx.x, R = b.R;
  const int64_t cell0 = (int64_t)blockIdx.x * BANDS_CELLS;
  const int nc = b.cells - cell0 < BANDS_CELLS ? (int)(b.cells - cell0) : BANDS_CELLS;
  for (int i = tid; i < R * BANDS_CELLS; i += BANDS_THREADS) {
    const int r = i / BANDS_CELLS, c = i - r * BANDS_CELLS;
    v[i] = c < nc ? b.x[(int64_t)r * b.cells + cell0 + c] : 0.0f;
  }
  __syncthreads();
  if (tid < nc && (b.mean || b.std)) {
    const int64_t cell = cell0 + tid;
    bool nan = false;
    double s = 0.0;
    for (int r = 0; r < R; ++r) {
      const float x = v[r * BANDS_CELLS + tid];
      nan = nan || x != x;
      s = __dadd_rn(s, (double)x);
    }
    const double m = __ddiv_rn(s, (double)R);
    double q = 0.0;
    for (int r = 0; r < R; ++r) {
      const double e = __dsub_rn((double)v[r * BANDS_CELLS + tid], m);
      q = __dadd_rn(q, __dmul_rn(e, e));
    }
    if (b.mean) b.mean[cell] = nan ? (double)NAN : m;
    if (b.std) b.std[cell] = nan ? (double)NAN : __dsqrt_rn(__ddiv_rn(q, (double)R));
  }
  if (!b.quant) return;
  for (int i = tid; i < R * BANDS_CELLS; i += BANDS_THREADS) {
    const int r = i / BANDS_CELLS, c = i - r * BANDS_CELLS;
    if (c >= nc) continue;
    const float x = v[i];
    int rank = 0;                                                        // #{r' : v < x, or equal and r' < r}: a permutation
    bool nan = false;
    for (int o = 0; o < R; ++o) {
      const float y = v[o * BANDS_CELLS + c];
      nan = nan || y != y;
      rank += (y < x || (y == x && o < r)) ? 1 : 0;
    }
    for (int q = 0; q < b.Q; ++q)                                        // a NaN cell: member 0 writes every row
      if (nan ? r == 0 : rank == b.ranks[q]) b.quant[(int64_t)q * b.cells + cell0 + c] = nan ? NAN : x;
  }
}

}  // namespace mfg

using namespace mfg;

static bool boot_shape_ok(int R, int N, int H, int C, int width) {
  return R >= 1 && R <= MFG_DEMOS_BOOT_MAX_R && N >= 1 && H >= 2 && C >= 1 && C <= MFG_DEMOS_MAX_C && width >= 1 && width <= C &&
         width <= DEMOS_MAX_WIDTH && (int64_t)R * N * H <= INT32_MAX;
}

extern "C" size_t mfg_demos_bootstrap_workspace_bytes(int R, int N, int H, int C, int width) {
  if (!boot_shape_ok(R, N, H, C, width)) return 0;
  return boot_layout(nullptr, R, N, H, width).bytes;
}

extern "C" int mfg_demos_bootstrap(const mfg_demos_boot_t* boot) {
  REQUIRE(boot, "null descriptor");
  const mfg_demos_boot_t& f = *boot;
  REQUIRE(f.topic && f.status, "demos_bootstrap: null topic or status");
  REQUIRE(f.N >= 1 && f.H >= 2, "demos_bootstrap: N < 1 or H < 2");
  REQUIRE(f.R >= 1 && f.R <= MFG_DEMOS_BOOT_MAX_R, "demos_bootstrap: R outside [1, MFG_DEMOS_BOOT_MAX_R]");
  REQUIRE((int64_t)f.R * f.N * f.H <= INT32_MAX, "demos_bootstrap: R N H > 2^31 - 1");
  REQUIRE(f.d >= 1 && f.d <= f.width, "demos_bootstrap: d < 1 or d > width");
  REQUIRE(f.empty_row == MFG_DEMOS_EMPTY_UNIFORM || f.empty_row == MFG_DEMOS_EMPTY_IDENTITY, "demos_bootstrap: unknown empty_row");
  REQUIRE(f.groups >= 0, "demos_bootstrap: groups < 0");
  REQUIRE(f.U >= 1 && 12 * f.U <= INT32_MAX, "demos_bootstrap: U < 1 or 12 U > 2^31 - 1 (a weighted cell must fit int32)");
  REQUIRE(f.C >= 1 && f.C <= MFG_DEMOS_MAX_C, "demos_bootstrap: C outside [1, MFG_DEMOS_MAX_C]");
  REQUIRE(f.width <= f.C, "demos_bootstrap: width > C");
  REQUIRE(f.rank && (f.rank_rows == 1 || f.rank_rows == f.N), "demos_bootstrap: the rank table is null or has neither 1 nor N rows");
  REQUIRE(f.unit == MFG_DEMOS_UNIT_AGENT_DAY || f.unit == MFG_DEMOS_UNIT_AGENT, "demos_bootstrap: unknown unit");
  if (f.unit == MFG_DEMOS_UNIT_AGENT_DAY)
    REQUIRE(f.day_offset >= 0 && f.day_offset <= ((int64_t)1 << 48) - f.N, "demos_bootstrap: day_offset + n outside [0, 2^48)");
  if (f.width > DEMOS_MAX_WIDTH) return fail(MFG_EUNSUPPORTED, "demos_bootstrap: width=%d > %d", f.width, DEMOS_MAX_WIDTH);
  const int64_t chunks = (f.U + MFG_DEMOS_CHUNK - 1) / MFG_DEMOS_CHUNK;
  REQUIRE((int64_t)f.R * f.N * chunks <= INT32_MAX, "demos_bootstrap: more than 2^31 - 1 workgroups (R N chunks)");
  REQUIRE(f.workspace && (reinterpret_cast<uintptr_t>(f.workspace) & 7) == 0, "demos_bootstrap: workspace null or not 8-byte aligned");
  const size_t need = mfg_demos_bootstrap_workspace_bytes(f.R, f.N, f.H, f.C, f.width);
  if (f.workspace_bytes < need)
    return fail(MFG_EINVAL, "demos_bootstrap workspace: need %lld bytes, have %lld", (long long)need, (long long)f.workspace_bytes);
  launch_boot(f, S(f.stream));
  return check_launch("demos_bootstrap");
}

extern "C" int mfg_replicate_bands(const mfg_replicate_bands_t* bands) {
  REQUIRE(bands, "null descriptor");
  const mfg_replicate_bands_t& b = *bands;
  REQUIRE(b.x, "replicate_bands: null x");
  REQUIRE(b.R >= 1 && b.R <= MFG_DEMOS_BOOT_MAX_R, "replicate_bands: R outside [1, MFG_DEMOS_BOOT_MAX_R]");
  REQUIRE(b.cells >= 0 && (b.cells + BANDS_CELLS - 1) / BANDS_CELLS <= INT32_MAX, "replicate_bands: cells < 0 or too many");
  REQUIRE(b.Q >= 0 && b.Q <= MFG_FORECAST_MAX_RANKS, "replicate_bands: Q outside [0, MFG_FORECAST_MAX_RANKS]");
  REQUIRE(b.Q == 0 || b.quant, "replicate_bands: Q > 0 needs quant");
  for (int q = 0; q < b.Q; ++q) REQUIRE(b.ranks[q] >= 0 && b.ranks[q] < b.R, "replicate_bands: a rank outside [0, R)");
  if (b.cells == 0) return MFG_OK;
  mfg_replicate_bands_t k = b;
  if (k.Q == 0) k.quant = nullptr;
  hipLaunchKernelGGL(k_bands, dim3((unsigned)((b.cells + BANDS_CELLS - 1) / BANDS_CELLS)), dim3(BANDS_THREADS),
                     (size_t)b.R * BANDS_CELLS * 4, S(b.stream), k);
  return check_launch("replicate_bands");
}
