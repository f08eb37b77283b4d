// Finite-population kernels (mfg_agents.h): one resampling step of the A agents of every member, the forecast's row 0, and the
// entry point mfg_agents_step_pop.  mfg_forecast_agents_pop, which alternates the sampling kernel with k_agents_step, is with
// the other drivers in mfg_kernels.hip.
#include "mfg_core.h"
#include "mfg_agents.h"
#include "mfg_host.h"

namespace mfg {

constexpr int AG_CHUNK = 4 * WAVE;  // agents of one wave iteration: a Philox block (four words) per lane

__global__ __launch_bounds__(BLOCK) void k_agents_step(AgentsArgs a) {
  extern __shared__ double ag_lds[];
  __shared__ int bad_s;
  const int d = a.d, dd = d * d;
  double* stage = ag_lds;                                   // phase 1: [d (column), d (row)] S_ic, then t_ic in place
  uint64_t* tq = reinterpret_cast<uint64_t*>(stage);
  int32_t* mv = reinterpret_cast<int32_t*>(stage);          // phases 2, 3: [d, d] moves
  double* last_s = stage + dd;                              // [d] S_i,d-1
  uint32_t* thr = reinterpret_cast<uint32_t*>(last_s + d);  // [d, d] thresholds below 2^32 (the first cap_s[i] of row i)
  int32_t* n_s = reinterpret_cast<int32_t*>(thr + dd);      // [d] agents per row
  int32_t* cap_s = n_s + d;                                 // [d] thresholds of the row below 2^32
  const int k = blockIdx.y;
  const int64_t b = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & (WAVE - 1);
  const int wv = __builtin_amdgcn_readfirstlane(tid / WAVE);
  const int64_t m = (int64_t)k * a.B + b;
  // (no __restrict__: counts_next may be counts -- every count is read in phase 1 and written in phase 3, a member's own rows)
  const int32_t* cnt = a.counts + k * a.cs_k + b * a.cs_m;
  const float* __restrict__ P = a.P + m * dd;
  if (tid == 0) bad_s = 0;
  if (float* pc = a.P_copy ? a.P_copy + k * a.as_k + b * a.as_m : nullptr)
    for (int e = tid; e < dd; e += BLOCK) pc[e] = P[e];
  __syncthreads();

  // ---- phase 1: the thresholds.  Thread i adds up row i in column order (the one serial part: d adds per row, not per
  // element), all threads divide, thread i takes the running maxima ----
  if (tid < d) {
    const int n = cnt[tid];
    const float* __restrict__ row = P + tid * d;
    double S = 0.0;
    for (int c = 0; c < d; ++c) {
      S += (double)row[c];
      stage[c * d + tid] = S;
    }
    last_s[tid] = S;
    n_s[tid] = n;
    if (n < 0 || n > a.agents || (n > 0 && !(S > 0.0 && S < (double)INFINITY))) bad_s = 1;  // (whoever writes, writes 1)
  }
  __syncthreads();
  const bool bad = bad_s != 0;
  if (!bad) {
    for (int e = tid; e < dd; e += BLOCK) {
      const int i = e % d;
      uint64_t t = 0;
      if (n_s[i] > 0) {  // (a row with agents of a member that has not failed: its sum is finite and > 0)
        const double q = stage[e] / last_s[i] * 4294967296.0;
        t = q >= 4294967296.0 ? (1ull << 32) : (q > 0.0 ? (uint64_t)floor(q) : 0ull);
      }
      tq[e] = t;
    }
    __syncthreads();
    // the running maximum u_c = max(t_0 .. t_c): the first column with w < t_c is the first with w < u_c, and u ascends
    // (u = t unless P has negative entries), so that column is the number of u_c <= w
    if (tid < d) {
      uint64_t run = 0;
      int cap = 0;
      for (int c = 0; c < d; ++c) {
        const uint64_t t = tq[c * d + tid];
        run = t > run ? t : run;
        thr[tid * d + c] = (uint32_t)run;
        cap += run < (1ull << 32);
      }
      cap_s[tid] = cap;  // (u_d-1 = 2^32 in a row with agents: cap < d there)
    }
    __syncthreads();
    for (int e = tid; e < dd; e += BLOCK) mv[e] = 0;
  }
  __syncthreads();

  // ---- phase 2: the agents, chunk g of the member's chunks (rows in order) by wave g mod WAVES ----
  if (!bad) {
    const uint64_t j = a.traj_offset + (uint64_t)b;
    const uint64_t seed = a.seed[k];
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    int g = 0;
    for (int i = 0; i < d; ++i) {
      const int n = __builtin_amdgcn_readfirstlane(n_s[i]);
      const int nch = (n + AG_CHUNK - 1) / AG_CHUNK;
      int ch = (wv - g) & (WAVES - 1);
      g = (g + nch) & (WAVES - 1);
      if (ch >= nch) continue;
      const int cap = __builtin_amdgcn_readfirstlane(cap_s[i]);
      const int s0 = cap ? 1 << (31 - __clz(cap)) : 0;  // the largest power of two <= cap
      const uint32_t* tr = thr + i * d;
      int32_t* mr = mv + i * d;
      for (; ch < nch; ch += WAVES) {
        const uint32_t q = (uint32_t)ch * WAVE + lane;  // Philox block: agents 4 q .. 4 q + 3
        const int a0 = (int)(q * 4);
        u32x4 ctr;
        ctr.x = 0x80000000u | ((uint32_t)i << 22) | q;
        ctr.y = a.step;
        ctr.z = (uint32_t)j;
        ctr.w = (uint32_t)(j >> 32) & 0xFFFFu;
        const u32x4 r = philox4x32_10(ctr, k0, k1);
        const uint32_t w[4] = {r.x, r.y, r.z, r.w};
        int pos[4] = {0, 0, 0, 0};  // thresholds <= w among the first pos + s, bit by bit: four searches side by side
        for (int s = s0; s > 0; s >>= 1) {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int nx = pos[e] + s;
            const uint32_t tv = tr[min(nx, cap) - 1];
            pos[e] = (nx <= cap && tv <= w[e]) ? nx : pos[e];
          }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (a0 + e < n) atomicAdd(&mr[pos[e]], 1);  // (integers: the order does not matter)
      }
    }
  }
  __syncthreads();

  // ---- phase 3: the next counts and their histogram row ----
  if (tid < d) {
    int cn = -1;
    float pn = NAN;
    if (!bad) {
      cn = 0;
      for (int i = 0; i < d; ++i) cn += mv[i * d + tid];
      pn = (float)((double)cn / (double)a.agents);
    }
    a.counts_next[k * a.ns_k + b * a.ns_m + tid] = cn;
    if (a.pi_next) a.pi_next[k * a.ps_k + b * a.ps_m + tid] = pn;
    if (a.pi_cur && !bad) a.pi_cur[m * d + tid] = pn;
  }
  if (a.moves) {
    int32_t* mo = a.moves + m * dd;
    for (int e = tid; e < dd; e += BLOCK) mo[e] = bad ? -1 : mv[e];
  }
}

void launch_agents_step(const AgentsArgs& a, int K, hipStream_t st) {
  hipLaunchKernelGGL(k_agents_step, dim3((unsigned)a.B, (unsigned)K), dim3(BLOCK), agents_lds_bytes(a.d), st, a);
}

// element e = ((k NR + j) d + c): member j of group k starts from counts0[j mod N]
__global__ __launch_bounds__(BLOCK) void k_agents_init(const int32_t* __restrict__ counts0, int64_t N, int64_t NR, int H, int d,
                                                       int64_t total, int agents, int32_t* __restrict__ counts_traj,
                                                       float* __restrict__ pi_traj, float* __restrict__ pi_cur) {
  for (int64_t e = (int64_t)blockIdx.x * BLOCK + threadIdx.x; e < total; e += (int64_t)gridDim.x * BLOCK) {
    const int64_t mj = e / d;
    const int c = (int)(e - mj * d);
    const int32_t v = counts0[(mj % NR) % N * d + c];
    const float pi = (float)((double)v / (double)agents);
    counts_traj[mj * H * d + c] = v;
    pi_traj[mj * H * d + c] = pi;
    pi_cur[e] = pi;
  }
}

void launch_agents_init(const int32_t* counts0, int64_t N, int64_t NR, int H, int d, int K, int agents, int32_t* counts_traj,
                        float* pi_traj, float* pi_cur, hipStream_t st) {
  const int64_t total = (int64_t)K * NR * d;
  hipLaunchKernelGGL(k_agents_init, dim3((unsigned)grid_for(total, BLOCK, 8)), dim3(BLOCK), 0, st, counts0, N, NR, H, d, total, agents,
                     counts_traj, pi_traj, pi_cur);
}

}  // namespace mfg

using namespace mfg;

extern "C" int mfg_agents_step_pop(const int32_t* counts, const float* P, int64_t B, int d, int K, int agents, const uint64_t* seed,
                                   uint32_t step, uint64_t traj_offset, int32_t* counts_next, float* pi_next, int32_t* moves,
                                   mfg_stream_t stream) {
  REQUIRE(K >= 1 && K <= MFG_POP_MAX_K, "number of groups K outside [1, MFG_POP_MAX_K]");
  REQUIRE(B >= 0, "B < 0");
  REQUIRE(d >= 1, "d < 1");
  if (d > WAVE) return fail(MFG_EUNSUPPORTED, "finite population: d=%d > 64 (as for the populations)", d);
  REQUIRE(agents >= 1 && agents <= MFG_AGENTS_MAX, "agents outside [1, MFG_AGENTS_MAX]");
  REQUIRE(counts && P && seed && counts_next, "null pointer");
  REQUIRE(B <= 0x7FFFFFFF, "B too large for the grid");
  REQUIRE(traj_offset <= MFG_TRAJ_ID_LIMIT && (uint64_t)B <= MFG_TRAJ_ID_LIMIT - traj_offset,
          "member ids traj_offset + B exceed 2^48 (MFG_TRAJ_ID_LIMIT)");
  if (B == 0) return MFG_OK;
  AgentsArgs a{};
  a.counts = counts;
  a.cs_k = a.ns_k = a.ps_k = B * d;
  a.cs_m = a.ns_m = a.ps_m = d;
  a.P = P;
  a.counts_next = counts_next;
  a.pi_next = pi_next;
  a.moves = moves;
  a.seed = seed;
  a.B = B;
  a.d = d;
  a.agents = agents;
  a.step = step;
  a.traj_offset = traj_offset;
  launch_agents_step(a, K, S(stream));
  return check_launch("agents_step_pop");
}
