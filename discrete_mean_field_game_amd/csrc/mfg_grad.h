// Batch sums of the actor-critic update (a6 / a8) and their fixed-order row reduction: the bodies and template kernels of
// mfg_batch_sums.hip that the population launches (mfg_population.hip, mfg_pop_resident.hip) run as well.  Each __global__ is a
// thin shell around a __device__ body, so these translation units run the same code.  The non-template shells (k_grad_partial,
// k_add_reward, k_reduce_partials) are in mfg_batch_sums.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mfg_core.h"

using namespace mfg;

// ---------------------------------------------------------------------------------------------
// a6/a8 batch sums: G = [ sum_n delta_n phi(pi_n) | sum delta_n g_n | sum r_n | N ].
// The quadratic block is sum_n delta_n pi_n pi_n^T (upper triangle): each block owns a chunk of
// samples (staged in LDS) x a chunk of 4*BLOCK outputs; partials go to the workspace and are summed
// in a fixed order by k_reduce_partials, so results are run-to-run deterministic.
// ---------------------------------------------------------------------------------------------
constexpr int MFG_GRAD_SMALL_MAX_D = 28;  // k_grad_mfma_small: d + 4 augmented entries fit two 16-wide halves
constexpr int GR_OUT_PER_THREAD = 4;
constexpr int GR_OUT_PER_BLOCK = GR_OUT_PER_THREAD * BLOCK;

struct GradArgs {
  const float* pi;  // sample n=(b,s): pi + b*stride_b + s*d
  int64_t stride_b;
  const double* delta;
  const double* g;
  const float* reward;
  int64_t N;
  int T, d, chunk;  // chunk = samples staged per iteration
  int64_t nsb;      // number of sample-blocks (grid.x)
  double* partial;  // [nsb][F+3]
  // in-kernel finalisation by the last block to finish (k_grad_small with few rows): G, optional parameter update
  int add_reward;     // delta_n <- delta_n + reward_n first (external reward arrived after the rollout); written back
  unsigned* counter;  // zero on entry, zero again on exit; NULL -> separate k_reduce_partials launch
  double* G;
  int accumulate, apply;
  double lr_c, lr_a;
  double *w, *theta, *reward_acc;
};

__device__ __forceinline__ void grad_partial_body(const GradArgs& a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const int d = a.d, Q = d * (d + 1) / 2, F = Q + d + 1, FO = F + 3;
  double* dl = reinterpret_cast<double*>(smem_raw);  // [chunk][3] delta, delta*g, reward
  float* sp = reinterpret_cast<float*>(dl + 3 * a.chunk);  // [chunk][d]
  const int tid = threadIdx.x;
  int oi[GR_OUT_PER_THREAD], oj[GR_OUT_PER_THREAD], kind[GR_OUT_PER_THREAD];
  double acc[GR_OUT_PER_THREAD];
#pragma unroll
  for (int u = 0; u < GR_OUT_PER_THREAD; ++u) {
    const int k = blockIdx.y * GR_OUT_PER_BLOCK + u * BLOCK + tid;
    acc[u] = 0.0;
    oi[u] = oj[u] = 0;
    if (k < Q) {
      // invert k = i*d - i(i-1)/2 + (j-i): largest i with start(i) <= k
      int i = (int)(((2.0 * d + 1.0) - sqrt((2.0 * d + 1.0) * (2.0 * d + 1.0) - 8.0 * (double)k)) * 0.5);
      while (i > 0 && feat_idx(i, i, d) > k) --i;
      while (i + 1 < d && feat_idx(i + 1, i + 1, d) <= k) ++i;
      oi[u] = i;
      oj[u] = i + (k - feat_idx(i, i, d));
      kind[u] = 0;
    } else if (k < Q + d) {
      oi[u] = k - Q;
      kind[u] = 1;
    } else if (k < FO) {
      kind[u] = 2 + (k - (Q + d));  // 2 bias, 3 delta*g, 4 reward, 5 count
    } else {
      kind[u] = -1;
    }
  }
  for (int64_t n0 = (int64_t)blockIdx.x * a.chunk; n0 < a.N; n0 += a.nsb * a.chunk) {
    const int cn = (int)((a.N - n0) < a.chunk ? (a.N - n0) : a.chunk);
    __syncthreads();
    for (int k = tid; k < cn * d; k += BLOCK) {
      const int q = k / d, c = k - q * d;
      const int64_t n = n0 + q;
      const int64_t b = n / a.T;
      const int s = (int)(n - b * a.T);
      sp[k] = a.pi[b * a.stride_b + (int64_t)s * d + c];
    }
    for (int q = tid; q < cn; q += BLOCK) {
      const double de = a.delta[n0 + q];
      dl[3 * q] = de;
      dl[3 * q + 1] = a.g ? de * a.g[n0 + q] : 0.0;
      dl[3 * q + 2] = a.reward ? (double)a.reward[n0 + q] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < GR_OUT_PER_THREAD; ++u) {
      double s_ = acc[u];
      if (kind[u] == 0) {
        for (int q = 0; q < cn; ++q) s_ = fma(dl[3 * q] * (double)sp[q * d + oi[u]], (double)sp[q * d + oj[u]], s_);
      } else if (kind[u] == 1) {
        for (int q = 0; q < cn; ++q) s_ = fma(dl[3 * q], (double)sp[q * d + oi[u]], s_);
      } else if (kind[u] == 2) {
        for (int q = 0; q < cn; ++q) s_ += dl[3 * q];
      } else if (kind[u] == 3) {
        for (int q = 0; q < cn; ++q) s_ += dl[3 * q + 1];
      } else if (kind[u] == 4) {
        for (int q = 0; q < cn; ++q) s_ += dl[3 * q + 2];
      } else if (kind[u] == 5) {
        s_ += (double)cn;
      }
      acc[u] = s_;
    }
  }
#pragma unroll
  for (int u = 0; u < GR_OUT_PER_THREAD; ++u) {
    const int k = blockIdx.y * GR_OUT_PER_BLOCK + u * BLOCK + tid;
    if (kind[u] >= 0) a.partial[(int64_t)blockIdx.x * FO + k] = acc[u];
  }
}

// Small d (d <= 28; compile-time for the reference's 21 and 15): ALL the batch sums of an update on the fp64 matrix cores.
// Per sample n two augmented vectors of length d + 4 <= 32,
//     a_n = [ delta pi_0 .. delta pi_{d-1} | delta | 1 | 0 | 0 ]        (A operand, "row" index i)
//     b_n = [ pi_0 .. pi_{d-1}             | 1 | g | r | 1 ]            (B operand, "column" index j)
// and C = sum_n a_n b_n^T holds every entry of G = [sum delta phi | sum delta g | sum r | N] in its upper triangle:
//     C[i][j], i <= j < d   = sum delta pi_i pi_j     (quadratic features)      C[i][d]     = sum delta pi_i   (linear)
//     C[d][d]   = sum delta (bias)     C[d][d+1] = sum delta g     C[d+1][d+2] = sum r     C[d+1][d+3] = N.
// v_mfma_f64_16x16x4_f64: a wave keeps the three 16 x 16 tiles (0,0), (0,1), (1,1) of the 32 x 32 product (12 fp64
// accumulators per lane) and retires FOUR samples per K step with three matrix instructions; lane (li = lane & 15,
// lk = lane >> 4) feeds entries li and 16 + li of sample 4 ks + lk, straight from global memory (pi_traj / delta / g /
// reward as the rollout left them; the next batch of K steps is loaded while this one is multiplied).  The round-2 kernel
// kept row i of the sum in d fp64 registers per lane and fetched pi_n[j] from LDS for every FMA: one LDS read per FMA,
// 109 us for the 983 040 samples of the bench rollout against ~20 us of matrix-core time here.
// Partial rows are combined in a fixed order (k_reduce_partials, or in-kernel by the last block for few rows): run-to-run
// deterministic, no floating-point atomics.
// Data path (second version): a wave works through chunks of 64 consecutive samples.  Their pi rows are fetched with d
// fully used load instructions (flat element e = 64 k + lane of the chunk -> sample e / d, entry e % d: consecutive lanes
// read consecutive floats except at trajectory boundaries), delta / g / reward with one load each (lane = sample), all
// into registers while the previous chunk is multiplied, then parked in the wave's own LDS region (compact rows, no
// block barrier) from where the 16 K steps of the chunk read their operands in the matrix layout.  The first version
// loaded the operands directly (5 load instructions per K step, delta / g / reward fetched by 16 lanes each): the
// kernel was bound by the vector-memory issue rate of the CU, 58 us whatever the occupancy.
constexpr int GS_CH = 64;  // samples per chunk = 16 K steps
#ifndef MFG_GS_BPC
#define MFG_GS_BPC 2  // blocks per CU of the launch (2 waves per SIMD: measured)
#endif

template <int D>
struct GradChunk {
  static constexpr int NL = D ? D : MFG_GRAD_SMALL_MAX_D;  // pi loads per lane and chunk
  float pi[NL];
  double de, dg;
  float rr;
};

// n0 = first sample of the chunk (wave uniform); (b0, s0) = its trajectory / step.  Sample n0 + j sits at trajectory
// b0 + (s0 + j) / T, step (s0 + j) % T: small integers, so the division is an fp32 multiply.  The multiply is exact for every
// T < 2^22 and puts step T - 1 behind the boundary from T = 6 556 022 on (oracle/grad_index_ref.py restates it,
// tests/test_grad_index_host.py checks every T): the host sends T >= 2^22 to the WIDE form, which counts the boundaries of a
// long trajectory with a compare -- for T >= 64 a chunk of 64 samples crosses at most one.
constexpr int MFG_GRAD_LONG_T = 1 << 22;
__device__ __forceinline__ int grad_boundaries_wide(int sj, int T, float invT) {
  return T >= GS_CH ? (int)(sj >= T) : (int)(((float)sj + 0.5f) * invT);
}
template <int D, bool WIDE>
__device__ __forceinline__ void grad_chunk_load(GradChunk<D>& c, const GradArgs& a, const double* gp, const float* rp, int d,
                                                int64_t n0, int64_t b0, int s0, int lane, float invT, float inv_d) {
  const int last = (int)((a.N - 1 - n0) < (GS_CH - 1) ? (a.N - 1 - n0) : (GS_CH - 1));  // last live sample of the chunk
  {
    const int64_t n = n0 + (lane < last ? lane : last);  // lane = sample for the per-sample scalars (clamped: masked at use)
    c.de = a.delta[n];
    c.dg = gp[n];
    c.rr = rp[n];
  }
  // The chunk's [64][d] block is contiguous in memory except for the rows the layout skips between trajectories
  // (stride_b - T d floats, the T+1-th state of pi_traj): element e of the block sits at  base + e + q extra,  q = number of
  // trajectory boundaries in front of its sample -- 32-bit arithmetic on a wave-uniform 64-bit base (the (b, s) form cost
  // two 64-bit multiplies and three 64-bit shifts-and-adds per load: 330 of the kernel's 790 VALU instructions per chunk,
  // and f64 VALU work does not overlap the f64 matrix instructions).  Wide strides and long trajectories (WIDE, chosen by the
  // host: skipped part >= 2^23 floats, or T >= MFG_GRAD_LONG_T) keep the general form.
  if constexpr (!WIDE) {
    const float* cb = a.pi + b0 * a.stride_b + (int64_t)s0 * d;
    const int extra = (int)(a.stride_b - (int64_t)a.T * d);
#pragma unroll
    for (int k = 0; k < GradChunk<D>::NL; ++k) {
      if (!D && k * WAVE >= GS_CH * d) {                  // run-time d: loads past the chunk are not needed
        c.pi[k] = 0.0f;
        continue;
      }
      int e = k * WAVE + lane;                            // flat element of the chunk's [64][d] block
      int j = (int)(((float)e + 0.5f) * inv_d);           // sample of the chunk (e < 64 * 28: exact in fp32)
      if (j > last) { j = last; e = last * d; }           // past the end of the batch / of a run-time-d chunk: any live entry
      const int q = (int)(((float)(s0 + j) + 0.5f) * invT);
      c.pi[k] = cb[(unsigned)(e + __mul24(q, extra))];
    }
  } else {
#pragma unroll
    for (int k = 0; k < GradChunk<D>::NL; ++k) {
      if (!D && k * WAVE >= GS_CH * d) {
        c.pi[k] = 0.0f;
        continue;
      }
      const int e = k * WAVE + lane;
      int j = (int)(((float)e + 0.5f) * inv_d);
      int col = e - j * d;
      if (j > last) { j = last; col = 0; }
      const int sj = s0 + j;
      const int q = grad_boundaries_wide(sj, a.T, invT);
      const int64_t off = (b0 + q) * a.stride_b + ((int64_t)(sj - q * a.T) * d + col);  // (T d need not fit 32 bits)
      c.pi[k] = a.pi[off];
    }
  }
}

template <int D, bool WIDE>
__device__ __forceinline__ void grad_mfma_small_body(const GradArgs& a) {
  const int d = D ? D : a.d;
  const int Q = d * (d + 1) / 2, F = Q + d + 1, FO = F + 3;
  constexpr int DMAX = D ? D : MFG_GRAD_SMALL_MAX_D;
  // per wave: pi rows [64][d] (+ 16 floats: the hi-half read of the last row may run past it), then per sample
  // (delta, g, reward as double) -- 64 x 3 doubles; the block reduction reuses the space
  constexpr int PI_FL = GS_CH * DMAX + 16;
  constexpr int W_BYTES = ((PI_FL * 4 + 15) / 16) * 16 + GS_CH * 3 * 8;
  constexpr int RED_BYTES = WAVES * 3 * 4 * WAVE * 8;
  __shared__ __attribute__((aligned(16))) unsigned char smem[(WAVES * W_BYTES > RED_BYTES) ? WAVES * W_BYTES : RED_BYTES];
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), wv = __builtin_amdgcn_readfirstlane(tid / WAVE);
  float* lpi = reinterpret_cast<float*>(smem + (size_t)wv * W_BYTES);
  double* lsc = reinterpret_cast<double*>(smem + (size_t)wv * W_BYTES + ((PI_FL * 4 + 15) / 16) * 16);
  const int li = lane & 15, lk = lane >> 4;
  // lane constants of the augmented entries li (lo half) and 16 + li (hi half)
  auto consts = [&](int idx, float& a_d, double& a_1, float& b_1, double& b_g, double& b_r) {
    a_d = idx == d ? 1.0f : 0.0f;       // a: delta at idx == d
    a_1 = idx == d + 1 ? 1.0 : 0.0;     // a: 1 at idx == d + 1
    b_1 = (idx == d || idx == d + 3) ? 1.0f : 0.0f;
    b_g = idx == d + 1 ? 1.0 : 0.0;
    b_r = idx == d + 2 ? 1.0 : 0.0;
  };
  float ad_lo, b1_lo, ad_hi, b1_hi;
  double a1_lo, a1_hi, bg_lo, br_lo, bg_hi, br_hi;
  consts(li, ad_lo, a1_lo, b1_lo, bg_lo, br_lo);
  consts(16 + li, ad_hi, a1_hi, b1_hi, bg_hi, br_hi);
  const bool pi_lo = li < d, pi_hi = 16 + li < d;
  const int ilo = pi_lo ? li : 0, ihi = pi_hi ? 16 + li : 0;
  // optional inputs: a valid address to load from, and whether the loaded value counts
  const bool has_g = a.g != nullptr, has_r = a.reward != nullptr;
  const double* gp = has_g ? a.g : a.delta;
  const float* rp = has_r ? a.reward : a.pi;
  v4d_t c00 = (v4d_t)(0.0), c01 = (v4d_t)(0.0), c11 = (v4d_t)(0.0);
  const float invT = 1.0f / (float)a.T, inv_d = 1.0f / (float)d;
  const int64_t NC = (a.N + GS_CH - 1) / GS_CH;           // chunks
  const int64_t W = (int64_t)gridDim.x * WAVES;           // waves of the launch
  const int64_t gw = (int64_t)blockIdx.x * WAVES + wv;
  GradChunk<D> nx;
  if (gw < NC) grad_chunk_load<D, WIDE>(nx, a, gp, rp, d, gw * GS_CH, (gw * GS_CH) / a.T, (int)((gw * GS_CH) % a.T), lane, invT, inv_d);
  for (int64_t ch = gw; ch < NC; ch += W) {
    const int64_t n0 = ch * GS_CH;
    // park the chunk in LDS (the previous chunk's reads are complete: wave-local barrier)
    __builtin_amdgcn_s_waitcnt(0xc07f);
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int k = 0; k < GradChunk<D>::NL; ++k)
      if (D || k * WAVE < GS_CH * d) lpi[k * WAVE + lane] = nx.pi[k];
    {
      const bool ok = n0 + lane < a.N;
      const double rr = (ok && has_r) ? (double)nx.rr : 0.0;
      double de = ok ? nx.de : 0.0;
      if (a.add_reward) {
        de += rr;
        if (ok) const_cast<double*>(a.delta)[n0 + lane] = de;  // the lane that owns sample n writes it back
      }
      lsc[3 * lane] = de;
      lsc[3 * lane + 1] = (ok && has_g) ? nx.dg : 0.0;
      lsc[3 * lane + 2] = rr;
    }
    const int nvalid = (int)((a.N - n0) < GS_CH ? (a.N - n0) : GS_CH);  // samples of this chunk (wave uniform)
    if (ch + W < NC) {
      const int64_t n1 = (ch + W) * GS_CH;
      grad_chunk_load<D, WIDE>(nx, a, gp, rp, d, n1, n1 / a.T, (int)(n1 % a.T), lane, invT, inv_d);
    }
    __builtin_amdgcn_s_waitcnt(0xc07f);
    __builtin_amdgcn_wave_barrier();
#pragma unroll 4
    for (int ks = 0; ks < GS_CH / 4; ++ks) {
      const int j = 4 * ks + lk;
      const float plo = lpi[j * d + ilo], phi = lpi[j * d + ihi];
      const double de = lsc[3 * j], dg = lsc[3 * j + 1];
      const double rr = lsc[3 * j + 2];
      const double one = j < nvalid ? 1.0 : 0.0;               // slots past the last sample hold zeros and count nothing
      double A_lo, B_lo;
      if constexpr (D >= 16) {  // entries 0 .. 15 are all state entries: no constants, no selects
        B_lo = (double)plo;
        A_lo = de * B_lo;
      } else {
        A_lo = fma(de, (double)(pi_lo ? plo : ad_lo), a1_lo * one);
        B_lo = fma(bg_lo, dg, fma(br_lo, rr, (double)(pi_lo ? plo : b1_lo)));
      }
      const double A_hi = fma(de, (double)(pi_hi ? phi : ad_hi), a1_hi * one);
      const double B_hi = fma(bg_hi, dg, fma(br_hi, rr, (double)(pi_hi ? phi : b1_hi)));
      // (timing ablations at the bench shape, 44 us: without these three instructions 24 us, without the chunk loads 38 us --
      //  the matrix-core time, 20 us, ADDS to the rest whatever the occupancy (1 / 2 / 4 blocks per CU: 49 / 44 / 44 us):
      //  the fp64 matrix instructions of this kernel do not hide behind its other work)
      c00 = __builtin_amdgcn_mfma_f64_16x16x4f64(A_lo, B_lo, c00, 0, 0, 0);
      c01 = __builtin_amdgcn_mfma_f64_16x16x4f64(A_lo, B_hi, c01, 0, 0, 0);
      c11 = __builtin_amdgcn_mfma_f64_16x16x4f64(A_hi, B_hi, c11, 0, 0, 0);
    }
  }
  __syncthreads();  // every wave is done with its staging region: the block reduction reuses the space
  double (*red)[3][4][WAVE] = reinterpret_cast<double (*)[3][4][WAVE]>(smem);
  // block reduction in a fixed order: every wave parks its tiles, then each output is added up over the WAVES copies
#pragma unroll
  for (int v = 0; v < 4; ++v) {
    red[wv][0][v][lane] = c00[v];
    red[wv][1][v][lane] = c01[v];
    red[wv][2][v][lane] = c11[v];
  }
  __syncthreads();
  double* out = a.partial + (int64_t)blockIdx.x * FO;
  for (int e = tid; e < 3 * 4 * WAVE; e += BLOCK) {
    const int t = e / (4 * WAVE), v = (e / WAVE) & 3, l = e & (WAVE - 1);
    // D[i][j] of a tile: lane l holds row (l >> 4) + 4 v, column l & 15 (f64 MFMA layout)
    const int gi = (t == 2 ? 16 : 0) + 4 * v + (l >> 4), gj = (t == 0 ? 0 : 16) + (l & 15);
    int k = -1;
    if (gj < d) {
      if (gi <= gj) k = feat_idx(gi, gj, d);
    } else if (gj == d) {
      if (gi <= d) k = Q + gi;            // linear terms, then the bias at gi == d
    } else if (gj == d + 1) {
      if (gi == d) k = F;                 // sum delta g
    } else if (gj == d + 2) {
      if (gi == d + 1) k = F + 1;         // sum r
    } else if (gj == d + 3) {
      if (gi == d + 1) k = F + 2;         // N
    }
    if (k >= 0) {
      double tsum = red[0][t][v][l];
#pragma unroll
      for (int q = 1; q < WAVES; ++q) tsum += red[q][t][v][l];
      out[k] = tsum;
    }
  }
  if (!a.counter) return;
  // Few rows (small batches, per-step updates): the last block to finish sums the rows in a fixed order, writes G
  // and, when asked, applies the parameter update -- one launch instead of three dependent ones.
  __shared__ int s_last;
  __threadfence();
  __syncthreads();
  if (tid == 0) s_last = (atomicAdd(a.counter, 1u) == gridDim.x - 1) ? 1 : 0;
  __syncthreads();
  if (!s_last) return;
  __threadfence();
  double* fin = &red[0][0][0][0];  // FO <= 32 * 33 / 2 + ... < 3 * 4 * 64 * WAVES doubles
  const int nrows = (int)gridDim.x;
  for (int k = tid; k < FO; k += BLOCK) {
    // plain loads: the agent-scope fence above already invalidated this CU's L1, and nothing here was read before it
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    const double* col = a.partial + k;
    int r = 0;
    for (; r + 7 < nrows; r += 8) {
      const double v0 = col[(int64_t)r * FO], v1 = col[(int64_t)(r + 1) * FO], v2 = col[(int64_t)(r + 2) * FO],
                   v3 = col[(int64_t)(r + 3) * FO], v4 = col[(int64_t)(r + 4) * FO], v5 = col[(int64_t)(r + 5) * FO],
                   v6 = col[(int64_t)(r + 6) * FO], v7 = col[(int64_t)(r + 7) * FO];
      s0 += v0;
      s1 += v1;
      s2 += v2;
      s3 += v3;
      s0 += v4;
      s1 += v5;
      s2 += v6;
      s3 += v7;
    }
    for (; r < nrows; ++r) s0 += col[(int64_t)r * FO];
    const double tot = (s0 + s1) + (s2 + s3);
    const double gk = a.accumulate ? a.G[k] + tot : tot;
    a.G[k] = gk;
    fin[k] = gk;  // (`red` as tiles was last read before the barriers around the completion counter)
  }
  __syncthreads();
  if (a.apply) {
    // identical arithmetic to k_apply_update
    const double count = fin[F + 2];
    if (count > 0.0) {
      const double inv = 1.0 / count;
      for (int k = tid; k < F; k += BLOCK) a.w[k] = updated_param(a.w[k], a.lr_c, fin[k], inv);
      if (tid == 0) {
        if (a.reward_acc) *a.reward_acc += fin[F + 1] * inv;
        *a.theta = updated_param(*a.theta, a.lr_a, fin[F], inv);
      }
    }
  }
  if (tid == 0) *a.counter = 0u;
}
template <int D, bool WIDE = false>
__global__ __launch_bounds__(BLOCK) void k_grad_mfma_small(GradArgs a) { grad_mfma_small_body<D, WIDE>(a); }

// ---------------------------------------------------------------------------------------------
// Critic-gradient sums on the fp64 matrix cores for d a multiple of 16 (d >= 64): the one GEMM-shaped piece of the
// path, M = sum_n delta_n pi_n pi_n^T = A B with A = (delta pi)^T [d x N], B = pi [N x d].  v_mfma_f64_16x16x4_f64:
// a wave owns up to 8 upper-triangle 16x16 tiles of M (4 fp64 accumulators per lane per tile), a block stages 32
// samples (fp32 rows + delta) in LDS and runs 8 K-steps of 4 samples over them; operands are widened / scaled on
// the way from LDS (2 LDS reads + 2 cvt + 1 mul per 2 048-flop MFMA instead of 3 LDS reads per FMA in
// k_grad_partial, which ran at 4.5 % of the fp64 peak: 3.1 ms per C3 rollout).  Split-K over grid.x with one partial
// row per x, tiles split over grid.y; the linear / scalar sums ride on the y = 0 blocks.  Deterministic.
// ---------------------------------------------------------------------------------------------
constexpr int GM_KC = 32;    // samples staged per chunk
#ifndef MFG_GM_TPW
#define MFG_GM_TPW 8
#endif
constexpr int GM_TPW = MFG_GM_TPW;    // max tiles per wave

// NPF > 0 (float4 staging, NPF = d / 32 sixteen-byte loads per thread and chunk): the NEXT chunk's rows and deltas are
// fetched into registers before this chunk's matrix instructions and committed to LDS after them, so the staging
// latency (every sample chunk is staged by all blockIdx.y slices) hides behind the MFMAs.  NPF == 0: unpipelined.
template <int NPF>
__device__ __forceinline__ void grad_mfma_body(const GradArgs& a, int tpw) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const int d = a.d, nt = d >> 4, pitch = d + 16;  // pitch = 16 mod 32: the four k-rows of an operand hit distinct banks
  const int Q = d * (d + 1) / 2, F = Q + d + 1, FO = F + 3;
  double* dl = reinterpret_cast<double*>(smem_raw);                  // [KC] delta
  double* red = dl + GM_KC;                                          // [4][BLOCK] scalar reduction scratch
  float* sp = reinterpret_cast<float*>(red + 4 * BLOCK);             // [KC][pitch] pi rows
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), wv = tid / WAVE;
  const int ntiles = nt * (nt + 1) / 2;
  // this wave's tiles: linear ids t0 .. t0+nmine-1 of the row-major upper-triangle tile list
  const int t0 = ((int)blockIdx.y * WAVES + wv) * tpw;
  int nmine = ntiles - t0;
  nmine = nmine < 0 ? 0 : (nmine > tpw ? tpw : nmine);
  int tr[GM_TPW], tc[GM_TPW];
#pragma unroll
  for (int i = 0; i < GM_TPW; ++i) {
    int t = t0 + i, r = 0;
    if (i < nmine) {
      while (t >= nt - r) {  // row r of the tile triangle holds nt - r tiles
        t -= nt - r;
        ++r;
      }
    } else {
      t = 0;
    }
    tr[i] = r;
    tc[i] = r + t;
  }
  v4d_t acc[GM_TPW];
#pragma unroll
  for (int i = 0; i < GM_TPW; ++i) acc[i] = (v4d_t)(0.0);
  const bool side = blockIdx.y == 0;  // also owns the linear and scalar sums
  double lin[4] = {0.0, 0.0, 0.0, 0.0}, s_d = 0.0, s_dg = 0.0, s_r = 0.0, s_n = 0.0;
  const int li = lane & 15, lk = lane >> 4;
  const double invT = 1.0 / (double)a.T;
  // register prefetch of a chunk (NPF > 0): thread -> (row q0 + rpp u, float4 column c4), no divisions per element
  const int dq = d >> 2, rpp = BLOCK / (dq > 0 ? dq : 1);
  const int q0 = tid / dq, c4 = tid - q0 * dq;
  float4 pf[NPF > 0 ? NPF : 1];
  double pf_de = 0.0, pf_dg = 0.0, pf_rr = 0.0;
  bool pf_on = false;
#define MFG_GM_FETCH(n0_)                                                                              \
  {                                                                                                    \
    const int cn_ = (int)((a.N - (n0_)) < GM_KC ? (a.N - (n0_)) : GM_KC);                              \
    _Pragma("unroll") for (int u = 0; u < NPF; ++u) {                                                  \
      const int q = q0 + u * rpp;                                                                      \
      pf[u] = make_float4(0.f, 0.f, 0.f, 0.f);                                                         \
      if (q < cn_) {                                                                                   \
        const int64_t n = (n0_) + q;                                                                   \
        const int64_t b = (int64_t)(((double)n + 0.5) * invT);                                         \
        pf[u] = *reinterpret_cast<const float4*>(a.pi + b * a.stride_b + (n - b * a.T) * d + 4 * c4);  \
      }                                                                                                \
    }                                                                                                  \
    pf_de = 0.0; pf_dg = 0.0; pf_rr = 0.0; pf_on = false;                                              \
    if (tid < cn_) {                                                                                   \
      const int64_t n = (n0_) + tid;                                                                   \
      pf_de = a.delta[n];                                                                              \
      pf_rr = a.reward ? (double)a.reward[n] : 0.0;                                                    \
      if (a.g) pf_dg = a.g[n];                                                                         \
      pf_on = true;                                                                                    \
    }                                                                                                  \
  }
  if (NPF > 0 && (int64_t)blockIdx.x * GM_KC < a.N) MFG_GM_FETCH((int64_t)blockIdx.x * GM_KC)
  for (int64_t n0 = (int64_t)blockIdx.x * GM_KC; n0 < a.N; n0 += (int64_t)gridDim.x * GM_KC) {
    const int cn = (int)((a.N - n0) < GM_KC ? (a.N - n0) : GM_KC);
    __syncthreads();
    if (NPF > 0) {
#pragma unroll
      for (int u = 0; u < NPF; ++u) *reinterpret_cast<float4*>(sp + (q0 + u * rpp) * pitch + 4 * c4) = pf[u];
      if (tid < GM_KC) {
        if (side && pf_on) {
          s_d += pf_de;
          if (a.g) s_dg = fma(pf_de, pf_dg, s_dg);
          s_r += pf_rr;
          s_n += 1.0;
        }
        dl[tid] = pf_de;
      }
      __syncthreads();
      const int64_t nn = n0 + (int64_t)gridDim.x * GM_KC;
      if (nn < a.N) MFG_GM_FETCH(nn)
    } else {
    if (a.chunk) {
      // rows are 16-byte aligned and BLOCK is a multiple of d/4: thread -> (row, float4 column) without divisions
      for (int q = q0; q < GM_KC; q += rpp) {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (q < cn) {
          const int64_t n = n0 + q;
          const int64_t b = (int64_t)(((double)n + 0.5) * invT);
          v = *reinterpret_cast<const float4*>(a.pi + b * a.stride_b + (n - b * a.T) * d + 4 * c4);
        }
        *reinterpret_cast<float4*>(sp + q * pitch + 4 * c4) = v;  // rows past the end are zero: they add nothing
      }
    } else {
      for (int k = tid; k < GM_KC * d; k += BLOCK) {
        const int q = k / d, c = k - q * d;
        float v = 0.0f;
        if (q < cn) {
          const int64_t n = n0 + q;
          const int64_t b = (int64_t)(((double)n + 0.5) * invT);
          v = a.pi[b * a.stride_b + (n - b * a.T) * d + c];
        }
        sp[q * pitch + c] = v;
      }
    }
    if (tid < GM_KC) {
      double de = 0.0;
      if (tid < cn) {
        const int64_t n = n0 + tid;
        de = a.delta[n];
        const double rr = a.reward ? (double)a.reward[n] : 0.0;
        if (side) {
          s_d += de;
          if (a.g) s_dg = fma(de, a.g[n], s_dg);
          s_r += rr;
          s_n += 1.0;
        }
      }
      dl[tid] = de;
    }
    __syncthreads();
    }
#pragma unroll
    for (int ks = 0; ks < GM_KC / 4; ++ks) {
      const int k = ks * 4 + lk;
      const double dk = dl[k];
      const float* row = sp + k * pitch + li;
#pragma unroll
      for (int i = 0; i < GM_TPW; ++i) {
        if (i < nmine) {
          const double av = dk * (double)row[tr[i] << 4];   // A[i = li][k] = delta_k pi_k[16 r + li]
          const double bv = (double)row[tc[i] << 4];        // B[k][j = li] = pi_k[16 c + li]
          acc[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc[i], 0, 0, 0);
        }
      }
    }
    if (side) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int c = tid + u * BLOCK;
        if (c < d) {
          double t = lin[u];
          for (int q = 0; q < GM_KC; ++q) t = fma(dl[q], (double)sp[q * pitch + c], t);
          lin[u] = t;
        }
      }
    }
  }
#undef MFG_GM_FETCH
  // D[i][j] of a tile: lane holds rows i = 4 v + lane / 16, v = 0..3, column j = lane % 16
  double* out = a.partial + (int64_t)blockIdx.x * FO;
#pragma unroll
  for (int i = 0; i < GM_TPW; ++i) {
    if (i < nmine) {
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int gi = (tr[i] << 4) + 4 * v + lk, gj = (tc[i] << 4) + li;
        if (gi <= gj) out[feat_idx(gi, gj, d)] = acc[i][v];
      }
    }
  }
  if (side) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int c = tid + u * BLOCK;
      if (c < d) out[Q + c] = lin[u];
    }
    __syncthreads();
    red[tid] = s_d;
    red[BLOCK + tid] = s_dg;
    red[2 * BLOCK + tid] = s_r;
    red[3 * BLOCK + tid] = s_n;
    __syncthreads();
    if (tid < 4) {
      double t = 0.0;
      for (int q = 0; q < GM_KC; ++q) t += red[tid * BLOCK + q];  // only threads < KC hold scalar partials
      out[Q + d + tid] = t;
    }
  }
}
template <int NPF>
__global__ __launch_bounds__(BLOCK) void k_grad_mfma(GradArgs a, int tpw) { grad_mfma_body<NPF>(a, tpw); }

// Sum nsb partial rows in a fixed order: block = 64 slices x 16 outputs (16 consecutive doubles = one 128-byte line per
// slice); slice s adds rows s, s+64, ... (eight loads in flight), the 64 slice sums are combined in slice order through
// LDS.  (Round 2: 16 slices x 64 outputs -- four blocks for the 256 outputs of d = 21, each thread a chain of 4-6
// dependent L2 round trips: 4.8-6 us for the 342-512 rows of a per-step update; now FO / 16 blocks and one or two rounds.)
constexpr int RP_SLICES = 64, RP_OUT = 16;
// `ap` != NULL (single-GPU training rollout, accumulate == 0): the parameter update rides along -- the number of samples
// is known on the host (count), so every output updates its own parameter without waiting for another block's sum:
// k < F: w[k] += lr_c G[k] / count; k == F: theta += lr_a G[F] / count; k == F+1: *reward_acc += G[F+1] / count
// (the arithmetic of k_apply_update).
struct ReduceApply {
  double lr_c, lr_a, count;
  double *w, *theta, *reward_acc;
  int on;
};
__device__ __forceinline__ void reduce_partials_body(const double* __restrict__ partial, int64_t nsb, int64_t FO, int accumulate,
                                                     double* __restrict__ G, const ReduceApply& ap) {
  __shared__ double red[RP_SLICES][RP_OUT + 1];
  const int lo = threadIdx.x & (RP_OUT - 1), sl = threadIdx.x / RP_OUT;
  const int64_t k = (int64_t)blockIdx.x * RP_OUT + lo;
  // the value this output updates (parameter / accumulator / running G): read FIRST, under the row reads -- read where it is
  // used it was one more dependent L2 round trip at the end of a kernel that is nothing but such round trips
  double old_val = 0.0, old_G = 0.0;
  if (sl == 0 && k < FO) {
    const int64_t F = FO - 3;
    if (accumulate) old_G = G[k];
    if (ap.on) {
      if (k < F) old_val = ap.w[k];
      else if (k == F) old_val = *ap.theta;
      else if (k == F + 1 && ap.reward_acc) old_val = *ap.reward_acc;
    }
  }
  double s = 0.0;
  if (k < FO) {
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    int64_t p = sl;
    for (; p + 7 * RP_SLICES < nsb; p += 8 * RP_SLICES) {
      const double v0 = partial[p * FO + k], v1 = partial[(p + RP_SLICES) * FO + k], v2 = partial[(p + 2 * RP_SLICES) * FO + k],
                   v3 = partial[(p + 3 * RP_SLICES) * FO + k], v4 = partial[(p + 4 * RP_SLICES) * FO + k],
                   v5 = partial[(p + 5 * RP_SLICES) * FO + k], v6 = partial[(p + 6 * RP_SLICES) * FO + k],
                   v7 = partial[(p + 7 * RP_SLICES) * FO + k];
      s0 += v0;
      s1 += v1;
      s2 += v2;
      s3 += v3;
      s0 += v4;
      s1 += v5;
      s2 += v6;
      s3 += v7;
    }
    // tail: up to seven rows, loaded together
    double t[7];
#pragma unroll
    for (int u = 0; u < 7; ++u) t[u] = (p + u * RP_SLICES < nsb) ? partial[(p + u * RP_SLICES) * FO + k] : 0.0;
    s0 += t[0];
    s1 += t[1];
    s2 += t[2];
    s3 += t[3];
    s0 += t[4];
    s1 += t[5];
    s2 += t[6];
    s = (s0 + s1) + (s2 + s3);
  }
  red[sl][lo] = s;
  __syncthreads();
  if (sl == 0 && k < FO) {
    double t0 = 0.0, t1 = 0.0, t2 = 0.0, t3 = 0.0;
#pragma unroll
    for (int q = 0; q < RP_SLICES; q += 4) {
      t0 += red[q][lo];
      t1 += red[q + 1][lo];
      t2 += red[q + 2][lo];
      t3 += red[q + 3][lo];
    }
    const double tot = (t0 + t1) + (t2 + t3);
    const double gk = accumulate ? old_G + tot : tot;
    G[k] = gk;
    if (ap.on) {
      const int64_t F = FO - 3;
      const double inv = 1.0 / ap.count;
      if (k < F) ap.w[k] = updated_param(old_val, ap.lr_c, gk, inv);
      else if (k == F) *ap.theta = updated_param(old_val, ap.lr_a, gk, inv);
      else if (k == F + 1 && ap.reward_acc) *ap.reward_acc = old_val + gk * inv;
    }
  }
}
