// The given-P env step (a3 + a4) for MI355X (gfx950 / CDNA4, wave64): pi' = pi P and the reward, HBM-bound -- every P is read
// once.  The kernels and the launch rule that chooses between them (launch_step_given_P; the entry point mfg_step_given_P in
// mfg_kernels.hip checks its arguments and calls it).  Two work decompositions:
//   small d (d <= 64): G = 64/d trajectories packed per wavefront, lane = (trajectory, column j); the d x d action matrices
//       are staged in LDS -- per block tile (k_step_small, k_step_small_unaligned) or, at d = 21 / 15, per wave
//       (k_step_wave, k_step_wave_batched).
//   large d (d > 64): one wavefront per trajectory, lanes own columns, rows are streamed from HBM with coalesced loads
//       (k_step_rows at d = 128 / 256, k_step_large otherwise); per-row quantities use wavefront reductions.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include <type_traits>

#include "../../include/mfg_hip.h"
#include "mfg_core.h"
#include "mfg_host.h"
#include "mfg_step.h"

using namespace mfg;

// ---------------------------------------------------------------------------------------------
// a3+a4, small d: HBM-bound.  Block = 4 waves, tile = 4*G consecutive trajectories whose P slab
// (contiguous in HBM) is copied flat with 16-byte loads into LDS; lane = (trajectory, column j).
// Per element the lane does: cvt, p^2, and three fp64 FMAs
//     pi'_j += p pi_i,   s1_j += pi_i p^2,   s2_j += pi_i^2 p^2        (reward_j = pi_j s1_j - s2_j)
// with (pi_i, pi_i^2) staged once per tile as fp64 pairs in LDS (one broadcast 16-byte read per row).
// D > 0: compile-time d (rows unrolled, immediate LDS offsets); D == 0: runtime d.
// ---------------------------------------------------------------------------------------------
// The P slab of the NEXT tile is prefetched into registers (PER 16-byte loads per thread, all in flight
// together) while the current tile is consumed from LDS, so each block keeps ~a tile of HBM traffic in
// flight at all times (the un-pipelined version spent 83 % of its wave cycles waiting: SQ_WAIT_ANY).
#ifndef MFG_STEP_UNROLL
#define MFG_STEP_UNROLL 3
#endif
// Streamed-once data: non-temporal loads (measured +5 % on the d=21 kernel, +8..12 % on the row kernels).
// Depth-2 register prefetch was tried and lost (3.8-4.9 TB/s): the extra 24 VGPRs cost a block per CU.
typedef float v4f_t __attribute__((ext_vector_type(4)));
#define MFG_STREAM_LOAD(p) __builtin_nontemporal_load(p)
#ifndef MFG_STEP_WAVES
#define MFG_STEP_WAVES 7
#endif
template <int KIND, int D, int PER>
__global__ __launch_bounds__(BLOCK, (PER <= 6 ? MFG_STEP_WAVES : 4)) void k_step_small(const float* __restrict__ pi, const float* __restrict__ P,
                                                      int64_t B, int d_rt, float* __restrict__ pi_next,
                                                      float* __restrict__ reward) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int d = D ? D : d_rt;
  const int G = WAVE / d, TB = WAVES * G, dd = d * d;
  float* tQ = smem;                  // [TB][d] pi (fp32; widened on the fly: VALU is idle here, LDS bytes are not)
  float* tP = smem + ((TB * d + 3) & ~3);  // [TB][d][d], 16-byte aligned
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), wv = tid / WAVE;
  const int t = lane / d, j = lane - t * d;
  const int p2 = next_pow2(d);
  const int64_t ntiles = (B + TB - 1) / TB;
  v4f_t pre[PER];
  float prepi = 0.0f;
  // prefetch of tile TT into registers (a macro, not a lambda: capturing pre[] by reference sends it to scratch)
#define MFG_STEP_PREFETCH(TT)                                                  \
  {                                                                            \
    const int64_t pb0 = (TT) * TB;                                             \
    const int pnb = (int)((B - pb0) < TB ? (B - pb0) : TB);                    \
    const int pn4 = (pnb * dd) >> 2;                                           \
    const v4f_t* s4 = reinterpret_cast<const v4f_t*>(P + pb0 * dd);            \
    _Pragma("unroll") for (int u = 0; u < PER; ++u) {                          \
      const int k = tid + u * BLOCK;                                           \
      pre[u] = (k < pn4) ? MFG_STREAM_LOAD(s4 + k) : (v4f_t)(0.0f);            \
    }                                                                          \
    prepi = (tid < pnb * d) ? pi[pb0 * d + tid] : 0.0f;                        \
  }
  if ((int64_t)blockIdx.x < ntiles) MFG_STEP_PREFETCH((int64_t)blockIdx.x)
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t b0 = tile * TB;
    const int nb = (int)((B - b0) < TB ? (B - b0) : TB);
    const int n = nb * dd, n4 = n >> 2;
    v4f_t* d4 = reinterpret_cast<v4f_t*>(tP);
#pragma unroll
    for (int u = 0; u < PER; ++u) {
      const int k = tid + u * BLOCK;
      if (k < n4) d4[k] = pre[u];
    }
    for (int k = (n4 << 2) + tid; k < n; k += BLOCK) tP[k] = P[b0 * dd + k];  // ragged last tile only
    if (tid < nb * d) tQ[tid] = prepi;
    __syncthreads();
    if (tile + gridDim.x < ntiles) MFG_STEP_PREFETCH(tile + gridDim.x)
    const int tl = wv * G + t;
    const bool valid = (t < G) && (tl < nb);
    const int tlc = valid ? tl : 0;
    const float* colp = tP + tlc * dd + j;
    const float* qv = tQ + tlc * d;
    double acc = 0.0, s1 = 0.0, s2 = 0.0;
    // rows in groups of col_group_rows(d) (mfg_device.h: three groups of seven at d = 21, the plain row order otherwise)
    const int dr = D ? D : d, grp = col_group_rows(dr);
    for (int g0 = 0; g0 < dr; g0 += grp) {
      double pa = 0.0, p1 = 0.0, p2 = 0.0;
#pragma unroll MFG_STEP_UNROLL
      for (int i = g0; i < g0 + grp && i < (D ? D : d); ++i) {
        const double p = (double)colp[i * d];
        const double qx = (double)qv[i];
        // u = pi_i P_ij is exact in fp64 (two fp32 factors), so acc += u equals the fma, and pi_i P_ij^2 = u p,
        // pi_i^2 P_ij^2 = u^2 are formed inside the fmas with the same single rounding as before: 4 fp64 ops, not 5
        const double u = p * qx;
        pa += u;
        if (KIND != MFG_REWARD_EXTERNAL) {
          p1 = fma(u, p, p1);
          if (KIND == MFG_REWARD_MFG_AC2) p2 = fma(u, u, p2);
        }
      }
      acc = g0 ? acc + pa : pa;
      s1 = g0 ? s1 + p1 : p1;
      s2 = g0 ? s2 + p2 : p2;
    }
    double racc = 0.0;
    if (KIND == MFG_REWARD_MFG_AC2) racc = fma((double)qv[j], s1, -s2);
    if (KIND == MFG_REWARD_SYNTHETIC) racc = -0.5 * s1;
    if (KIND != MFG_REWARD_EXTERNAL) racc = seg_sum(racc, j, d, p2);
    if (valid) {
      pi_next[(b0 + tl) * d + j] = (float)acc;
      if (KIND != MFG_REWARD_EXTERNAL && j == 0) reward[b0 + tl] = (float)racc;
    }
    __syncthreads();
  }
}

#undef MFG_STEP_PREFETCH

// ---------------------------------------------------------------------------------------------
// a3+a4, compile-time small d (21, 15), WAVE-PRIVATE tiles: each wavefront stages the contiguous slab of its own
// G = 64/D trajectories (16-byte loads from the enclosing aligned window, the few bytes of the neighbours that come
// along are never read back), so there is no block-wide barrier at all -- a wave waits only for its OWN prefetch --
// and the per-trajectory reward sum goes through the wave's LDS region (dead after its column walk) instead of a
// shuffle tree.  Same arithmetic and summation order as k_core_small's column pass.
// ---------------------------------------------------------------------------------------------
// Prefetch of tile TT (the G trajectories' slab, as 16-byte words of its enclosing aligned window) into pre[] / prepi.
// MFG_WAVE_PREFETCH: B is a multiple of lcm(G, 4) (the launcher splits off the remainder), so every tile is full and
// the slab is a whole number of 16-byte words: every word of a window lies inside it, the first PER-1 loads are
// unconditional and issue back to back; the last one clamps its lane's word index to the window.  (With per-load lane
// tests, partial register writes or a second code path for partial tiles the compiler serialised the loads with
// s_waitcnt vmcnt(0), or waited for the prefetch right after issuing it in order to copy the whole pre[] tuple through
// a phi -- 2x on the low-occupancy batched kernel.)
#define MFG_WAVE_PREFETCH(TT)                                                             \
  {                                                                                       \
    const int64_t f0 = (TT) * (int64_t)(G * DD);                                          \
    const int pn4 = (int)(((f0 & 3) + (int64_t)(G * DD) + 3) >> 2);                       \
    const v4f_t* src = P4 + (f0 >> 2);                                                    \
    _Pragma("unroll") for (int u = 0; u < PER; ++u) {                                     \
      /* every load unconditional (no phi over pre[]): lanes past the window re-read its last word */ \
      const int k = lane + u * WAVE;                                                      \
      pre[u] = MFG_STREAM_LOAD(src + (((u + 1) * WAVE <= ((G * DD) >> 2)) ? k : (k < pn4 ? k : pn4 - 1))); \
    }                                                                                     \
    prepi = pi[(TT) * (int64_t)(G * D) + (lane < G * D ? lane : G * D - 1)];              \
  }
// MFG_WAVE_PREFETCH_RAG: any B (the tail launch): word addresses clamped to the slab, the 1..3 floats after its last
// whole word are patched into LDS by MFG_WAVE_TAIL.
#define MFG_WAVE_PREFETCH_RAG(TT)                                                             \
  {                                                                                       \
    const int64_t f0 = (TT) * (int64_t)(G * DD);                                          \
    const int64_t a4 = f0 >> 2;                                                           \
    const int png = (int)((B - (TT) * G) < G ? (B - (TT) * G) : G);                       \
    const int pn4 = (int)(((f0 & 3) + (int64_t)png * DD + 3) >> 2);                       \
    _Pragma("unroll") for (int u = 0; u < PER; ++u) {                                     \
      const int k = lane + u * WAVE;                                                      \
      pre[u] = (v4f_t)(0.0f);                                                             \
      /* whole words only, address clamped to the slab: no partial register writes, so the PER loads issue back to  \
         back; the 1..3 floats after the last whole word are patched into LDS by MFG_WAVE_TAIL */                    \
      if (k < pn4) pre[u] = MFG_STREAM_LOAD(P4 + ((a4 + k) < total4 ? (a4 + k) : total4 - 1));                    \
    }                                                                                     \
    prepi = (lane < png * D) ? pi[(TT) * (int64_t)(G * D) + lane] : 0.0f;                 \
  }
// The 1..3 floats after the slab's last whole 16-byte word (B d^2 not a multiple of 4) belong to the LAST tile only: its
// wave copies them into its LDS window after the vector staging (wave-uniform test, off the hot path).
#define MFG_WAVE_TAIL(TT)                                                                  \
  if ((TT) == ntiles - 1 && ((B * DD) & 3)) {                                              \
    const int64_t w0 = total4 << 2;                                                        \
    if (lane < (int)((B * DD) & 3)) wP[(int)(w0 - ((((TT) * (int64_t)(G * DD)) >> 2) << 2)) + lane] = P[w0 + lane]; \
  }
template <int KIND, int D, bool RAG>
__global__ __launch_bounds__(BLOCK, MFG_STEP_WAVES) void k_step_wave(const float* __restrict__ pi, const float* __restrict__ P,
                                                                      int64_t B, float* __restrict__ pi_next,
                                                                      float* __restrict__ reward) {
  constexpr int G = WAVE / D, DD = D * D;
  constexpr int WF = ((G * DD + 6 + 3) / 4) * 4;        // floats of a wave's LDS window (16-byte multiple, + alignment slack)
  constexpr int PER = (WF / 4 + WAVE - 1) / WAVE;       // 16-byte loads per lane per tile
  __shared__ __attribute__((aligned(16))) float sP[WAVES][WF];
  __shared__ float sQ[WAVES][G * D];
  const int tid = threadIdx.x, lane = tid & (WAVE - 1);
  const int wv = __builtin_amdgcn_readfirstlane(tid / WAVE);  // wave-uniform by construction: keeps the tile bookkeeping scalar
  const int t = lane / D, j = lane - t * D;
  float* wP = sP[wv];
  float* wQ = sQ[wv];
  const int64_t total4 = (B * DD) >> 2;                 // whole 16-byte words of the slab
  const int64_t ntiles = (B + G - 1) / G;
  const int64_t nwaves = (int64_t)gridDim.x * WAVES;
  v4f_t pre[PER];
  float prepi = 0.0f;
  const v4f_t* P4 = reinterpret_cast<const v4f_t*>(P);
  int64_t tile = (int64_t)blockIdx.x * WAVES + wv;
  if (tile < ntiles) {
    if (RAG) MFG_WAVE_PREFETCH_RAG(tile) else MFG_WAVE_PREFETCH(tile)
  }
  for (; tile < ntiles; tile += nwaves) {
    const int ng = (int)((B - tile * G) < G ? (B - tile * G) : G);
    const int off = (int)((tile * (int64_t)(G * DD)) & 3);   // position of the slab inside its aligned window
    v4f_t* d4 = reinterpret_cast<v4f_t*>(wP);
#pragma unroll
    for (int u = 0; u < PER; ++u) {
      const int k = lane + u * WAVE;
      if (k < WF / 4) d4[k] = pre[u];
    }
    if (lane < G * D) wQ[lane] = prepi;
    if (RAG) MFG_WAVE_TAIL(tile)
    __builtin_amdgcn_s_waitcnt(0xc07f);
    __builtin_amdgcn_wave_barrier();
    if (tile + nwaves < ntiles) {
      if (RAG) MFG_WAVE_PREFETCH_RAG(tile + nwaves) else MFG_WAVE_PREFETCH(tile + nwaves)
    }
    const bool valid = (t < G) && (t < ng);
    const int tc = valid ? t : 0;
    const float* colp = wP + off + tc * DD + j;
    const float* qv = wQ + tc * D;
    double acc = 0.0, s1 = 0.0, s2 = 0.0;
    // rows in groups of col_group_rows(D) (mfg_device.h: three groups of seven at d = 21; one group = the plain row order at 15):
    // THE loop of rounds 2-5 with the running sums folded into the totals at the end of a group (all sums start from 0: 0 + u,
    // fma(u, p, 0) and 0 + P0 are exact -- the bits of col_walk_row)
    constexpr int GR = col_group_rows(D);
    double pa = 0.0, p1 = 0.0, p2 = 0.0;
#ifndef MFG_COLWALK_STEP
#define MFG_COLWALK_STEP 2  // developer switch: 2 seven rows per unrolled body (static folds), 3 MFG_STEP_UNROLL rows + a uniform test
#endif
    constexpr int UN = (MFG_COLWALK_STEP == 2 && GR < D) ? (D == 15 ? 8 : GR) : MFG_STEP_UNROLL;  // a whole number of groups per body
#pragma unroll UN
    for (int i = 0; i < D; ++i) {
      const double p = (double)colp[i * D];
      const double qx = (double)qv[i];
      const double u = p * qx;
      pa += u;
      if (KIND != MFG_REWARD_EXTERNAL) {
        p1 = fma(u, p, p1);
        if (KIND == MFG_REWARD_MFG_AC2) p2 = fma(u, u, p2);
      }
      if (GR < D && col_group_end(i, D)) {
        acc += pa;
        s1 += p1;
        s2 += p2;
        pa = p1 = p2 = 0.0;
      }
    }
    if (GR >= D) {
      acc = pa;
      s1 = p1;
      s2 = p2;
    }
    double racc = 0.0;
    if (KIND == MFG_REWARD_MFG_AC2) racc = fma((double)qv[j], s1, -s2);
    if (KIND == MFG_REWARD_SYNTHETIC) racc = s1;
    const int64_t b = tile * G + tc;
    if (valid) pi_next[b * D + j] = (float)acc;
    if (KIND != MFG_REWARD_EXTERNAL) {
      // the wave's tile region is dead now: park the column terms there (8-byte aligned line per trajectory)
      __builtin_amdgcn_s_waitcnt(0xc07f);
      __builtin_amdgcn_wave_barrier();
      double* line = reinterpret_cast<double*>(wP) + tc * (D + 1);
      if (valid) line[j] = racc;
      __builtin_amdgcn_s_waitcnt(0xc07f);
      __builtin_amdgcn_wave_barrier();
      if (valid && j == 0) {
        double r0 = 0.0, r1 = 0.0;
        int k = 0;
#pragma unroll 4
        for (; k + 1 < D; k += 2) {
          r0 += line[k];
          r1 += line[k + 1];
        }
        if (k < D) r0 += line[k];
        double r = r0 + r1;
        if (KIND == MFG_REWARD_SYNTHETIC) r *= -0.5;
        reward[b] = (float)r;
      }
      __builtin_amdgcn_s_waitcnt(0xc07f);
      __builtin_amdgcn_wave_barrier();
    }
  }
}

// ---------------------------------------------------------------------------------------------
// a3+a4, d = 21 / 15, LARGE batches: k_step_wave with the OUTPUT side rebuilt.  tools/micro/step_lab.hip (round 2) showed
// that the walk costs 4 % and the 4.5 % of bytes that are written cost 25 %: the same kernel without its stores streams at
// 6.95 TB/s, with them at 5.5, and with the stores aimed at an L2-resident scratch again at 7.05 -- it is the trickle of
// small writes reaching HBM in between the reads, not the store instructions.  So here a wave
//   * takes KB CONSECUTIVE tiles (KB*G trajectories), parks their pi' / rewards in its own LDS stash and writes them out
//     once per super tile as one contiguous burst of 16-byte stores (KB = 32 at d = 21: 8 KB of pi' per wave),
//   * issues those stores at device scope (sc1: written through the L2 right away instead of trickling out of it line by
//     line whenever the cache replaces one),
//   * and the grid is sized to 8 waves per CU with an equal number of super tiles per wave (the batch costs 42 KB of LDS
//     per block; more resident waves measured slower with the batched stores, fewer starve the read stream).
// Same arithmetic, same summation order, bit-identical outputs.  Measured on the 983 040-transition slab: 5.5 -> 6.4 TB/s.
// A ragged last super tile falls back to per-tile stores.
// ---------------------------------------------------------------------------------------------
// Device-scope (sc1) stores through the raw-buffer intrinsics (a plain C++ store cannot carry a scope; inline asm would
// hide the store from the compiler's hazard / waitcnt bookkeeping).  The base must be wave-uniform.
typedef unsigned int v4u_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ __amdgpu_buffer_rsrc_t out_rsrc(void* base) {
  return __builtin_amdgcn_make_buffer_rsrc(base, 0, 0x7fffffff, 0x27000);  // raw buffer, 32-bit dword format (gfx9 family)
}
__device__ __forceinline__ void store16_device_scope(__amdgpu_buffer_rsrc_t r, int byte_off, v4f_t v) {
  __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(v4u_t, v), r, byte_off, 0, 16 /* sc1 */);
}
__device__ __forceinline__ void store4_device_scope(__amdgpu_buffer_rsrc_t r, int byte_off, float v) {
  __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned int, v), r, byte_off, 0, 16 /* sc1 */);
}
template <int KIND, int D, int KB>
__global__ __launch_bounds__(BLOCK, 2) void k_step_wave_batched(const float* __restrict__ pi, const float* __restrict__ P,
                                                                 int64_t B, float* __restrict__ pi_next,
                                                                 float* __restrict__ reward) {
  constexpr int G = WAVE / D, DD = D * D;
  constexpr int WF = ((G * DD + 6 + 3) / 4) * 4;
  constexpr int PER = (WF / 4 + WAVE - 1) / WAVE;
  constexpr int NO = KB * G * D, NR = KB * G;          // floats of pi' / rewards per super tile
  constexpr bool REW = KIND != MFG_REWARD_EXTERNAL;
  static_assert(NO % 4 == 0 && NR % 4 == 0, "a super tile's outputs must be whole 16-byte words");
  __shared__ __attribute__((aligned(16))) float sP[WAVES][WF];
  __shared__ float sQ[WAVES][G * D];
  __shared__ __attribute__((aligned(16))) float sO[WAVES][NO];
  __shared__ __attribute__((aligned(16))) float sR[WAVES][NR];
  __shared__ double sL[WAVES][G * (D + 1)];  // per-trajectory line of the column terms of the reward
  const int tid = threadIdx.x, lane = tid & (WAVE - 1);
  const int wv = __builtin_amdgcn_readfirstlane(tid / WAVE);  // wave-uniform by construction: keeps the tile bookkeeping scalar
  const int t = lane / D, j = lane - t * D;
  const bool valid = t < G;  // every tile is full (B is a multiple of G)
  const int tc = valid ? t : 0;
  float* wP = sP[wv];
  float* wQ = sQ[wv];
  float* wO = sO[wv];
  float* wR = sR[wv];
  double* line = sL[wv] + tc * (D + 1);
  const int64_t ntiles = (B + G - 1) / G;
  const int64_t nsuper = (ntiles + KB - 1) / KB;
  const int64_t nwaves = (int64_t)gridDim.x * WAVES;
  v4f_t pre[PER];
  float prepi = 0.0f;
  const v4f_t* P4 = reinterpret_cast<const v4f_t*>(P);
  int64_t sup = (int64_t)blockIdx.x * WAVES + wv;
  if (sup * KB < ntiles) MFG_WAVE_PREFETCH(sup * KB)
  for (; sup < nsuper; sup += nwaves) {
    const bool full = (sup + 1) * (int64_t)(KB * G) <= B;  // every trajectory of the super tile exists: batched stores
    int oo = lane, ro = 0;  // running stash offsets of the tile (no per-tile multiply)
    int kk = 0;
#pragma unroll 1
    for (; kk < KB; ++kk, oo += G * D, ro += G) {
      const int64_t tile = sup * KB + kk;
      if (tile >= ntiles) break;  // wave-uniform (last super tile only)
      const int off = (int)((tile * (int64_t)(G * DD)) & 3);
      v4f_t* d4 = reinterpret_cast<v4f_t*>(wP);
#pragma unroll
      for (int u = 0; u < PER; ++u) {
        const int k = lane + u * WAVE;
        if (k < WF / 4) d4[k] = pre[u];
      }
      if (lane < G * D) wQ[lane] = prepi;
      __builtin_amdgcn_s_waitcnt(0xc07f);
      __builtin_amdgcn_wave_barrier();
      {
        const int64_t nxt = (kk + 1 < KB && tile + 1 < ntiles) ? tile + 1 : (sup + nwaves) * KB;
        if (nxt < ntiles) MFG_WAVE_PREFETCH(nxt)
      }
      const float* colp = wP + off + tc * DD + j;
      const float* qv = wQ + tc * D;
      double acc = 0.0, s1 = 0.0, s2 = 0.0;
      // The reward of the PREVIOUS tile is summed here, one line entry per row of this tile's walk, by every lane of
      // the trajectory (broadcast reads; the VALU is idle anyway): the per-tile serial phase of k_step_wave -- two wave
      // barriers and 21 dependent adds on one lane -- disappears into the walk.  Same order: even terms, odd terms.
      double r0 = 0.0, r1 = 0.0;
      // rows in groups of col_group_rows(D) (mfg_device.h: three groups of seven at d = 21; the plain row order at 15): the fully
      // unrolled walk of round 2 with the running sums folded at the end of a group (see k_step_wave)
      constexpr int GR = col_group_rows(D);
      double pa = 0.0, p1 = 0.0, p2 = 0.0;
#pragma unroll
      for (int i = 0; i < D; ++i) {
        const double p = (double)colp[i * D];
        const double qx = (double)qv[i];
        const double u = p * qx;
        pa += u;
        if (REW) {
          p1 = fma(u, p, p1);
          if (KIND == MFG_REWARD_MFG_AC2) p2 = fma(u, u, p2);
          if (i & 1) r1 += line[i];
          else r0 += line[i];
        }
        if (GR < D && col_group_end(i, D)) {
          acc += pa;
          s1 += p1;
          s2 += p2;
          pa = p1 = p2 = 0.0;
        }
      }
      if (GR >= D) {
        acc = pa;
        s1 = p1;
        s2 = p2;
      }
      double racc = 0.0;
      if (KIND == MFG_REWARD_MFG_AC2) racc = fma((double)qv[j], s1, -s2);
      if (KIND == MFG_REWARD_SYNTHETIC) racc = s1;
      const int64_t b = tile * G + tc;
      if (full) {
        if (valid) wO[oo] = (float)acc;
      } else if (valid) {
        pi_next[b * D + j] = (float)acc;
      }
      if (REW) {
        if (kk > 0 && valid) {  // the previous tile's reward (stash: every lane of the trajectory writes the same value,
          double r = r0 + r1;   // so the sums above stay in the walk instead of sinking into a one-lane branch)
          if (KIND == MFG_REWARD_SYNTHETIC) r *= -0.5;
          if (full) wR[ro - G + tc] = (float)r;
          else if (j == 0) reward[b - G] = (float)r;
        }
        __builtin_amdgcn_wave_barrier();  // every lane has read the line (LDS operations of a wave execute in order)
        if (valid) line[j] = racc;
        __builtin_amdgcn_wave_barrier();
      }
    }
    if (REW && kk > 0) {
      // the super tile's last reward: the one serial sum left
      __builtin_amdgcn_s_waitcnt(0xc07f);
      __builtin_amdgcn_wave_barrier();
      if (valid && j == 0) {
        double r0 = 0.0, r1 = 0.0;
        int k = 0;
#pragma unroll 4
        for (; k + 1 < D; k += 2) {
          r0 += line[k];
          r1 += line[k + 1];
        }
        if (k < D) r0 += line[k];
        double r = r0 + r1;
        if (KIND == MFG_REWARD_SYNTHETIC) r *= -0.5;
        if (full) wR[ro - G + tc] = (float)r;
        else reward[(sup * KB + kk - 1) * G + tc] = (float)r;
      }
    }
    if (full) {
      __builtin_amdgcn_s_waitcnt(0xc07f);
      __builtin_amdgcn_wave_barrier();
      const __amdgpu_buffer_rsrc_t ob = out_rsrc(pi_next + sup * (int64_t)NO);
      const v4f_t* s4 = reinterpret_cast<const v4f_t*>(wO);
      for (int k = lane; k < NO / 4; k += WAVE) store16_device_scope(ob, k * 16, s4[k]);
      if (REW) {
        const __amdgpu_buffer_rsrc_t rb = out_rsrc(reward + sup * (int64_t)NR);
        const v4f_t* sr4 = reinterpret_cast<const v4f_t*>(wR);
        for (int k = lane; k < NR / 4; k += WAVE) store16_device_scope(rb, k * 16, sr4[k]);
      }
      __builtin_amdgcn_s_waitcnt(0xc07f);
      __builtin_amdgcn_wave_barrier();
    }
  }
}

// Fallback for a P pointer that is not 16-byte aligned: scalar staging, no prefetch.
template <int KIND>
__global__ __launch_bounds__(BLOCK) void k_step_small_unaligned(const float* __restrict__ pi, const float* __restrict__ P,
                                                                int64_t B, int d, float* __restrict__ pi_next,
                                                                float* __restrict__ reward) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int G = WAVE / d, TB = WAVES * G, dd = d * d;
  double2* tQ = reinterpret_cast<double2*>(smem);
  float* tP = reinterpret_cast<float*>(tQ + TB * d);
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), wv = tid / WAVE;
  const int t = lane / d, j = lane - t * d;
  const int p2 = next_pow2(d);
  const int64_t ntiles = (B + TB - 1) / TB;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t b0 = tile * TB;
    const int nb = (int)((B - b0) < TB ? (B - b0) : TB);
    for (int k = tid; k < nb * dd; k += BLOCK) tP[k] = P[b0 * dd + k];
    for (int k = tid; k < nb * d; k += BLOCK) {
      const double v = (double)pi[b0 * d + k];
      tQ[k] = make_double2(v, v * v);
    }
    __syncthreads();
    const int tl = wv * G + t;
    const bool valid = (t < G) && (tl < nb);
    const int tlc = valid ? tl : 0;
    const float* colp = tP + tlc * dd + j;
    const double2* qv = tQ + tlc * d;
    double acc = 0.0, s1 = 0.0, s2 = 0.0;
    const int grp = col_group_rows(d);  // (mfg_device.h: pi' of the aligned kernels bit for bit, also at d = 21)
    for (int g0 = 0; g0 < d; g0 += grp) {
      double pa = 0.0, p1 = 0.0, p2 = 0.0;
      for (int i = g0; i < g0 + grp && i < d; ++i) {
        const double p = (double)colp[i * d];
        const double2 q = qv[i];
        const double pp = p * p;
        pa = fma(p, q.x, pa);
        p1 = fma(q.x, pp, p1);
        p2 = fma(q.y, pp, p2);
      }
      acc = g0 ? acc + pa : pa;
      s1 = g0 ? s1 + p1 : p1;
      s2 = g0 ? s2 + p2 : p2;
    }
    double racc = 0.0;
    if (KIND == MFG_REWARD_MFG_AC2) racc = fma(qv[j].x, s1, -s2);
    if (KIND == MFG_REWARD_SYNTHETIC) racc = -0.5 * s1;
    if (KIND != MFG_REWARD_EXTERNAL) racc = seg_sum(racc, j, d, p2);
    if (valid) {
      pi_next[(b0 + tl) * d + j] = (float)acc;
      if (KIND != MFG_REWARD_EXTERNAL && j == 0) reward[b0 + tl] = (float)racc;
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------------
// a3+a4, d = 4*LPR (d = 128: LPR = 32, d = 256: LPR = 64): one wavefront per trajectory, every lane issues
// 16-byte loads and one wave instruction covers 64/LPR consecutive rows (1 KiB, fully coalesced).  8-byte
// or half-populated loads reach only ~0.55x of this rate (the d = 128 case of k_step_large).  The lane
// groups that hold the same columns of different rows are combined with xor-shuffles at the end.
// ---------------------------------------------------------------------------------------------
#ifndef MFG_ROWS_UNROLL
#define MFG_ROWS_UNROLL 8   // row groups (1 KiB wave loads) per chunk; two chunks are in flight / in use per wave
#endif
#ifndef MFG_ROWS_BPC
#define MFG_ROWS_BPC 2      // resident blocks per CU the grid is sized for (8 waves per CU)
#endif
#ifndef MFG_ROWS_KT
#define MFG_ROWS_KT 8       // consecutive trajectories per wave whose outputs are written as one burst (large batches)
#endif
#ifndef MFG_ROWS_ABL_NOREW   // timing ablations (tools/variant.sh): drop the reward sums / the output stores
#define MFG_ROWS_ABL_NOREW 0
#endif
#ifndef MFG_ROWS_ABL_NOSTORE
#define MFG_ROWS_ABL_NOSTORE 0
#endif
#ifndef MFG_ROWS_ABL_NOMATH
#define MFG_ROWS_ABL_NOMATH 0
#endif
// Round 2: a CONTINUOUS load stream per wave.  The first version loaded pi, staged it, and only then started the row
// loads of a trajectory -- two serial memory latencies per trajectory during which the wave streamed nothing (12 % of
// the time at d = 128, fitted from the d = 128 / 256 rates) -- and ran 32 waves per CU.  Now the rows are consumed in
// chunks of U row groups from two register buffers (ping-pong): while one chunk is multiplied the next one is in flight,
// and the chunk after a trajectory's last is the FIRST chunk of the wave's next trajectory, issued before the reduction /
// stores of the current one; the next trajectory's state is prefetched into registers at the start of the current one.
// 8 waves per CU (more resident waves measured slower: d = 256 6.5 TB/s at 32 waves/CU, 6.9-7.0 at 8), outputs stored at
// device scope (sc1).  Per-lane summation order is unchanged (rows in increasing order) => bit-identical results.
// KT > 1: a wave takes KT CONSECUTIVE trajectories (a super tile), parks their pi' / rewards in its LDS stash and writes
// them as one contiguous burst (the d = 21 finding: it is the trickle of small writes between the reads that costs
// bandwidth -- the 0.8 % of bytes written here cost 6 % at d = 128).  KT = 1 (small batches): direct stores.
template <int KIND, int LPR, int KT>
__global__ __launch_bounds__(BLOCK, 2) void k_step_rows(const float* __restrict__ pi, const float* __restrict__ P, int64_t B,
                                                        float* __restrict__ pi_next, float* __restrict__ reward) {
  constexpr int d = 4 * LPR, RPW = WAVE / LPR;
  constexpr int U = MFG_ROWS_UNROLL;
  constexpr int CPT = d / RPW / U;   // chunks per trajectory
  constexpr int NQ = d / WAVE;       // state entries per lane
  static_assert(CPT >= 2 && CPT % 2 == 0, "ping-pong needs an even number of chunks per trajectory");
  static_assert(KT == 1 || KT % 4 == 0, "a super tile's rewards must be whole 16-byte words");
  __shared__ double2 qs[WAVES][d];  // (pi_i, pi_i^2) fp64 per wave
  __shared__ __attribute__((aligned(16))) float sO[WAVES][KT > 1 ? KT * d : 4];
  __shared__ __attribute__((aligned(16))) float sR[WAVES][KT > 1 ? KT : 4];
  const int tid = threadIdx.x, lane = tid & (WAVE - 1);
  const int wv = __builtin_amdgcn_readfirstlane(tid / WAVE);
  const int sub = lane / LPR, c4 = lane - sub * LPR;
  double2* q = qs[wv];
  float* wO = sO[wv];
  float* wR = sR[wv];
  const int64_t nw = (int64_t)gridDim.x * WAVES;
  const int64_t nsup = (B + KT - 1) / KT;
  int64_t sup = (int64_t)blockIdx.x * WAVES + wv;
  if (sup >= nsup) return;
  v4f_t va[U], vb[U];
  float pnx[NQ];
  // chunk c of trajectory bb -> register buffer BUF (U wave-wide 1 KiB loads)
#define MFG_ROWS_ISSUE(BUF, bb, c)                                                                          \
  {                                                                                                         \
    const v4f_t* src = reinterpret_cast<const v4f_t*>(P + (bb) * (int64_t)d * d) + (c) * (U * WAVE) + lane; \
    _Pragma("unroll") for (int u = 0; u < U; ++u) BUF[u] = MFG_STREAM_LOAD(src + u * WAVE);                 \
  }
#define MFG_ROWS_COMPUTE(BUF, c)                                    \
  _Pragma("unroll") for (int u = 0; u < U; ++u) {                   \
    if (MFG_ROWS_ABL_NOMATH) {                                      \
      acc[0] += (double)(BUF[u].x + BUF[u].y + BUF[u].z + BUF[u].w); \
      continue;                                                     \
    }                                                               \
    const double2 qq = q[((c) * U + u) * RPW + sub];                \
    const float pv[4] = {BUF[u].x, BUF[u].y, BUF[u].z, BUF[u].w};   \
    _Pragma("unroll") for (int k = 0; k < 4; ++k) {                 \
      const double p = (double)pv[k];                               \
      acc[k] = fma(p, qq.x, acc[k]);                                \
      if (KIND != MFG_REWARD_EXTERNAL && !MFG_ROWS_ABL_NOREW) {     \
        const double pp = p * p;                                    \
        s1[k] = fma(qq.x, pp, s1[k]);                               \
        if (KIND == MFG_REWARD_MFG_AC2) s2 = fma(qq.y, pp, s2);     \
      }                                                             \
    }                                                               \
  }
  // prologue: state of the first trajectory, its first chunk
  {
    const int64_t b0 = sup * KT;
#pragma unroll
    for (int m = 0; m < NQ; ++m) pnx[m] = pi[b0 * d + lane + m * WAVE];
    MFG_ROWS_ISSUE(va, b0, 0)
  }
  for (; sup < nsup; sup += nw) {
    const bool full = KT > 1 && (sup + 1) * KT <= B;  // every trajectory of the super tile exists: batched stores
#pragma unroll 1
    for (int kk = 0; kk < KT; ++kk) {
      const int64_t b = sup * KT + kk;
      if (b >= B) break;  // wave-uniform (last super tile only)
      // the wave's next trajectory (B = none: the very last chunk issue re-reads this trajectory's chunk 0)
      const int64_t bn = (kk + 1 < KT && b + 1 < B) ? b + 1 : ((sup + nw) * KT < B ? (sup + nw) * KT : B);
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int m = 0; m < NQ; ++m) {
        const double v = (double)pnx[m];
        q[lane + m * WAVE] = make_double2(v, v * v);
      }
      __builtin_amdgcn_s_waitcnt(0xc07f);
      __builtin_amdgcn_wave_barrier();
      if (bn < B) {
#pragma unroll
        for (int m = 0; m < NQ; ++m) pnx[m] = pi[bn * d + lane + m * WAVE];
      }
      double acc[4] = {0.0, 0.0, 0.0, 0.0}, s1[4] = {0.0, 0.0, 0.0, 0.0}, s2 = 0.0;
#pragma unroll 1
      for (int c = 0; c < CPT; c += 2) {
        MFG_ROWS_ISSUE(vb, b, c + 1)
        MFG_ROWS_COMPUTE(va, c)
        {
          // always issued (no phi over the register buffer): the chunk after the wave's very last one re-reads chunk 0
          const bool more = c + 2 < CPT;
          const int64_t nb = more ? b : (bn < B ? bn : b);
          const int nc = more ? c + 2 : 0;
          MFG_ROWS_ISSUE(va, nb, nc)
        }
        MFG_ROWS_COMPUTE(vb, c + 1)
      }
#pragma unroll
      for (int off = LPR; off < WAVE; off <<= 1) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          acc[k] += __shfl_xor(acc[k], off, WAVE);
          if (KIND != MFG_REWARD_EXTERNAL) s1[k] += __shfl_xor(s1[k], off, WAVE);
        }
      }
      if (sub == 0 && (!MFG_ROWS_ABL_NOSTORE || acc[0] == 123.456)) {
        const v4f_t ov = {(float)acc[0], (float)acc[1], (float)acc[2], (float)acc[3]};
        if (full) reinterpret_cast<v4f_t*>(wO + kk * d)[c4] = ov;
        else store16_device_scope(out_rsrc(pi_next + b * d), c4 * 16, ov);
      }
      if (KIND != MFG_REWARD_EXTERNAL) {
        double racc = 0.0;
        if (sub == 0) {
#pragma unroll
          for (int k = 0; k < 4; ++k) racc += (KIND == MFG_REWARD_MFG_AC2) ? q[4 * c4 + k].x * s1[k] : s1[k];
        }
        if (KIND == MFG_REWARD_MFG_AC2) racc -= s2;
        racc = wave_sum(racc);
        if (KIND == MFG_REWARD_SYNTHETIC) racc *= -0.5;
        if (lane == 0 && (!MFG_ROWS_ABL_NOSTORE || racc == 123.456)) {
          if (full) wR[kk] = (float)racc;
          else store4_device_scope(out_rsrc(reward + b), 0, (float)racc);
        }
      }
    }
    if (full) {
      __builtin_amdgcn_s_waitcnt(0xc07f);
      __builtin_amdgcn_wave_barrier();
      const __amdgpu_buffer_rsrc_t ob = out_rsrc(pi_next + sup * (int64_t)(KT * d));
      const v4f_t* s4 = reinterpret_cast<const v4f_t*>(wO);
#pragma unroll
      for (int k = lane; k < KT * d / 4; k += WAVE) store16_device_scope(ob, k * 16, s4[k]);
      if (KIND != MFG_REWARD_EXTERNAL && lane < KT / 4)
        store16_device_scope(out_rsrc(reward + sup * (int64_t)KT), lane * 16, reinterpret_cast<const v4f_t*>(wR)[lane]);
      __builtin_amdgcn_s_waitcnt(0xc07f);
      __builtin_amdgcn_wave_barrier();
    }
  }
#undef MFG_ROWS_ISSUE
#undef MFG_ROWS_COMPUTE
}

// ---------------------------------------------------------------------------------------------
// a3+a4, large d: one wavefront per trajectory; lane owns VEC consecutive columns in each of R
// 64*VEC-wide column chunks; rows stream from HBM with coalesced VEC*4-byte loads per lane.
// ---------------------------------------------------------------------------------------------
template <int VEC>
struct VecT;
template <>
struct VecT<1> {
  using type = float;
};
template <>
struct VecT<2> {
  using type = float2;
};
template <>
struct VecT<4> {
  using type = float4;
};

template <int VEC, int R, int KIND>
__global__ __launch_bounds__(BLOCK) void k_step_large(const float* __restrict__ pi, const float* __restrict__ P,
                                                      int64_t B, int d, float* __restrict__ pi_next,
                                                      float* __restrict__ reward) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  using V = typename VecT<VEC>::type;
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), wv = tid / WAVE;
  float* pis = smem + wv * d;
  const int64_t nw = (int64_t)gridDim.x * WAVES;
  for (int64_t b = (int64_t)blockIdx.x * WAVES + wv; b < B; b += nw) {
    for (int c = lane; c < d; c += WAVE) pis[c] = pi[b * d + c];
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): LDS writes of this wave landed
    double pc[R][VEC], acc[R][VEC], s1[R][VEC];
    int col[R];
#pragma unroll
    for (int m = 0; m < R; ++m) {
      col[m] = (m * WAVE + lane) * VEC;
#pragma unroll
      for (int v = 0; v < VEC; ++v) {
        pc[m][v] = (col[m] + v < d) ? (double)pis[col[m] + v] : 0.0;
        acc[m][v] = 0.0;
        s1[m][v] = 0.0;
      }
    }
    double s2 = 0.0;  // sum_i pi_i^2 sum_(own columns) p^2
    const float* Pb = P + b * (int64_t)d * d;
#pragma unroll 4
    for (int i = 0; i < d; ++i) {
      const double pii = (double)pis[i];
      const double pii2 = pii * pii;
      const float* row = Pb + (int64_t)i * d;
#pragma unroll
      for (int m = 0; m < R; ++m) {
        if (col[m] < d) {  // VEC divides d on the vector paths, so a chunk is fully in or out
          float pv[VEC];
          *reinterpret_cast<V*>(pv) = *reinterpret_cast<const V*>(row + col[m]);
#pragma unroll
          for (int v = 0; v < VEC; ++v) {
            const double p = (double)pv[v];
            acc[m][v] = fma(p, pii, acc[m][v]);
            if (KIND != MFG_REWARD_EXTERNAL) {
              const double pp = p * p;
              s1[m][v] = fma(pii, pp, s1[m][v]);
              if (KIND == MFG_REWARD_MFG_AC2) s2 = fma(pii2, pp, s2);
            }
          }
        }
      }
    }
#pragma unroll
    for (int m = 0; m < R; ++m) {
      if (col[m] < d) {
        float pv[VEC];
#pragma unroll
        for (int v = 0; v < VEC; ++v) pv[v] = (float)acc[m][v];
        *reinterpret_cast<V*>(pi_next + b * d + col[m]) = *reinterpret_cast<V*>(pv);
      }
    }
    if (KIND != MFG_REWARD_EXTERNAL) {
      double racc = 0.0;
#pragma unroll
      for (int m = 0; m < R; ++m)
#pragma unroll
        for (int v = 0; v < VEC; ++v) racc += (KIND == MFG_REWARD_MFG_AC2) ? pc[m][v] * s1[m][v] : s1[m][v];
      if (KIND == MFG_REWARD_MFG_AC2) racc -= s2;
      racc = wave_sum(racc);
      if (KIND == MFG_REWARD_SYNTHETIC) racc *= -0.5;
      if (lane == 0) reward[b] = (float)racc;
    }
    __builtin_amdgcn_wave_barrier();
  }
}

// ---------------------------------------------------------------------------------------------
// host side: the launch rule
// ---------------------------------------------------------------------------------------------
// developer knob (tools/step_probe.py): MFG_STEP_BATCH = 0 | 8 | 16 | 32 forces the tiles per super tile of the d = 21 / 15
// given-P kernel (0 = per-tile stores); unset / anything else = chosen from the batch size
static int step_batch_override() {
#ifdef MFG_DEV_KNOBS  // developer builds only (tools/variant.sh ... "-DMFG_DEV_KNOBS"): the shipped library reads no environment
  static const int v = [] {
    const char* e = getenv("MFG_STEP_BATCH");
    if (!e || !*e) return -1;
    const int k = atoi(e);
    return (k == 0 || k == 8 || k == 16 || k == 32) ? k : -1;
  }();
  return v;
#else
  return -1;
#endif
}

// The kernels take the reward kind at compile time: f(Int<KIND>{}) with KIND = reward_kind.  The other compile-time
// parameters of a launch travel the same way, as Int<..> / Flag<..> values.
template <int V>
using Int = std::integral_constant<int, V>;
template <bool V>
using Flag = std::integral_constant<bool, V>;
template <class F>
static void with_reward_kind(int reward_kind, F&& f) {
  switch (reward_kind) {
    case 0: f(Int<0>{}); break;
    case 1: f(Int<1>{}); break;
    default: f(Int<2>{}); break;
  }
}

namespace mfg {

int launch_step_given_P(const float* pi, const float* P, int64_t B, int d, int reward_kind, float* pi_next, float* reward,
                        hipStream_t st) {
  if (d <= WAVE) {
    const int G = WAVE / d, TB = WAVES * G;
    const size_t lds_pre = (size_t)TB * d * d * 4 + (size_t)((TB * d + 3) & ~3) * 4;   // prefetching kernel (fp32 pi)
    const size_t lds_una = (size_t)TB * d * d * 4 + (size_t)TB * d * 16;               // unaligned fallback (fp64 pi, pi^2)
    const size_t lds = (((uintptr_t)P & 15) == 0) ? lds_pre : lds_una;
    int bpc = (int)((160 * 1024) / (lds + 64));
    if (bpc > 8) bpc = 8;
    if (bpc < 1) bpc = 1;
    const int grid = grid_for(B, TB, bpc);
    const bool aligned = (((uintptr_t)P & 15) == 0);
    const int per = (int)(((int64_t)TB * d * d / 4 + BLOCK - 1) / BLOCK);  // 16-byte loads per thread per tile
    auto step_small = [&](auto dd, auto pp) {
      with_reward_kind(reward_kind, [&](auto k) {
        hipLaunchKernelGGL((k_step_small<decltype(k)::value, decltype(dd)::value, decltype(pp)::value>), dim3(grid), dim3(BLOCK),
                           lds, st, pi, P, B, d, pi_next, reward);
      });
    };
    if (!aligned) {
      with_reward_kind(reward_kind, [&](auto k) {
        hipLaunchKernelGGL((k_step_small_unaligned<decltype(k)::value>), dim3(grid), dim3(BLOCK), lds, st, pi, P, B, d, pi_next,
                           reward);
      });
    } else if (d == 21 || d == 15) {
#ifdef MFG_STEP_BLOCK_TILES
      if (d == 21) step_small(Int<21>{}, Int<6>{});
      else step_small(Int<15>{}, Int<4>{});
#else
      // The main launch covers B4 = B - B mod lcm(G, 4) trajectories (full tiles only and a whole number of 16-byte words
      // of P, so its prefetch needs no partial-tile / end-of-slab handling); the remaining < 12 trajectories go through
      // the ragged-capable instantiation.
      const int G = WAVE / d;
      const int64_t unit = (G % 4 == 0) ? G : (G % 2 == 0 ? 2 * G : 4 * G);
      const int64_t B4 = B - B % unit;
      auto step_wave = [&](auto dd, auto rag, int gw, const float* pi_, const float* P_, int64_t nb, float* pn_, float* rw_) {
        with_reward_kind(reward_kind, [&](auto k) {
          hipLaunchKernelGGL((k_step_wave<decltype(k)::value, decltype(dd)::value, decltype(rag)::value>), dim3(gw), dim3(BLOCK), 0,
                             st, pi_, P_, nb, pn_, rw_);
        });
      };
      if (B4 > 0) {
        // Large batches: consecutive-tile super tiles with batched device-scope stores (k_step_wave_batched), as soon as
        // every one of the 8 waves per CU gets >= 2 super tiles; KB = tiles per super tile, the largest that qualifies.
        const int64_t ntiles = (B4 + G - 1) / G;
        const int64_t nw_target = (int64_t)num_cus() * 2 * WAVES;
        int kb = 0;
        for (int cand : {32, 16, 8}) {  // >= 2 super tiles per wave, and the last round >= 90 % full
          const int64_t ns = (ntiles + cand - 1) / cand, rr = (ns + nw_target - 1) / nw_target;
          if (!kb && rr >= 2 && 10 * ns >= 9 * rr * nw_target) kb = cand;
        }
        const int forced = step_batch_override();  // developer knob: MFG_STEP_BATCH = 0 (never) | 8 | 16 | 32
        if (forced >= 0) kb = forced;
        const bool out16 = (((uintptr_t)pi_next & 15) == 0) && (((uintptr_t)reward & 15) == 0);
        if (kb && out16) {
          const int64_t nsuper = (ntiles + kb - 1) / kb;
          const int64_t rounds = (nsuper + nw_target - 1) / nw_target;
          const int64_t nwv = (nsuper + rounds - 1) / rounds;
          const int gb = (int)((nwv + WAVES - 1) / WAVES);
          auto step_wave_batched = [&](auto dd, auto kbt) {
            with_reward_kind(reward_kind, [&](auto k) {
              hipLaunchKernelGGL((k_step_wave_batched<decltype(k)::value, decltype(dd)::value, decltype(kbt)::value>), dim3(gb),
                                 dim3(BLOCK), 0, st, pi, P, B4, pi_next, reward);
            });
          };
          auto by_kb = [&](auto dd) {
            if (kb == 32) step_wave_batched(dd, Int<32>{});
            else if (kb == 16) step_wave_batched(dd, Int<16>{});
            else step_wave_batched(dd, Int<8>{});
          };
          if (d == 21) by_kb(Int<21>{});
          else by_kb(Int<15>{});
        } else {
          const int gw = grid_for(B4, G * WAVES, MFG_STEP_WAVES);
          if (d == 21) step_wave(Int<21>{}, Flag<false>{}, gw, pi, P, B4, pi_next, reward);
          else step_wave(Int<15>{}, Flag<false>{}, gw, pi, P, B4, pi_next, reward);
        }
      }
      if (B > B4) {
        const float* pi_t = pi + B4 * d;
        const float* P_t = P + B4 * d * d;   // 16-byte aligned: B4 is a multiple of 4
        float* pn_t = pi_next + B4 * d;
        float* rw_t = reward ? reward + B4 : nullptr;
        const int64_t Bt = B - B4;
        if (d == 21) step_wave(Int<21>{}, Flag<true>{}, 1, pi_t, P_t, Bt, pn_t, rw_t);
        else step_wave(Int<15>{}, Flag<true>{}, 1, pi_t, P_t, Bt, pn_t, rw_t);
      }
#endif
    }
    else if (per <= 4) step_small(Int<0>{}, Int<4>{});
    else if (per <= 8) step_small(Int<0>{}, Int<8>{});
    else step_small(Int<0>{}, Int<16>{});
  } else {
    const size_t lds = (size_t)WAVES * d * 4;
    const int grid = grid_for(B, WAVES, (d == 128 || d == 256) ? MFG_ROWS_BPC : 8);
    const bool a16 = (((uintptr_t)P & 15) == 0) && (((uintptr_t)pi_next & 15) == 0);
    int vec = 1;
    if (a16 && d % 4 == 0) vec = 4;
    else if (a16 && d % 2 == 0) vec = 2;
    // keep at most 2 chunks per lane on the vector paths, fall back to narrower vectors otherwise
    int R = (d + WAVE * vec - 1) / (WAVE * vec);
    if (a16 && (d == 128 || d == 256)) {
      auto step_rows = [&](auto lpr, auto ktt, int gr) {
        with_reward_kind(reward_kind, [&](auto k) {
          hipLaunchKernelGGL((k_step_rows<decltype(k)::value, decltype(lpr)::value, decltype(ktt)::value>), dim3(gr), dim3(BLOCK), 0,
                             st, pi, P, B, pi_next, reward);
        });
      };
      // super tiles of MFG_ROWS_KT consecutive trajectories (batched output bursts) once every resident wave gets one
      const bool out16 = (((uintptr_t)pi_next & 15) == 0) && (((uintptr_t)reward & 15) == 0);
      const int64_t nw_target = (int64_t)num_cus() * MFG_ROWS_BPC * WAVES;
      // ... and the last round is >= 90 % full (a half-empty round of 8-trajectory units costs more than the bursts save:
      // 20 000 trajectories ran at 0.70 of peak as 2 500 super tiles over two rounds, 0.78 one trajectory at a time)
      int kt = 1;
      if (out16) {
        const int64_t ns8 = (B + MFG_ROWS_KT - 1) / MFG_ROWS_KT, rr8 = (ns8 + nw_target - 1) / nw_target;
        if (ns8 >= nw_target && 10 * ns8 >= 9 * rr8 * nw_target) kt = MFG_ROWS_KT;
      }
      const int64_t nsup = (B + kt - 1) / kt;
      const int64_t rounds = (nsup + nw_target - 1) / nw_target;
      const int gr = (int)(((nsup + rounds - 1) / rounds + WAVES - 1) / WAVES);
      if (d == 128) {
        if (kt > 1) step_rows(Int<32>{}, Int<MFG_ROWS_KT>{}, gr);
        else step_rows(Int<32>{}, Int<1>{}, gr);
      } else {
        if (kt > 1) step_rows(Int<64>{}, Int<MFG_ROWS_KT>{}, gr);
        else step_rows(Int<64>{}, Int<1>{}, gr);
      }
      return check_launch("step_given_P");
    }
    auto step_large = [&](auto vv, auto rr) {
      with_reward_kind(reward_kind, [&](auto k) {
        hipLaunchKernelGGL((k_step_large<decltype(vv)::value, decltype(rr)::value, decltype(k)::value>), dim3(grid), dim3(BLOCK), lds,
                           st, pi, P, B, d, pi_next, reward);
      });
    };
    if (vec == 4 && R == 1) step_large(Int<4>{}, Int<1>{});
    else if (vec == 4 && R == 2) step_large(Int<4>{}, Int<2>{});
    else if (vec == 2 && R == 1) step_large(Int<2>{}, Int<1>{});
    else if (vec == 2 && R == 2) step_large(Int<2>{}, Int<2>{});
    else if (vec == 2 && R == 3) step_large(Int<2>{}, Int<3>{});
    else if (vec == 2 && R == 4) step_large(Int<2>{}, Int<4>{});
    else {
      R = (d + WAVE - 1) / WAVE;
      switch (R) {
        case 2: step_large(Int<1>{}, Int<2>{}); break;
        case 3: step_large(Int<1>{}, Int<3>{}); break;
        case 4: step_large(Int<1>{}, Int<4>{}); break;
        case 5: step_large(Int<1>{}, Int<5>{}); break;
        case 6: step_large(Int<1>{}, Int<6>{}); break;
        case 7: step_large(Int<1>{}, Int<7>{}); break;
        case 8: step_large(Int<1>{}, Int<8>{}); break;
        default: return fail(MFG_EUNSUPPORTED, "%s: d=%lld > %lld", "step", (long long)d, (long long)MFG_MAX_D);
      }
    }
  }
  return check_launch("step_given_P");
}

}  // namespace mfg
