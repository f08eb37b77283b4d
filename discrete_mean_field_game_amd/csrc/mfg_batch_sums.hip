// Batch sums of the actor-critic update (a6 / a8) and the critic values of a whole rollout, for MI355X (gfx950 / CDNA4,
// wave64): the two GEMM-shaped pieces of the path, on the fp64 matrix cores.  They share the workspace of a call
// (mfg_batch_sums.h).  Here: the non-template kernels around the bodies of mfg_grad.h (which the population units run too),
// k_grad_mfma2, k_value_mfma / k_value_mfma2 / k_td_delta, and the launch rules launch_grad and launch_values_and_delta.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "../../include/mfg_hip.h"
#include "mfg_batch_sums.h"
#include "mfg_core.h"
#include "mfg_grad.h"
#include "mfg_host.h"
#include "mfg_population.h"

using namespace mfg;

__global__ __launch_bounds__(BLOCK) void k_grad_partial(GradArgs a) { grad_partial_body(a); }

__global__ void k_add_reward(double* __restrict__ delta, const float* __restrict__ reward, int64_t N) {
  for (int64_t n = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; n < N; n += (int64_t)gridDim.x * blockDim.x)
    delta[n] += (double)reward[n];
}

__global__ __launch_bounds__(RP_SLICES* RP_OUT) void k_reduce_partials(const double* __restrict__ partial, int64_t nsb, int64_t FO,
                                                                      int accumulate, double* __restrict__ G, ReduceApply ap) { reduce_partials_body(partial, nsb, FO, accumulate, G, ap); }

// ---------------------------------------------------------------------------------------------
// Round 3: register-blocked form of k_grad_mfma for d = 128 / 256 (C3, C5).  k_grad_mfma gives a wave an arbitrary run of
// tiles, fetches BOTH operands of every matrix instruction from LDS and tests `i < nmine` (a scalar branch, i.e. a basic
// block boundary) in front of each: nothing overlaps, 190-220 cycles per instruction against the ~70 the matrix core needs,
// whatever the tile count per wave or the number of sample slices (variants measured: no better).  Here a wave owns
// RECTANGLES of tiles given at compile time as (rows NA, columns NB, tile mask) -- one K step of 4 samples fetches NA + NB
// operands for up to NA NB instructions, no branch in the K loop, and the fetches of a step issue under the matrix
// instructions of the step before.  The upper triangle is cut so that EVERY wave has the same number of tiles (the
// instruction stream of a SIMD is the bound; 64 x 64 "super tiles" s = 0 .. d/64-1 on the diagonal, (r, c) off it):
//   d = 256, 136 tiles = 8 waves x 17 (grid.y = 2 blocks of 4 waves):
//     y = 0: (0,1) + one tile of diagonal 1 | (0,2) + one | (0,3) + one | diagonal 0 (10 tiles) + the first two rows of diagonal 1 (7)
//     y = 1: (1,2) + one tile of diagonal 3 | (1,3) + one | (2,3) + one | diagonal 2 + the first two rows of diagonal 3
//   d = 128, 36 tiles = 4 waves x 9: half of (0,1) (2 x 4 tiles) + tile (3,3) of a diagonal | ... | diagonal 0 less (3,3) | diagonal 1 less (3,3)
// Staging, split-K over grid.x, partial rows, side sums and the row reduction are those of k_grad_mfma.
// ---------------------------------------------------------------------------------------------
constexpr unsigned GM2_RECT44 = 0xFFFFu, GM2_DIAG44 = 0x8CEFu, GM2_DIAG44M = 0x0CEFu, GM2_TRAP24 = 0xEFu, GM2_RECT24 = 0xFFu,
                   GM2_ONE = 1u;
__host__ __device__ constexpr int gm2_count(unsigned m) { return m == 0 ? 0 : (int)(m & 1u) + gm2_count(m >> 1); }

// one rectangle over one staged chunk
template <int D, int NA, int NB, unsigned MASK>
__device__ __forceinline__ void gm2_step(const float* __restrict__ abase, const float* __restrict__ bbase, int off, double dk,
                                         v4d_t* acc) {
  double av[NA], bv[NB];
#pragma unroll
  for (int i = 0; i < NA; ++i) av[i] = dk * (double)abase[off + (i << 4)];  // A[row li][k] = delta_k pi_k[16 (ra + i) + li]
#pragma unroll
  for (int j = 0; j < NB; ++j) bv[j] = (double)bbase[off + (j << 4)];       // B[k][col li] = pi_k[16 (cb + j) + li]
  int t = 0;
#pragma unroll
  for (int i = 0; i < NA; ++i) {
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      if ((MASK >> (i * NB + j)) & 1u) {
        acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[i], bv[j], acc[t], 0, 0, 0);
        ++t;
      }
    }
  }
}
template <int D, int NA0, int NB0, unsigned M0, int NA1, int NB1, unsigned M1>
__device__ __forceinline__ void gm2_chunk(const float* __restrict__ sp, const double* __restrict__ dl, int lk, int li,
                                          const int* ra, const int* cb, v4d_t* acc) {
  constexpr int pitch = D + 16;
  const float* lb = sp + lk * pitch + li;
  const float *a0 = lb + (ra[0] << 4), *b0 = lb + (cb[0] << 4), *a1 = lb + (ra[1] << 4), *b1 = lb + (cb[1] << 4);
#pragma unroll 2
  for (int ks = 0; ks < GM_KC / 4; ++ks) {  // (fully unrolled the compiler hoists all 8 steps' operands: 444 spilled registers)
    const double dk = dl[ks * 4 + lk];
    gm2_step<D, NA0, NB0, M0>(a0, b0, ks * 4 * pitch, dk, acc);
    if constexpr (M1 != 0) gm2_step<D, NA1, NB1, M1>(a1, b1, ks * 4 * pitch, dk, acc + gm2_count(M0));
  }
}
template <int D, int NA, int NB, unsigned MASK>
__device__ __forceinline__ void gm2_store(double* __restrict__ out, int lk, int li, int ra, int cb, const v4d_t* acc) {
  int t = 0;
#pragma unroll
  for (int i = 0; i < NA; ++i) {
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      if ((MASK >> (i * NB + j)) & 1u) {
#pragma unroll
        for (int v = 0; v < 4; ++v) {  // D[i][j] of a tile: lane holds rows 4 v + lane / 16, column lane % 16
          const int gi = ((ra + i) << 4) + 4 * v + lk, gj = ((cb + j) << 4) + li;
          if (gi <= gj) out[feat_idx(gi, gj, D)] = acc[t][v];
        }
        ++t;
      }
    }
  }
}

template <int D>
struct Gm2Geom {
  static constexpr int NY = D == 256 ? 2 : 1, ACCN = D == 256 ? 17 : 9;
};
template <int NA_, int NB_, unsigned MASK_>
struct Gm2Rect {
  static constexpr int NA = NA_, NB = NB_;
  static constexpr unsigned MASK = MASK_;
};
template <int D>
__global__ __launch_bounds__(BLOCK, 2) void k_grad_mfma2(GradArgs a) {
  static_assert(D == 128 || D == 256, "tile maps exist for d = 128 and 256");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  constexpr int d = D, pitch = D + 16;
  constexpr int Q = d * (d + 1) / 2, F = Q + d + 1, FO = F + 3;
  constexpr int ACCN = Gm2Geom<D>::ACCN;
  double* dl = reinterpret_cast<double*>(smem_raw);       // [KC] delta
  double* red = dl + GM_KC;                               // [4][BLOCK] scalar reduction scratch
  float* sp = reinterpret_cast<float*>(red + 4 * BLOCK);  // [KC][pitch] pi rows
  const int tid = threadIdx.x, lane = tid & (WAVE - 1);
  const int wv = __builtin_amdgcn_readfirstlane(tid / WAVE), y = (int)blockIdx.y;
  // this wave's two rectangles (tile coordinates of their corners); the last wave of a block owns the diagonal pieces
  const bool diag = D == 256 ? wv == 3 : wv >= 2;
  int ra[2] = {0, 0}, cb[2] = {0, 0};
  if (D == 256) {
    const int sd = 2 * y;  // this block's diagonal super tiles: sd (whole), sd + 1 (split)
    if (diag) {
      ra[0] = cb[0] = 4 * sd;
      ra[1] = cb[1] = 4 * sd + 4;
    } else {
      const int sr = y == 0 ? 0 : (wv == 2 ? 2 : 1), sc = y == 0 ? wv + 1 : (wv == 0 ? 2 : 3);
      ra[0] = 4 * sr;
      cb[0] = 4 * sc;
      ra[1] = 4 * sd + 4 + (wv == 2 ? 3 : 2);  // tiles (2,2) (2,3) (3,3) of super tile sd + 1
      cb[1] = 4 * sd + 4 + (wv == 0 ? 2 : 3);
    }
  } else {
    if (diag) ra[0] = cb[0] = 4 * (wv - 2);
    else {
      ra[0] = 2 * wv;
      cb[0] = 4;
      ra[1] = cb[1] = 4 * wv + 3;  // tile (3,3) of diagonal super tile wv
    }
  }
  const bool side = blockIdx.y == 0;  // also owns the linear and scalar sums
  double lin = 0.0, s_d = 0.0, s_dg = 0.0, s_r = 0.0, s_n = 0.0;  // (d <= BLOCK: one linear column per thread)
  const int li = lane & 15, lk = lane >> 4;
  const double invT = 1.0 / (double)a.T;
  // register prefetch of a chunk: thread -> (row q0 + rpp u, float4 column c4)
  constexpr int dq = d >> 2, rpp = BLOCK / dq, NPF = GM_KC / rpp;
  static_assert(BLOCK % dq == 0 && GM_KC % rpp == 0, "whole rows per staging pass");
  const int q0 = tid / dq, c4 = tid - q0 * dq;
  double* out = a.partial + (int64_t)blockIdx.x * FO;
  // The whole sample loop is instantiated once per ROLE and the role is chosen outside it: with the role test inside the
  // loop the two instantiations' accumulators are merged at every iteration (two full sets live: 254 spilled registers
  // at d = 256).  Both instantiations execute the same barriers.
  auto run = [&](auto r0, auto r1) __attribute__((always_inline)) {
    using R0 = decltype(r0);
    using R1 = decltype(r1);
    v4d_t acc[ACCN];
#pragma unroll
    for (int i = 0; i < ACCN; ++i) acc[i] = (v4d_t)(0.0);
    float4 pf[NPF];
    double pf_de = 0.0, pf_dg = 0.0, pf_rr = 0.0;
    bool pf_on = false;
    auto fetch = [&](int64_t n0_) __attribute__((always_inline)) {
      const int cn_ = (int)((a.N - n0_) < GM_KC ? (a.N - n0_) : GM_KC);
#pragma unroll
      for (int u = 0; u < NPF; ++u) {
        const int q = q0 + u * rpp;
        pf[u] = make_float4(0.f, 0.f, 0.f, 0.f);  // rows past the end are zero: they add nothing
        if (q < cn_) {
          const int64_t n = n0_ + q;
          const int64_t b = (int64_t)(((double)n + 0.5) * invT);
          pf[u] = *reinterpret_cast<const float4*>(a.pi + b * a.stride_b + (n - b * a.T) * d + 4 * c4);
        }
      }
      pf_de = 0.0, pf_dg = 0.0, pf_rr = 0.0, pf_on = false;
      if (tid < cn_) {
        const int64_t n = n0_ + tid;
        pf_de = a.delta[n];
        pf_rr = a.reward ? (double)a.reward[n] : 0.0;
        if (a.g) pf_dg = a.g[n];
        pf_on = true;
      }
    };
    if ((int64_t)blockIdx.x * GM_KC < a.N) fetch((int64_t)blockIdx.x * GM_KC);
    for (int64_t n0 = (int64_t)blockIdx.x * GM_KC; n0 < a.N; n0 += (int64_t)gridDim.x * GM_KC) {
      __syncthreads();
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
      if (nn < a.N) fetch(nn);
      gm2_chunk<D, R0::NA, R0::NB, R0::MASK, R1::NA, R1::NB, R1::MASK>(sp, dl, lk, li, ra, cb, acc);
      if (side && tid < d) {
        double t = lin;
#pragma unroll 8
        for (int q = 0; q < GM_KC; ++q) t = fma(dl[q], (double)sp[q * pitch + tid], t);
        lin = t;
      }
    }
    gm2_store<D, R0::NA, R0::NB, R0::MASK>(out, lk, li, ra[0], cb[0], acc);
    if constexpr (R1::MASK != 0) gm2_store<D, R1::NA, R1::NB, R1::MASK>(out, lk, li, ra[1], cb[1], acc + gm2_count(R0::MASK));
  };
  if (D == 256) {
    if (diag) run(Gm2Rect<4, 4, GM2_DIAG44>{}, Gm2Rect<2, 4, GM2_TRAP24>{});
    else run(Gm2Rect<4, 4, GM2_RECT44>{}, Gm2Rect<1, 1, GM2_ONE>{});
  } else {
    if (diag) run(Gm2Rect<4, 4, GM2_DIAG44M>{}, Gm2Rect<1, 1, 0u>{});
    else run(Gm2Rect<2, 4, GM2_RECT24>{}, Gm2Rect<1, 1, GM2_ONE>{});
  }
  if (side) {
    if (tid < d) out[Q + tid] = lin;
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

// ---------------------------------------------------------------------------------------------
// Critic values of a whole rollout on the fp64 matrix cores (d a multiple of 16, 64 <= d <= 512): the second GEMM-shaped
// piece of the path.  V_n = x_n^T U x_n + b.x_n + c for the N = B (T+1) states a rollout left in pi_traj, i.e. the
// diagonal of X U X^T: a wave owns 16 states (A operand: X[16 x 4] slices from its LDS copy of the rows), sweeps the
// column tiles of the upper triangle U (B operand straight from the L2-resident weight vector, row k of U is contiguous in
// c), and folds each finished 16 x 16 tile Y = X U into  v_n += sum_c (Y_nc + b_c) x_nc.  The 16 lanes that hold one state
// are one DPP row, so the final sum is four DPP steps.  Inside the wave-per-trajectory rollout kernel the same values
// cost a latency-bound triangular loop per state (10 % of the d = 128 training rollout); here they are ~2 nt (nt + 1)
// matrix instructions per 16 states.  Followed by k_td_delta (delta = r + gamma V' - V).
// ---------------------------------------------------------------------------------------------
// Round 2b: the B operand comes from LDS.  Before, every lane fetched its U element from the L2-resident weight vector
// with 64-bit index arithmetic and a select in front of every matrix instruction (~15 VALU + 1 dependent L2 load per
// MFMA, the whole of U re-read by every wave for its 16 states): 3-6x the matrix-core time.  Now the block's four waves
// (64 states) share each 64-row x 16-column piece of U: it is fetched once per block (zero-filled below the diagonal),
// double-buffered in LDS -- the loads of piece n+1 are issued before the matrix instructions of piece n and committed
// after them -- and a matrix instruction costs two LDS reads and a convert.
constexpr int VM_CH = 64;  // rows of U per staged piece
__global__ __launch_bounds__(BLOCK) void k_value_mfma(const float* __restrict__ pi, int64_t stride_b, int64_t N, int TP1, int d,
                                                      const double* __restrict__ w, double* __restrict__ V) {
  extern __shared__ __attribute__((aligned(16))) float smx[];
  const int tid = threadIdx.x, lane = tid & (WAVE - 1);
  const int wv = __builtin_amdgcn_readfirstlane(tid / WAVE);
  const int li = lane & 15, lk = lane >> 4;
  const int nt = d >> 4, pitch = d + 4;  // +4 floats: the 16 state rows of an A operand fall on distinct banks
  const int Q = d * (d + 1) / 2;
  float* xs = smx + (size_t)wv * 16 * pitch;
  double* Bs = reinterpret_cast<double*>(smx + (size_t)WAVES * 16 * pitch);  // [2][VM_CH][16]
  const double invT = 1.0 / (double)TP1;
  const int64_t ngroups = (N + 15) / 16;
  const int64_t npass = (ngroups + WAVES - 1) / WAVES;
  // staging role of this thread: column sc of the tile, rows sr, sr + 16, sr + 32, sr + 48 of the piece
  const int sc = tid & 15, sr = tid >> 4;
  double stg[4];
#define MFG_VM_LOAD(jt_, ch_)                                                              \
  _Pragma("unroll") for (int q = 0; q < 4; ++q) {                                          \
    const int k = VM_CH * (ch_) + sr + 16 * q, c = 16 * (jt_) + sc;                        \
    stg[q] = (k <= c) ? w[k * d - (k * (k - 1)) / 2 + (c - k)] : 0.0;                      \
  }
#define MFG_VM_COMMIT(buf_)                                                                \
  _Pragma("unroll") for (int q = 0; q < 4; ++q) Bs[((buf_) * VM_CH + sr + 16 * q) * 16 + sc] = stg[q];
  for (int64_t pass = blockIdx.x; pass < npass; pass += gridDim.x) {
    const int64_t n0 = (pass * WAVES + wv) * 16;
    __syncthreads();  // the previous pass is done with Bs
    // stage the 16 state rows (fp32, float4 copies: d is a multiple of 16 and rows are 16-byte aligned when stride_b % 4 == 0)
    for (int e = lane; e < 16 * (d >> 2); e += WAVE) {
      const int q = e / (d >> 2), c4 = e - q * (d >> 2);
      const int64_t n = n0 + q;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (n < N) {
        const int64_t b = (int64_t)(((double)n + 0.5) * invT);
        v = *reinterpret_cast<const float4*>(pi + b * stride_b + (n - b * TP1) * (int64_t)d + 4 * c4);
      }
      *reinterpret_cast<float4*>(xs + q * pitch + 4 * c4) = v;
    }
    MFG_VM_LOAD(0, 0)
    MFG_VM_COMMIT(0)
    __syncthreads();
    int buf = 0;
    double vs[4] = {0.0, 0.0, 0.0, 0.0};
    for (int jt = 0; jt < nt; ++jt) {
      const int c = (jt << 4) + li;  // this lane's column of the tile
      v4d_t acc = (v4d_t)(0.0);
      const int nch = (16 * (jt + 1) + VM_CH - 1) / VM_CH;
      for (int ch = 0; ch < nch; ++ch) {
        // the next piece of the sweep: issue its loads now, commit them after this piece's matrix instructions
        const bool last_ch = ch + 1 == nch;
        const bool has_next = !last_ch || jt + 1 < nt;
        const int njt = last_ch ? jt + 1 : jt, nc = last_ch ? 0 : ch + 1;
        if (has_next) MFG_VM_LOAD(njt, nc)
        int ksteps = 4 * (jt + 1) - (VM_CH / 4) * ch;  // rows 0 .. 16 jt + 15 of U, four at a time
        if (ksteps > VM_CH / 4) ksteps = VM_CH / 4;
        const float* xa = xs + li * pitch + VM_CH * ch + lk;
        const double* bb = Bs + (buf * VM_CH + lk) * 16 + li;
#pragma unroll 4
        for (int ks = 0; ks < ksteps; ++ks)
          acc = __builtin_amdgcn_mfma_f64_16x16x4f64((double)xa[4 * ks], bb[64 * ks], acc, 0, 0, 0);  // A[i = li][k], B[k][j = li]
        if (has_next) MFG_VM_COMMIT(buf ^ 1)
        __syncthreads();
        buf ^= 1;
      }
      const double bc = w[Q + c];
#pragma unroll
      for (int v = 0; v < 4; ++v) vs[v] = fma(acc[v] + bc, (double)xs[(4 * v + lk) * pitch + c], vs[v]);  // D[i = 4v + lk][j = li]
    }
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      double t = vs[v];
      t += dpp_mov_f64<0xB1, 0xF>(t);
      t += dpp_mov_f64<0x4E, 0xF>(t);
      t += dpp_mov_f64<0x141, 0xF>(t);
      t += dpp_mov_f64<0x140, 0xF>(t);
      const int64_t n = n0 + 4 * v + lk;
      if (li == 0 && n < N) V[n] = t + w[Q + d];
    }
  }
#undef MFG_VM_LOAD
#undef MFG_VM_COMMIT
}

// ---------------------------------------------------------------------------------------------
// Round 3: GEMM-tiled form of k_value_mfma for d a multiple of 64 (C3, C5).  k_value_mfma keeps the FULL rows of a wave's
// 16 states in LDS (66 KB per block at d = 256: one block per CU, one wave per SIMD), one accumulator tile per wave (every
// matrix instruction waits for the one before) and a block barrier every 16 instructions: 226 cycles per instruction
// against ~70.  Here a block owns 128 states and walks the upper triangle of U in 64 x 64 pieces (column block cb, row
// chunk kc <= cb): a piece of U (fp64, zero below the diagonal) and the matching 128 x 64 slab of states (fp32) are staged
// -- fetched into registers under the previous piece's matrix instructions, committed behind them -- and a wave runs
// 2 state groups x 4 column tiles = 8 independent accumulators over the 16 K steps of the piece: 2 + 4 operand reads
// for 8 matrix instructions, 128 instructions between barriers, two blocks per CU.  After a column block's last piece the
// finished tiles Y = X U are folded into  v_n += sum_c (Y_nc + b_c) x_nc  (x: 32 LDS reads per lane per 64
// columns, read back from the slab of the diagonal piece).  The all-zero tiles of a diagonal piece are skipped.
// ---------------------------------------------------------------------------------------------
constexpr int VM2_MB = 128, VM2_KC = 64, VM2_XP = VM2_KC + 2;  // states per block, rows per piece, pitch of the state slab
                                                               // (2 mod 32: the 32 lanes of a half wave hit 32 banks)
__global__ __launch_bounds__(BLOCK, 2) void k_value_mfma2(const float* __restrict__ pi, int64_t stride_b, int64_t N, int TP1, int d,
                                                           const double* __restrict__ w, double* __restrict__ V) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  double* Us = reinterpret_cast<double*>(smem_raw);                   // [KC][64]
  float* Xs = reinterpret_cast<float*>(Us + VM2_KC * 64);             // [MB][XP]
  const int tid = threadIdx.x, lane = tid & (WAVE - 1);
  const int wv = __builtin_amdgcn_readfirstlane(tid / WAVE);
  const int li = lane & 15, lk = lane >> 4;
  const int ncb = d >> 6, Q = d * (d + 1) / 2;
  const double invT = 1.0 / (double)TP1;
  const int64_t npass = (N + VM2_MB - 1) / VM2_MB;
  // staging roles.  U piece: thread -> row ur = tid / 4, sixteen columns from uc = 16 (tid % 4) (the row of U is contiguous in
  // the packed weight vector); state slab: thread -> state xr + 16 u (u < 8), float4 column xc.
  const int ur = tid >> 2, uc = (tid & 3) << 4;
  const int xr = tid >> 4, xc = (tid & 15) << 2;
  double ustg[16];
  float4 xstg[8];
  for (int64_t pass = blockIdx.x; pass < npass; pass += gridDim.x) {
    const int64_t n0 = pass * VM2_MB;
    // row pointers of this thread's staged states (clamped; rows past N are never written out)
    const float* xrow[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      int64_t n = n0 + xr + 16 * u;
      if (n >= N) n = N - 1;
      const int64_t b = (int64_t)(((double)n + 0.5) * invT);
      xrow[u] = pi + b * stride_b + (n - b * TP1) * (int64_t)d;
    }
    auto fetch = [&](int cbk, int kc) __attribute__((always_inline)) {
      const int k = VM2_KC * kc + ur, c0 = 64 * cbk + uc;
      const double* wr = w + ((int64_t)k * d - ((int64_t)k * (k - 1)) / 2 - k);  // U[k][c] = wr[c] for c >= k
#pragma unroll
      for (int q = 0; q < 16; ++q) ustg[q] = (c0 + q >= k) ? wr[c0 + q] : 0.0;
#pragma unroll
      for (int u = 0; u < 8; ++u) xstg[u] = *reinterpret_cast<const float4*>(xrow[u] + VM2_KC * kc + xc);
    };
    auto commit = [&]() __attribute__((always_inline)) {
#pragma unroll
      for (int q = 0; q < 16; q += 2) *reinterpret_cast<double2*>(Us + ur * 64 + uc + q) = make_double2(ustg[q], ustg[q + 1]);
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        float* dst = Xs + (xr + 16 * u) * VM2_XP + xc;  // (pitch 66: 8-byte aligned only)
        *reinterpret_cast<float2*>(dst) = make_float2(xstg[u].x, xstg[u].y);
        *reinterpret_cast<float2*>(dst + 2) = make_float2(xstg[u].z, xstg[u].w);
      }
    };
    double vs[2][4] = {{0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}};
    fetch(0, 0);
    for (int cbk = 0; cbk < ncb; ++cbk) {
      v4d_t acc[2][4];
#pragma unroll
      for (int sg = 0; sg < 2; ++sg)
#pragma unroll
        for (int cg = 0; cg < 4; ++cg) acc[sg][cg] = (v4d_t)(0.0);
      for (int kc = 0; kc <= cbk; ++kc) {
        __syncthreads();  // the previous piece's matrix instructions are done with Us / Xs
        commit();
        __syncthreads();
        // the next piece of the sweep (its loads land under this piece's matrix instructions)
        const bool last_kc = kc == cbk;
        if (!last_kc || cbk + 1 < ncb) fetch(last_kc ? cbk + 1 : cbk, last_kc ? 0 : kc + 1);
        const float* xa = Xs + (wv * 32 + li) * VM2_XP + lk;
        const double* ub = Us + lk * 64 + li;
        if (!last_kc) {
#pragma unroll 2
          for (int ks = 0; ks < VM2_KC / 4; ++ks) {
            const double a0 = (double)xa[4 * ks], a1 = (double)xa[16 * VM2_XP + 4 * ks];  // A[state li][k]
#pragma unroll
            for (int cg = 0; cg < 4; ++cg) {
              const double bv = ub[4 * ks * 64 + 16 * cg];  // B[k][col li]
              acc[0][cg] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, bv, acc[0][cg], 0, 0, 0);
              acc[1][cg] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, bv, acc[1][cg], 0, 0, 0);
            }
          }
        } else {
          // the piece on the diagonal: rows 16 p .. 16 p + 15 of it are zero left of column tile p -- skip those tiles
#pragma unroll
          for (int pq = 0; pq < 4; ++pq) {
#pragma unroll 2
            for (int ks = 4 * pq; ks < 4 * pq + 4; ++ks) {
              const double a0 = (double)xa[4 * ks], a1 = (double)xa[16 * VM2_XP + 4 * ks];
#pragma unroll
              for (int cg = pq; cg < 4; ++cg) {
                const double bv = ub[4 * ks * 64 + 16 * cg];
                acc[0][cg] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, bv, acc[0][cg], 0, 0, 0);
                acc[1][cg] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, bv, acc[1][cg], 0, 0, 0);
              }
            }
          }
        }
      }
      // fold the finished 32 x 64 block of Y: D[i = 4 v + lk][j = li] of tile (sg, cg).  The state slab of the diagonal
      // piece (still in LDS: the next commit waits behind the barrier) holds exactly the columns of this block.
#pragma unroll
      for (int cg = 0; cg < 4; ++cg) {
        const double bc = w[Q + 64 * cbk + 16 * cg + li];
#pragma unroll
        for (int sg = 0; sg < 2; ++sg) {
#pragma unroll
          for (int v = 0; v < 4; ++v) {
            const double x = (double)Xs[(wv * 32 + sg * 16 + 4 * v + lk) * VM2_XP + 16 * cg + li];
            vs[sg][v] = fma(acc[sg][cg][v] + bc, x, vs[sg][v]);
          }
        }
      }
    }
#pragma unroll
    for (int sg = 0; sg < 2; ++sg) {
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        double t = vs[sg][v];
        t += dpp_mov_f64<0xB1, 0xF>(t);
        t += dpp_mov_f64<0x4E, 0xF>(t);
        t += dpp_mov_f64<0x141, 0xF>(t);
        t += dpp_mov_f64<0x140, 0xF>(t);
        const int64_t n = n0 + wv * 32 + sg * 16 + 4 * v + lk;
        if (li == 0 && n < N) V[n] = t + w[Q + d];
      }
    }
  }
}

// delta[b, s] = r[b, s] + gd(s) V[b, s+1] - V[b, s],  gd = gamma (mfg_ac2.py:505) or the running gamma^s (ac_irl.py:691);
// reward == NULL: the IRL form without the reward (added by the gradient kernel once the network has run).
__global__ void k_td_delta(const double* __restrict__ V, const float* __restrict__ reward, int64_t B, int T, double gamma,
                           int discount_pow, double* __restrict__ delta) {
  const int64_t n_tot = B * T;
  for (int64_t n = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; n < n_tot; n += (int64_t)gridDim.x * blockDim.x) {
    const int64_t b = n / T;
    const int s = (int)(n - b * T);
    double gd = gamma;
    if (discount_pow) {
      gd = 1.0;
      for (int q = 0; q < s; ++q) gd *= gamma;  // the running product of the in-kernel form, same rounding
    }
    const double r = reward ? (double)reward[n] : 0.0;
    delta[n] = r + gd * V[b * (T + 1) + s + 1] - V[b * (T + 1) + s];
  }
}


// ---------------------------------------------------------------------------------------------
// host side: the launch rules
// ---------------------------------------------------------------------------------------------
namespace mfg {

bool value_batch_ok(int d) { return d > WAVE && d % 16 == 0 && d <= MFG_MAX_D; }
size_t value_buffer_bytes(int64_t N, int d) { return value_batch_ok(d) ? (size_t)(2 * N) * 8 : 0; }

void grad_geometry(int64_t N, int d, int* chunk, int64_t* nsb, int* nob) {
  const int64_t FO = mfg_num_features(d) + 3;
  int ch = 8192 / d;
  if (ch > 64) ch = 64;
  if (ch < 8) ch = 8;
  *chunk = ch;
  int64_t sb = (N + ch - 1) / ch;
#ifndef MFG_GRAD_WS_MB
#define MFG_GRAD_WS_MB 72  // partial rows of the batch sums: 256 rows at d = 256 (one per CU; 32 MB until round 3)
#endif
  int64_t cap = (int64_t)((long long)MFG_GRAD_WS_MB << 20) / (FO * 8);
  if (cap > 1024) cap = 1024;
  if (cap < 16) cap = 16;
  if (sb > cap) sb = cap;
  if (sb < 1) sb = 1;
  *nsb = sb;
  *nob = (int)((FO + GR_OUT_PER_BLOCK - 1) / GR_OUT_PER_BLOCK);
}

void launch_reduce_partials(const double* partial, int64_t nsb, int64_t FO, int accumulate, double* G, const ReduceApply& ap,
                            hipStream_t st) {
  hipLaunchKernelGGL(k_reduce_partials, dim3((unsigned)((FO + RP_OUT - 1) / RP_OUT)), dim3(RP_SLICES * RP_OUT), 0, st, partial, nsb,
                     FO, accumulate, G, ap);
}

// `apply` (optional): also perform the parameter update; *applied tells whether it was done in-kernel.
int launch_grad(const float* pi, int64_t stride_b, const double* delta, const double* g, const float* reward, int64_t N, int T,
                int d, double* G, int accumulate, void* ws, size_t ws_bytes, hipStream_t st, const ApplyArgs* apply, bool* applied,
                bool add_reward, const PopArgs* pop) {
  if (applied) *applied = false;
  // FIRST, before anything can be launched: the d <= 28 kernel keeps a chunk's step counter s0 + j (s0 < T, j < 64) in a
  // 32-bit int (tests/test_gpu_batch_sums_layouts.py calls with such a T over buffers that hold nothing)
  if (d <= MFG_GRAD_SMALL_MAX_D && T > INT_MAX - GS_CH)
    return fail(MFG_EUNSUPPORTED, "batch sums, d <= %d: T = %d above 2^31 - 65", MFG_GRAD_SMALL_MAX_D, T);
  const int64_t FO = mfg_num_features(d) + 3;
  int chunk, nob;
  int64_t nsb;
  grad_geometry(N, d, &chunk, &nsb, &nob);
  const size_t need = (size_t)(nsb * FO * 8) + MFG_WS_CONTROL_BYTES;  // (the value buffer, if any, lies behind)
  if (ws_bytes < need) return fail(MFG_EWORKSPACE, "%s: need %lld bytes, have %lld", "workspace", (long long)need,
                                   (long long)ws_bytes);
  // the parameter update, when asked for, rides in the kernel that finishes the sums (fixed-order; needs accumulate == 0
  // so that the sample count is the host-known N)
  ReduceApply rap{};
  if (apply && !accumulate) {
    rap.on = 1;
    rap.lr_c = apply->lr_c;
    rap.lr_a = apply->lr_a;
    rap.count = (double)N;
    rap.w = apply->w;
    rap.theta = apply->theta;
    rap.reward_acc = apply->reward_acc;
  }
  GradArgs a{};
  a.pi = pi;
  a.stride_b = stride_b;
  a.delta = delta;
  a.g = g;
  a.reward = reward;
  a.N = N;
  a.T = T;
  a.d = d;
  a.chunk = chunk;
  a.nsb = nsb;
  a.partial = reinterpret_cast<double*>((char*)ws + MFG_WS_CONTROL_BYTES);
  // (the small-d kernel folds delta += reward into its own load: every sample is read by exactly one wave there; the
  //  other kernels read a sample from several blocks, so the update is a separate elementwise launch first)
  const bool small = d <= MFG_GRAD_SMALL_MAX_D;
  if (add_reward && !small)
    hipLaunchKernelGGL(k_add_reward, dim3(grid_for(N, 256, 8)), dim3(256), 0, st, const_cast<double*>(delta), reward, N);
  if (small) {
    a.add_reward = add_reward ? 1 : 0;
    // one partial row per block; nsb rows fit the workspace by construction (grad_geometry).  A wave works through chunks of
    // 64 samples: one chunk per wave while the batch is small, then more chunks per wave (two blocks per CU at most)
    const int64_t NC = (N + GS_CH - 1) / GS_CH;  // chunks of 64 samples, one wave each at a time
    int64_t blocks = (NC + WAVES - 1) / WAVES;
    const int64_t cap = (int64_t)num_cus() * MFG_GS_BPC;
    if (blocks > cap) blocks = cap;
    if (blocks > nsb) blocks = nsb;
    if (blocks < 1) blocks = 1;
    a.nsb = blocks;
    // few rows (small batches, per-step updates): the last block to finish sums them (and applies the update) itself
    const bool fuse = blocks <= MFG_GRAD_FUSE_MAX_ROWS;
    if (fuse) {
      a.counter = reinterpret_cast<unsigned*>(ws);
      a.G = G;
      a.accumulate = accumulate;
      if (apply) {
        a.apply = 1;
        a.lr_c = apply->lr_c;
        a.lr_a = apply->lr_a;
        a.w = apply->w;
        a.theta = apply->theta;
        a.reward_acc = apply->reward_acc;
        if (applied) *applied = true;
      }
    }
    // 32-bit offsets and the fp32 step division inside a chunk: skipped part below 2^23 floats, T below 2^22
    const bool wide = stride_b - (int64_t)T * d >= (1 << 23) || T >= MFG_GRAD_LONG_T;
    if (pop) {  // (population: K learners side by side; `wide` never holds for the strides and lengths of a training episode)
      if (wide) return fail(MFG_EUNSUPPORTED, "%s", "population: trajectory stride or length beyond the small gradient kernel");
      launch_grad_mfma_small_pop(d == 21 || d == 15 ? d : 0, (unsigned)blocks, a, *pop, st);
      if (fuse) return check_launch("grad_mfma_small_pop");
      launch_reduce_partials_pop((unsigned)((FO + RP_OUT - 1) / RP_OUT), (const double*)a.partial, blocks, FO, G, rap, *pop, st);
      if (applied && rap.on) *applied = true;
      return check_launch("grad_mfma_small_pop");
    }
    if (wide) hipLaunchKernelGGL((k_grad_mfma_small<0, true>), dim3((unsigned)blocks), dim3(BLOCK), 0, st, a);
    else if (d == 21) hipLaunchKernelGGL((k_grad_mfma_small<21>), dim3((unsigned)blocks), dim3(BLOCK), 0, st, a);
    else if (d == 15) hipLaunchKernelGGL((k_grad_mfma_small<15>), dim3((unsigned)blocks), dim3(BLOCK), 0, st, a);
    else hipLaunchKernelGGL((k_grad_mfma_small<0>), dim3((unsigned)blocks), dim3(BLOCK), 0, st, a);
    if (fuse) return check_launch("grad_mfma_small");
    launch_reduce_partials(a.partial, blocks, FO, accumulate, G, rap, st);
    if (applied && rap.on) *applied = true;
    return check_launch("grad_mfma_small");
  }
  if (d % 16 == 0 && d >= 64 && d <= 4 * BLOCK) {
    const int nt = d / 16, ntiles = nt * (nt + 1) / 2;
    const int ny = (ntiles + WAVES * GM_TPW - 1) / (WAVES * GM_TPW);
    const int tpw = (ntiles + ny * WAVES - 1) / (ny * WAVES);
    a.chunk = (BLOCK % (d / 4) == 0 && (((uintptr_t)pi & 15) == 0) && (stride_b % 4 == 0)) ? 1 : 0;  // float4 staging
    const size_t lds_m = (size_t)GM_KC * 8 + (size_t)4 * BLOCK * 8 + (size_t)GM_KC * (d + 16) * 4;
    const int npf = a.chunk ? d / 32 : 0;
    if (pop) {
      if (npf != 0 && npf != 2) return fail(MFG_EUNSUPPORTED, "%s", "population: d > 64");
      launch_grad_mfma_pop(npf, (unsigned)nsb, (unsigned)ny, lds_m, a, tpw, *pop, st);
      launch_reduce_partials_pop((unsigned)((FO + RP_OUT - 1) / RP_OUT), (const double*)a.partial, nsb, FO, G, rap, *pop, st);
      if (applied && rap.on) *applied = true;
      return check_launch("grad_mfma_pop");
    }
#ifndef MFG_GRAD_MFMA_OLD
    if (a.chunk && (d == 128 || d == 256)) {
      // two resident blocks per CU (two waves per SIMD: the second hides the first one's staging and barriers)
#ifndef MFG_GM2_BPC128
#define MFG_GM2_BPC128 3  // 166 registers: three blocks per CU fit (measured 253 -> 236 us at C3)
#endif
      const int64_t want = d == 256 ? (int64_t)num_cus() * 2 / Gm2Geom<256>::NY : (int64_t)num_cus() * MFG_GM2_BPC128 / Gm2Geom<128>::NY;
      if (nsb > want) nsb = want;
      a.nsb = nsb;
      if (d == 256) hipLaunchKernelGGL((k_grad_mfma2<256>), dim3((unsigned)nsb, (unsigned)Gm2Geom<256>::NY), dim3(BLOCK), lds_m, st, a);
      else hipLaunchKernelGGL((k_grad_mfma2<128>), dim3((unsigned)nsb, (unsigned)Gm2Geom<128>::NY), dim3(BLOCK), lds_m, st, a);
    } else
#endif
    switch (npf) {
      case 2: hipLaunchKernelGGL((k_grad_mfma<2>), dim3((unsigned)nsb, (unsigned)ny), dim3(BLOCK), lds_m, st, a, tpw); break;
      case 4: hipLaunchKernelGGL((k_grad_mfma<4>), dim3((unsigned)nsb, (unsigned)ny), dim3(BLOCK), lds_m, st, a, tpw); break;
      case 8: hipLaunchKernelGGL((k_grad_mfma<8>), dim3((unsigned)nsb, (unsigned)ny), dim3(BLOCK), lds_m, st, a, tpw); break;
      case 16: hipLaunchKernelGGL((k_grad_mfma<16>), dim3((unsigned)nsb, (unsigned)ny), dim3(BLOCK), lds_m, st, a, tpw); break;
      default: hipLaunchKernelGGL((k_grad_mfma<0>), dim3((unsigned)nsb, (unsigned)ny), dim3(BLOCK), lds_m, st, a, tpw); break;
    }
    launch_reduce_partials(a.partial, nsb, FO, accumulate, G, rap, st);
    if (applied && rap.on) *applied = true;
    return check_launch("grad_mfma");
  }
  const size_t lds = (size_t)chunk * 3 * 8 + (size_t)chunk * d * 4;
  if (pop) {
    launch_grad_partial_pop((unsigned)nsb, (unsigned)nob, lds, a, *pop, st);
    launch_reduce_partials_pop((unsigned)((FO + RP_OUT - 1) / RP_OUT), (const double*)a.partial, nsb, FO, G, rap, *pop, st);
    if (applied && rap.on) *applied = true;
    return check_launch("grad_partial_pop");
  }
  hipLaunchKernelGGL(k_grad_partial, dim3((unsigned)nsb, (unsigned)nob), dim3(BLOCK), lds, st, a);
  launch_reduce_partials(a.partial, nsb, FO, accumulate, G, rap, st);
  if (applied && rap.on) *applied = true;
  return check_launch("grad_reduce");
}

// After a TD rollout that skipped the in-kernel values (large d): V of all B (T+1) states, then delta.
int launch_values_and_delta(const float* pi_traj, int64_t B, int T, int d, const double* w, const float* reward,
                                   double gamma, int discount_pow, double* delta, void* ws, size_t ws_bytes, hipStream_t st) {
  const int64_t N = B * T, NV = B * (int64_t)(T + 1);
  int chunk, nob;
  int64_t nsb;
  grad_geometry(N, d, &chunk, &nsb, &nob);
  const size_t off = (size_t)(nsb * (mfg_num_features(d) + 3) * 8) + MFG_WS_CONTROL_BYTES;
  if (!ws || ws_bytes < off + (size_t)NV * 8)
    return fail(MFG_EWORKSPACE, "%s: need %lld bytes, have %lld", "values", (long long)(off + (size_t)NV * 8), (long long)ws_bytes);
  double* V = reinterpret_cast<double*>((char*)ws + off);
  const size_t lds = (size_t)WAVES * 16 * (d + 4) * 4 + (size_t)2 * VM_CH * 16 * 8;  // state rows + two pieces of U
  int64_t groups = (NV + 15) / 16;
  int64_t blocks = (groups + WAVES - 1) / WAVES;
  const int64_t cap = (int64_t)num_cus() * 8;
  if (blocks > cap) blocks = cap;
#ifndef MFG_VALUE_MFMA_OLD
  if (d % 64 == 0) {
    const size_t lds2 = (size_t)VM2_KC * 64 * 8 + (size_t)VM2_MB * VM2_XP * 4;
    int64_t blocks2 = (NV + VM2_MB - 1) / VM2_MB;
    if (blocks2 > (int64_t)num_cus() * 2) blocks2 = (int64_t)num_cus() * 2;
    hipLaunchKernelGGL(k_value_mfma2, dim3((unsigned)blocks2), dim3(BLOCK), lds2, st, pi_traj, (int64_t)(T + 1) * d, NV, T + 1, d, w, V);
  } else
#endif
  hipLaunchKernelGGL(k_value_mfma, dim3((unsigned)blocks), dim3(BLOCK), lds, st, pi_traj, (int64_t)(T + 1) * d, NV, T + 1, d, w, V);
  hipLaunchKernelGGL(k_td_delta, dim3(grid_for(N, 256, 8)), dim3(256), 0, st, (const double*)V, reward, B, T, gamma, discount_pow,
                     delta);
  return check_launch("values");
}

}  // namespace mfg
