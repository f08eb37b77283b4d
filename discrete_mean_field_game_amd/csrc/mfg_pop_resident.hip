// Step-mode episodes of a small-batch population with every learner resident in one workgroup (mfg_train_episodes_pop_resident,
// include/mfg_hip.h; the reference's per-step updates, mfg_ac2.py:478-526).
//
// k_pop_resident<FAST, D>: grid (1, K), BLOCK threads, block k = learner k.  For every episode of the launch the block draws
// the learner's start states (draw_start_body), then runs T x [env step over all of the learner's tiles | row reduction +
// update], and finally leaves the last states in pi_io.  The env step is core_small_body<true, true, FAST, D, SUMS> itself --
// with a grid of one block it walks every tile and leaves a partial row per tile in the learner's workspace slice -- so its
// samples, TD errors, scores and rows are those of k_core_pop<FAST, D, true, 0>.  The reduction restates the order of
// reduce_partials_body (mfg_grad.h) for at most RP_SLICES rows, see resident_column_sum below.
//
// What passes from wave to wave -- states, partial rows, parameters -- stays inside the workgroup: __syncthreads() between
// the phases is the only synchronisation.  No fence wider than the workgroup, no flag, no spin; blocks of different learners
// never communicate.  (The one atomic is report_sep_range's, inside the env step: the range report into the status word that
// every mixed-precision sampling kernel makes.  Nothing waits on it.)
//
// theta and w live in LDS (par) and in a register of the thread that updates them; global memory gets them once, at the end
// of the launch.  The env step reads its parameters through CoreArgs::theta / w, which here point INTO LDS: a global address
// that this kernel also stores to could be fetched through the scalar data cache, which does not see the kernel's own vector
// stores.  States and partial rows are written and re-read with per-lane (vector) accesses on both sides of a barrier.
#include "mfg_core.h"
#include "mfg_grad.h"
#include "mfg_population.h"

namespace mfg {

static_assert(MFG_POP_RESIDENT_MAX_TILES <= RP_SLICES, "resident_column_sum: at most one row per slice of reduce_partials_body");

// Column `col` of the learner's `nt` <= RP_SLICES partial rows, added in the order of reduce_partials_body: there slice q holds
// row q alone (s0 = 0 + row, s1 = s2 = s3 = 0, (s0 + s1) + (s2 + s3) = 0 + row: a sum with +0 is never -0, and adding +0 to
// anything else changes nothing), a slice without a row holds +0, and the 64 slice sums go into t0 .. t3 by q mod 4, in slice
// order, closed by (t0 + t1) + (t2 + t3).  The +0 of the slices q >= nt leaves a running sum as it is: the loop stops at nt.
__device__ __forceinline__ double resident_column_sum(const double* rows, int nt, int FO, int col) {
  double t0 = 0.0, t1 = 0.0, t2 = 0.0, t3 = 0.0;
  for (int q = 0; q < nt; q += 4) {
    const double v0 = rows[(int64_t)q * FO + col];
    const double v1 = q + 1 < nt ? rows[(int64_t)(q + 1) * FO + col] : 0.0;
    const double v2 = q + 2 < nt ? rows[(int64_t)(q + 2) * FO + col] : 0.0;
    const double v3 = q + 3 < nt ? rows[(int64_t)(q + 3) * FO + col] : 0.0;
    t0 += 0.0 + v0;
    t1 += 0.0 + v1;
    t2 += 0.0 + v2;
    t3 += 0.0 + v3;
  }
  return (t0 + t1) + (t2 + t3);
}

template <bool FAST, int D>
__global__ __launch_bounds__(BLOCK, 2) void k_pop_resident(CoreArgs a, PopArgs p, PopResidentArgs r) {
  constexpr int F = D * (D + 1) / 2 + D + 1, FO = F + 3;
  constexpr int TB = WAVES * (WAVE / D);
  static_assert(FO <= BLOCK, "a thread per column of the rows");
  __shared__ double par[F + 1];  // w [F], theta
  const int k = blockIdx.y, tid = threadIdx.x;
  const int nt = (int)((a.B + TB - 1) / TB);
  const int64_t n_state = a.B * D;

  CoreArgs b = pop_core_args<true, 0>(a, p, k);  // (shift, alpha_scale, seed, reward / delta / g, the rows of learner k)
  b.theta = &par[F];
  b.w = par;
  float* const io = r.pi_io + p.s_state * k;
  float* const scratch = r.pi_scratch + p.s_state * k;
  double* const w_g = r.w + p.F * k;
  double* const G_g = r.G + (int64_t)FO * k;
  const double* const rows = b.part_rows;

  // thread c < F carries w[c], thread F theta, thread F + 1 the episode's return
  double val = 0.0;
  if (tid < F) val = w_g[tid];
  else if (tid == F) val = r.theta[k];
  if (tid <= F) par[tid] = val;
  const double lr_c0 = p.lr_c[k], lr_a0 = p.lr_a[k];
  const double inv = 1.0 / (double)a.B;

  float* cur = io;
  for (int e = 0; e < r.episodes; ++e) {
    const uint32_t step0 = r.first_step + (uint32_t)e * (uint32_t)r.T;
    draw_start_body(r.mat_pi0, r.num_start, a.B, D, b.seed, step0, a.traj_offset, nullptr, io);
    const double lr_c = lr_c0 * r.sc[e];
    const double lr_a = lr_a0 * r.sa[e];
    double* const acc = r.reward_acc ? r.reward_acc + p.s_acc * k + e : nullptr;
    if (tid == F + 1 && acc) val = *acc;
    __syncthreads();  // start states (and, in the first episode, par) are in place
    cur = io;
    float* nxt = scratch;
    for (int s = 0; s < r.T; ++s) {
      b.pi0 = cur;
      b.pi_next_out = nxt;
      b.first_step = step0 + (uint32_t)s;
      core_small_body<true, true, FAST, D, true, 0>(b);
      __syncthreads();  // every tile's row is written
      if (tid < FO) {
        const double gk = resident_column_sum(rows, nt, FO, tid);
        if (e == r.episodes - 1 && s == r.T - 1) G_g[tid] = gk;
        if (tid < F) {
          val = updated_param(val, lr_c, gk, inv);
          par[tid] = val;
        } else if (tid == F) {
          val = updated_param(val, lr_a, gk, inv);
          par[F] = val;
        } else if (tid == F + 1 && acc) {
          val = val + gk * inv;
        }
      }
      __syncthreads();  // the parameters of the next step are in par; the rows and `cur` may be overwritten
      float* const t = cur;
      cur = nxt;
      nxt = t;
    }
    if (tid == F + 1 && acc) *acc = val;
  }
  if (tid < F) w_g[tid] = val;
  else if (tid == F) r.theta[k] = val;
  if (cur != io)  // (T odd: the last step wrote the scratch side)
    for (int64_t j = tid; j < n_state; j += BLOCK) io[j] = cur[j];
}

template <bool FAST, int D>
static void go_resident(const CoreArgs& a, const PopArgs& p, const PopResidentArgs& r, hipStream_t st) {
  hipLaunchKernelGGL((k_pop_resident<FAST, D>), dim3(1u, (unsigned)p.K), dim3(BLOCK), core_small_lds(D, true, true), st, a, p, r);
}

int launch_pop_resident(const CoreArgs& a, const PopArgs& p, const PopResidentArgs& r, bool fast, hipStream_t st) {
  if (a.d == 21) fast ? go_resident<true, 21>(a, p, r, st) : go_resident<false, 21>(a, p, r, st);
  else if (a.d == 15) fast ? go_resident<true, 15>(a, p, r, st) : go_resident<false, 15>(a, p, r, st);
  else return MFG_EUNSUPPORTED;
  return MFG_OK;
}

}  // namespace mfg
