// Population forms of the IRL episode's core kernel and closing row reduction (mfg_irl_population.h): each wrapper rebases the
// argument block to learner blockIdx.y and runs the body of the single kernel (core_small_body, reduce_rows_apply_body).  The
// reward network's population form is in mfg_reward_net.hip, next to its body.
#include <atomic>

#include "mfg_core.h"
#include "mfg_irl_population.h"

namespace mfg {

template <class P>
__device__ __forceinline__ P* irl_pop_at(P* p, int64_t stride, int k) {
  return p ? p + stride * k : p;
}
template <class P>
__device__ __forceinline__ P* irl_pop_bytes(P* p, int64_t bytes, int k) {
  return p ? reinterpret_cast<P*>(reinterpret_cast<char*>(const_cast<std::remove_const_t<P>*>(p)) + bytes * k) : p;
}

// ---- packed core kernel, IRL variants (external reward): STEP 0 the rollout with P materialised, STEP 1 / 2 an env step ----
template <bool FAST, int D, int STEP>
__global__ __launch_bounds__(BLOCK, FAST ? MFG_CORE_SMALL_WAVES : MFG_CORE_SMALL_WAVES_F64) void k_core_irl_pop(CoreArgs a,
                                                                                                                IrlCorePop p) {
  const int k = blockIdx.y;
  CoreArgs b = a;
  b.pi0 = irl_pop_at(a.pi0, p.s_pi0, k);
  b.theta = irl_pop_bytes(a.theta, p.s_theta_b, k);
  b.w = irl_pop_at(a.w, p.F, k);
  b.shift = p.shift[k];
  b.alpha_scale = p.alpha_scale[k];
  b.seed = p.seed[k];
  b.pi_traj = irl_pop_at(a.pi_traj, p.s_traj, k);
  b.pi_next_out = irl_pop_at(a.pi_next_out, p.s_state, k);
  b.delta = irl_pop_at(a.delta, p.s_n, k);
  b.g = irl_pop_at(a.g, p.s_n, k);
  b.P_out = irl_pop_at(a.P_out, p.s_P, k);
  if constexpr (STEP == 2) b.pi_start_out = irl_pop_at(a.pi_start_out, p.s_state, k);
  if constexpr (STEP == 1) {
    b.step_G = irl_pop_at(a.step_G, p.F + 3, k);
    b.step_rows = irl_pop_bytes(a.step_rows, p.s_ws, k);
    b.w_out = irl_pop_at(a.w_out, p.F, k);
    b.theta_out = irl_pop_bytes(a.theta_out, p.s_ws, k);
    b.pend_reward_acc = irl_pop_at(a.pend_reward_acc, p.s_acc, k);
    b.pend_lr_c = p.lr_c[k] * p.sc;
    b.pend_lr_a = p.lr_a[k] * p.sa;
  }
  core_small_body<true, true, FAST, D, false, STEP>(b);
}

template <bool FAST, int D, int STEP>
static void go_irl_pop(const CoreArgs& a, const IrlCorePop& p, int num_cus, size_t lds, hipStream_t st) {
  // occupancy of this instantiation at this LDS size, cached per device (as launch_core_small does for the single kernel)
  static std::atomic<size_t> cached_lds[64];
  static std::atomic<int> cached_bpc[64];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
  if (cached_lds[dev].load() != lds + 1) {
    int n = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, k_core_irl_pop<FAST, D, STEP>, BLOCK, lds) != hipSuccess || n < 1) n = 1;
    cached_bpc[dev].store(n);
    cached_lds[dev].store(lds + 1);
  }
  const int TB = WAVES * (WAVE / a.d);
  const int grid = core_grid(a.B, TB, cached_bpc[dev].load() * (a.T == 1 ? 2 : MFG_CORE_OVERSUBSCRIBE), num_cus) +
                   (STEP == 1 ? core_step_red_blocks(a.d * (a.d + 1) / 2 + a.d + 1 + 3) : 0);
  hipLaunchKernelGGL((k_core_irl_pop<FAST, D, STEP>), dim3((unsigned)grid, (unsigned)p.K), dim3(BLOCK), lds, st, a, p);
}

template <int D, int STEP>
static void dispatch_irl_pop(const CoreArgs& a, const IrlCorePop& p, bool fast, int num_cus, size_t lds, hipStream_t st) {
  if (fast) go_irl_pop<true, D, STEP>(a, p, num_cus, lds, st);
  else go_irl_pop<false, D, STEP>(a, p, num_cus, lds, st);
}

template <int D>
static void dispatch_irl_pop_d(const CoreArgs& a, const IrlCorePop& p, bool fast, int num_cus, size_t lds, hipStream_t st) {
  if (a.step_nrows > 0) dispatch_irl_pop<D, 1>(a, p, fast, num_cus, lds, st);
  else if (a.step_nrows < 0) dispatch_irl_pop<D, 2>(a, p, fast, num_cus, lds, st);
  else dispatch_irl_pop<D, 0>(a, p, fast, num_cus, lds, st);
}

// Always the packed lane mapping (k_core_row3 gives the same bits for the batches it serves); d = 21 / 15, sampling + TD
int launch_core_irl_pop(const CoreArgs& a, const IrlCorePop& p, bool fast, int num_cus, hipStream_t st) {
  const size_t lds = core_small_lds(a.d, a.w != nullptr, true);
  if (a.d == 21) dispatch_irl_pop_d<21>(a, p, fast, num_cus, lds, st);
  else if (a.d == 15) dispatch_irl_pop_d<15>(a, p, fast, num_cus, lds, st);
  else return MFG_EUNSUPPORTED;
  return MFG_OK;
}

// ---- the row reduction + update that closes a step-mode episode, learner blockIdx.y ----
__global__ __launch_bounds__(BLOCK) void k_reduce_rows_apply_pop(const double* __restrict__ rows, int nrows, int64_t FO,
                                                                 double* __restrict__ G, double count, double* __restrict__ w,
                                                                 const double* theta_in, int64_t s_theta_in_b,
                                                                 double* theta_out, double* __restrict__ reward_acc,
                                                                 IrlCorePop p) {
  const int k = blockIdx.y;
  reduce_rows_apply_body(irl_pop_bytes(rows, p.s_ws, k), nrows, FO, G + FO * k, p.lr_c[k] * p.sc, p.lr_a[k] * p.sa, count,
                         w + p.F * k, irl_pop_bytes(theta_in, s_theta_in_b, k), theta_out + k, irl_pop_at(reward_acc, p.s_acc, k));
}

void launch_reduce_rows_apply_pop(const double* rows, int nrows, int64_t FO, double* G, double count, double* w,
                                  const double* theta_in, int64_t s_theta_in_b, double* theta_out, double* reward_acc,
                                  const IrlCorePop& p, hipStream_t st) {
  hipLaunchKernelGGL(k_reduce_rows_apply_pop, dim3((unsigned)((FO + WAVES - 1) / WAVES), (unsigned)p.K), dim3(BLOCK), 0, st, rows,
                     nrows, FO, G, count, w, theta_in, s_theta_in_b, theta_out, reward_acc, p);
}

}  // namespace mfg
