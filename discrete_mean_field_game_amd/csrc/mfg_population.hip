// Population forms of the kernels of a training episode at d <= 64 (mfg_population.h): the start draw, the packed core kernel
// (plain, SUMS and the IRL env-step variants), the gradient kernels and the two row reductions with their update.  Each wrapper
// rebases the argument block to learner k and runs the body of the single kernel (core_small_body, grad_*_body,
// reduce_partials_body, reduce_rows_apply_body, draw_start_body).
//
// Every training wrapper exists twice.  k_*_pop serves the launch without a control block: it reads no control field and is,
// instruction for instruction, the kernel it was before control blocks existed.  k_*_pop_ctl serves the launch with one
// (PopArgs::state set): it first tests its learner's state.  Each launcher picks by p.state, so a call without a block pays
// nothing for the test (measured: in the shared form it cost the step-mode episodes up to 7 %).  The pairs are written out and
// not folded into one inlined function with a compile-time flag: passing the argument blocks through such a function changed
// the register allocation and the schedule of the plain forms (tools/kernel_isa_diff.py; docs/HISTORY.md has the table).
// The packed core kernel's pair is written out in mfg_population_core.h; its _ctl half is instantiated by mfg_population_ctl.hip,
// a translation unit of its own (the two halves compile side by side).
#include "mfg_core.h"
#include "mfg_grad.h"
#include "mfg_population.h"
#include "mfg_population_core.h"

namespace mfg {

// ---- packed core kernel (mfg_population_core.h): the plain forms here, the _ctl forms in mfg_population_ctl.hip ----
int launch_core_pop(const CoreArgs& a, const PopArgs& p, bool fast, int num_cus, hipStream_t st) {
  return p.state ? launch_core_pop_ctl(a, p, fast, num_cus, st) : launch_core_pop_forms<false>(a, p, fast, num_cus, st);
}

// ---- start-state draw (a9) of learner blockIdx.y ----
__global__ void k_draw_start_pop(const float* __restrict__ mat, int64_t num_start, int64_t B, int d, uint32_t step,
                                 uint64_t traj_offset, float* __restrict__ out, PopArgs p) {
  const int k = blockIdx.y;
  draw_start_body(mat, num_start, B, d, p.seed[k], step, traj_offset, nullptr, out + p.s_state * k);
}
__global__ void k_draw_start_pop_ctl(const float* __restrict__ mat, int64_t num_start, int64_t B, int d, uint32_t step,
                                     uint64_t traj_offset, float* __restrict__ out, PopArgs p) {
  const int k = blockIdx.y;
  if (pop_retired(p, k)) return;
  draw_start_body(mat, num_start, B, d, p.seed[k], step, traj_offset, nullptr, out + p.s_state * k);
}

void launch_draw_start_pop(int grid, const float* mat, int64_t num_start, int64_t B, int d, uint32_t step, uint64_t traj_offset,
                           float* out, const PopArgs& p, hipStream_t st) {
  hipLaunchKernelGGL(p.state ? k_draw_start_pop_ctl : k_draw_start_pop, dim3((unsigned)grid, (unsigned)p.K), dim3(256), 0, st, mat,
                     num_start, B, d, step, traj_offset, out, p);
}

// ---- batch sums of the update (+ the fused finish and update of the small-d kernel) ----
__device__ __forceinline__ void pop_rebase_grad(GradArgs& a, const PopArgs& p, int k) {
  a.pi += p.s_gpi * k;
  a.delta += p.s_n * k;
  a.g += p.s_n * k;
  a.reward = pop_at(a.reward, p.s_n, k);
  a.partial = pop_bytes(a.partial, p.s_ws, k);
  a.counter = pop_bytes(a.counter, p.s_ws, k);
  a.G = pop_at(a.G, p.F + 3, k);
  a.w = pop_at(a.w, p.F, k);
  a.theta = pop_at(a.theta, 1, k);
  a.reward_acc = pop_at(a.reward_acc, p.s_acc, k);
  a.lr_c = p.lr_c[k] * p.sc;
  a.lr_a = p.lr_a[k] * p.sa;
}

template <int D>
__global__ __launch_bounds__(BLOCK) void k_grad_mfma_small_pop(GradArgs a, PopArgs p) {
  GradArgs b = a;
  pop_rebase_grad(b, p, blockIdx.y);
  grad_mfma_small_body<D, false>(b);
}
template <int D>
__global__ __launch_bounds__(BLOCK) void k_grad_mfma_small_pop_ctl(GradArgs a, PopArgs p) {
  if (pop_retired(p, blockIdx.y)) return;
  GradArgs b = a;
  pop_rebase_grad(b, p, blockIdx.y);
  grad_mfma_small_body<D, false>(b);
}

__global__ __launch_bounds__(BLOCK) void k_grad_partial_pop(GradArgs a, PopArgs p) {
  GradArgs b = a;
  pop_rebase_grad(b, p, blockIdx.z);
  grad_partial_body(b);
}
__global__ __launch_bounds__(BLOCK) void k_grad_partial_pop_ctl(GradArgs a, PopArgs p) {
  if (pop_retired(p, blockIdx.z)) return;
  GradArgs b = a;
  pop_rebase_grad(b, p, blockIdx.z);
  grad_partial_body(b);
}

template <int NPF>
__global__ __launch_bounds__(BLOCK) void k_grad_mfma_pop(GradArgs a, int tpw, PopArgs p) {
  GradArgs b = a;
  pop_rebase_grad(b, p, blockIdx.z);
  grad_mfma_body<NPF>(b, tpw);
}
template <int NPF>
__global__ __launch_bounds__(BLOCK) void k_grad_mfma_pop_ctl(GradArgs a, int tpw, PopArgs p) {
  if (pop_retired(p, blockIdx.z)) return;
  GradArgs b = a;
  pop_rebase_grad(b, p, blockIdx.z);
  grad_mfma_body<NPF>(b, tpw);
}

#define MFG_REDUCE_PARTIALS_POP()                                                                                        \
  ReduceApply q = ap;                                                                                                    \
  if (q.on) {                                                                                                            \
    q.w = pop_at(ap.w, p.F, k);                                                                                          \
    q.theta = pop_at(ap.theta, 1, k);                                                                                    \
    q.reward_acc = pop_at(ap.reward_acc, p.s_acc, k);                                                                    \
    q.lr_c = p.lr_c[k] * p.sc;                                                                                           \
    q.lr_a = p.lr_a[k] * p.sa;                                                                                           \
  }                                                                                                                      \
  /* (partial is never null: moved without pop_bytes' null test, which cost the kernel an SGPR) */                       \
  reduce_partials_body(reinterpret_cast<const double*>(reinterpret_cast<const char*>(partial) + p.s_ws * k), nsb, FO, 0, \
                       G + FO * k, q)
__global__ __launch_bounds__(RP_SLICES* RP_OUT) void k_reduce_partials_pop(const double* __restrict__ partial, int64_t nsb,
                                                                          int64_t FO, double* __restrict__ G, ReduceApply ap,
                                                                          PopArgs p) {
  const int k = blockIdx.y;
  MFG_REDUCE_PARTIALS_POP();
}
__global__ __launch_bounds__(RP_SLICES* RP_OUT) void k_reduce_partials_pop_ctl(const double* __restrict__ partial, int64_t nsb,
                                                                              int64_t FO, double* __restrict__ G, ReduceApply ap,
                                                                              PopArgs p) {
  const int k = blockIdx.y;
  if (pop_retired(p, k)) return;
  MFG_REDUCE_PARTIALS_POP();
}
#undef MFG_REDUCE_PARTIALS_POP

void launch_grad_mfma_small_pop(int D, unsigned blocks, const GradArgs& a, const PopArgs& p, hipStream_t st) {
  const dim3 grid(blocks, (unsigned)p.K);
  auto* k = D == 21   ? (p.state ? k_grad_mfma_small_pop_ctl<21> : k_grad_mfma_small_pop<21>)
            : D == 15 ? (p.state ? k_grad_mfma_small_pop_ctl<15> : k_grad_mfma_small_pop<15>)
                      : (p.state ? k_grad_mfma_small_pop_ctl<0> : k_grad_mfma_small_pop<0>);
  hipLaunchKernelGGL(k, grid, dim3(BLOCK), 0, st, a, p);
}

void launch_grad_partial_pop(unsigned nsb, unsigned nob, size_t lds, const GradArgs& a, const PopArgs& p, hipStream_t st) {
  hipLaunchKernelGGL(p.state ? k_grad_partial_pop_ctl : k_grad_partial_pop, dim3(nsb, nob, (unsigned)p.K), dim3(BLOCK), lds, st, a,
                     p);
}

void launch_grad_mfma_pop(int npf, unsigned nsb, unsigned ny, size_t lds, const GradArgs& a, int tpw, const PopArgs& p,
                          hipStream_t st) {
  const dim3 grid(nsb, ny, (unsigned)p.K);
  auto* k = npf == 2 ? (p.state ? k_grad_mfma_pop_ctl<2> : k_grad_mfma_pop<2>) : (p.state ? k_grad_mfma_pop_ctl<0> : k_grad_mfma_pop<0>);
  hipLaunchKernelGGL(k, grid, dim3(BLOCK), lds, st, a, tpw, p);
}

void launch_reduce_partials_pop(unsigned nob, const double* partial, int64_t nsb, int64_t FO, double* G, const ReduceApply& ap,
                                const PopArgs& p, hipStream_t st) {
  hipLaunchKernelGGL(p.state ? k_reduce_partials_pop_ctl : k_reduce_partials_pop, dim3(nob, (unsigned)p.K),
                     dim3(RP_SLICES * RP_OUT), 0, st, partial, nsb, FO, G, ap, p);
}

// ---- the row reduction + update that closes a step-mode IRL episode, learner blockIdx.y ----
__global__ __launch_bounds__(BLOCK) void k_reduce_rows_apply_pop(const double* __restrict__ rows, int nrows, int64_t FO,
                                                                 double* __restrict__ G, double count, double* __restrict__ w,
                                                                 const double* theta_in, double* theta_out,
                                                                 double* __restrict__ reward_acc, double* slots, PopArgs p) {
  const int k = blockIdx.y;
  reduce_rows_apply_body(pop_bytes(rows, p.s_ws, k), nrows, FO, G + FO * k, p.lr_c[k] * p.sc, p.lr_a[k] * p.sa, count,
                         w + p.F * k, pop_bytes(theta_in, p.s_theta_b, k), theta_out + k, pop_at(reward_acc, p.s_acc, k),
                         pop_bytes(slots, p.s_ws, k));
}
__global__ __launch_bounds__(BLOCK) void k_reduce_rows_apply_pop_ctl(const double* __restrict__ rows, int nrows, int64_t FO,
                                                                     double* __restrict__ G, double count,
                                                                     double* __restrict__ w, const double* theta_in,
                                                                     double* theta_out, double* __restrict__ reward_acc,
                                                                     double* slots, PopArgs p) {
  const int k = blockIdx.y;
  if (pop_retired(p, k)) return;
  reduce_rows_apply_body(pop_bytes(rows, p.s_ws, k), nrows, FO, G + FO * k, p.lr_c[k] * p.sc, p.lr_a[k] * p.sa, count,
                         w + p.F * k, pop_bytes(theta_in, p.s_theta_b, k), theta_out + k, pop_at(reward_acc, p.s_acc, k),
                         pop_bytes(slots, p.s_ws, k));
}

void launch_reduce_rows_apply_pop(const double* rows, int nrows, int64_t FO, double* G, double count, double* w,
                                  const double* theta_in, double* theta_out, double* reward_acc, double* slots, const PopArgs& p,
                                  hipStream_t st) {
  hipLaunchKernelGGL(p.state ? k_reduce_rows_apply_pop_ctl : k_reduce_rows_apply_pop,
                     dim3((unsigned)((FO + WAVES - 1) / WAVES), (unsigned)p.K), dim3(BLOCK), 0, st, rows, nrows, FO, G, count, w,
                     theta_in, theta_out, reward_acc, slots, p);
}

// ---- the learners' activity states between two episodes (mfg_population.h): one wave, learner blockIdx.x ----
__global__ __launch_bounds__(WAVE) void k_pop_retire(mfg_pop_control_t c, const double* __restrict__ theta,
                                                     const double* __restrict__ w, int64_t F, const double* __restrict__ shift,
                                                     int mixed, int after_episode) {
  const int k = blockIdx.x, lane = threadIdx.x;
  if (c.state[k] != 0) return;
  const double th = theta[k];
  bool nonfinite = !isfinite(th);
  for (int64_t j = lane; j < F; j += WAVE) nonfinite |= !isfinite(w[F * k + j]);
  nonfinite = __any(nonfinite);
  // (the predicate of report_sep_range; true for a NaN theta too)
  const bool range = mixed && !(fabs(th) * (1.0 + fabs(shift[k])) <= SEP_LIMIT);
  if (lane != 0) return;
  const unsigned bits = (mixed ? c.status[k] : 0u) | (range ? (unsigned)MFG_STATUS_MIXED_RANGE : 0u) |
                        (nonfinite ? (unsigned)MFG_STATUS_POP_NONFINITE : 0u);
  if (bits) {
    c.status[k] = bits;
    c.state[k] = 2;
    return;
  }
  if (after_episode) {
    c.episodes_run[k] += 1;
    if (fabs(th - c.theta_prev[k]) < c.stop_criteria[k]) c.state[k] = 1;  // (ac_irl.py:726; a criterion < 0 never stops)
  }
  c.theta_prev[k] = th;
}

void launch_pop_retire(const mfg_pop_control_t& c, const double* theta, const double* w, int64_t F, const double* shift, bool mixed,
                       bool after_episode, hipStream_t st) {
  hipLaunchKernelGGL(k_pop_retire, dim3((unsigned)c.K), dim3(WAVE), 0, st, c, theta, w, F, shift, mixed ? 1 : 0,
                     after_episode ? 1 : 0);
}

}  // namespace mfg
