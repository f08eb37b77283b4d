// The packed core kernel's population forms and their dispatch, shared by the two translation units that instantiate them:
// mfg_population.hip the plain forms (k_core_pop), mfg_population_ctl.hip the forms of a launch with a control block
// (k_core_pop_ctl).  Each unit instantiates only its own half -- the 18 instantiations of one form are the longest compile
// of the library -- and launch_core_pop picks across the two by p.state.  Why the two forms are written out and not folded
// into one: see the head of mfg_population.hip.
#pragma once
#include "mfg_core.h"
#include "mfg_population.h"

namespace mfg {

// ---- packed core kernel: sampling, transition, value, TD error, score of learner blockIdx.y; SUMS: the tile's batch-sum rows;
//      STEP 1 / 2: an IRL env step (external reward, P materialised) ----
#define MFG_CORE_POP_BOUNDS __launch_bounds__(BLOCK, SUMS ? 2 : (FAST ? MFG_CORE_SMALL_WAVES : MFG_CORE_SMALL_WAVES_F64))
template <bool FAST, int D, bool SUMS, int STEP>
__global__ MFG_CORE_POP_BOUNDS void k_core_pop(CoreArgs a, PopArgs p) {
  core_small_body<true, true, FAST, D, SUMS, STEP>(pop_core_args<SUMS, STEP>(a, p, blockIdx.y));
}
template <bool FAST, int D, bool SUMS, int STEP>
__global__ MFG_CORE_POP_BOUNDS void k_core_pop_ctl(CoreArgs a, PopArgs p) {
  if (pop_retired(p, blockIdx.y)) return;
  core_small_body<true, true, FAST, D, SUMS, STEP>(pop_core_args<SUMS, STEP, true>(a, p, blockIdx.y));
}
#undef MFG_CORE_POP_BOUNDS

template <bool CTL, bool FAST, int D, bool SUMS, int STEP>
static void go_pop(const CoreArgs& a, const PopArgs& p, int num_cus, size_t lds, hipStream_t st) {
  const int red = STEP == 1 ? core_step_red_blocks(a.d * (a.d + 1) / 2 + a.d + 1 + 3) : 0;
  if constexpr (CTL) {
    const int grid = core_small_grid<k_core_pop_ctl<FAST, D, SUMS, STEP>>(a, lds, num_cus) + red;
    hipLaunchKernelGGL((k_core_pop_ctl<FAST, D, SUMS, STEP>), dim3((unsigned)grid, (unsigned)p.K), dim3(BLOCK), lds, st, a, p);
  } else {
    const int grid = core_small_grid<k_core_pop<FAST, D, SUMS, STEP>>(a, lds, num_cus) + red;
    hipLaunchKernelGGL((k_core_pop<FAST, D, SUMS, STEP>), dim3((unsigned)grid, (unsigned)p.K), dim3(BLOCK), lds, st, a, p);
  }
}

// (as dispatch<D> in mfg_core_small.hip, sampling + TD only)
template <bool CTL, int D>
static void dispatch_pop(const CoreArgs& a, const PopArgs& p, bool fast, int num_cus, size_t lds, hipStream_t st) {
  if constexpr (D > 0) {
    if (a.step_nrows > 0) {
      if (fast) go_pop<CTL, true, D, false, 1>(a, p, num_cus, lds, st);
      else go_pop<CTL, false, D, false, 1>(a, p, num_cus, lds, st);
      return;
    }
    if (a.step_nrows < 0) {
      if (fast) go_pop<CTL, true, D, false, 2>(a, p, num_cus, lds, st);
      else go_pop<CTL, false, D, false, 2>(a, p, num_cus, lds, st);
      return;
    }
    if (a.part_rows) {
      if (fast) go_pop<CTL, true, D, true, 0>(a, p, num_cus, lds, st);
      else go_pop<CTL, false, D, true, 0>(a, p, num_cus, lds, st);
      return;
    }
  }
  if (fast) go_pop<CTL, true, D, false, 0>(a, p, num_cus, lds, st);
  else go_pop<CTL, false, D, false, 0>(a, p, num_cus, lds, st);
}

// The body of launch_core_pop (CTL false) / launch_core_pop_ctl (CTL true).  Always the packed lane mapping: k_core_row3 is
// for batches that under-fill the machine, a population fills it (both mappings give the same bits).  Training launches only
// (sampling + TD).
template <bool CTL>
static int launch_core_pop_forms(const CoreArgs& a, const PopArgs& p, bool fast, int num_cus, hipStream_t st) {
  const int d = a.d;
  if (d > WAVE) return MFG_EUNSUPPORTED;
  const size_t lds = core_small_lds(d, a.w != nullptr, true);
  if (d == 21) dispatch_pop<CTL, 21>(a, p, fast, num_cus, lds, st);
  else if (d == 15) dispatch_pop<CTL, 15>(a, p, fast, num_cus, lds, st);
  else if (!a.part_rows && a.step_nrows == 0) dispatch_pop<CTL, 0>(a, p, fast, num_cus, lds, st);
  else return MFG_EUNSUPPORTED;  // (SUMS rows and the STEP variants: compile-time d only)
  return MFG_OK;
}

}  // namespace mfg
