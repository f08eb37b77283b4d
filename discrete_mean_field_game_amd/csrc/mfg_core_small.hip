// Instantiations of the packed small-d core kernel (d <= 64): generic runtime d plus compile-time
// specialisations for the reference's two problem sizes (d = 21: mfg_ac2.py:25, d = 15: ac_irl.py:33).
#include "mfg_core.h"

namespace mfg {

// Grid = tiles, capped at MFG_CORE_OVERSUBSCRIBE x the blocks that can be resident (registers AND LDS, asked from the
// runtime per instantiation); blocks loop over tiles beyond that.  Measured at d=21, B=65536 (5 462 tiles, 1 024
// resident blocks): exactly-resident persistent grid 2.30 ms, x1.5 2.21, x2 2.14, x4 2.07, one tile per block 2.07 --
// tiles do not take equal time (rejection retries), so the hardware dispatcher back-filling finished blocks beats
// a static tile split.
template <bool SAMPLE, bool TD, bool FAST, int D, bool SUMS = false, int STEP = 0>
static void go(const CoreArgs& a, int num_cus, size_t lds, hipStream_t st) {
  const int grid = core_small_grid<k_core_small<SAMPLE, TD, FAST, D, SUMS, STEP>>(a, lds, num_cus);
  // (STEP: the blocks that reduce the previous env step's partial rows ride behind the sampling blocks)
  hipLaunchKernelGGL((k_core_small<SAMPLE, TD, FAST, D, SUMS, STEP>), dim3(grid + (STEP == 1 ? core_step_red_blocks(a.d * (a.d + 1) / 2 + a.d + 1 + 3) : 0)), dim3(BLOCK), lds, st, a);
}

// the training call (k_core_small_lean, mfg_core.h): the same grid rule, asked for its own register count
template <int D>
static void go_lean(const CoreArgs& a, int num_cus, size_t lds, hipStream_t st) {
  const int grid = core_small_grid<k_core_small_lean<D>>(a, lds, num_cus);
  hipLaunchKernelGGL((k_core_small_lean<D>), dim3(grid), dim3(BLOCK), lds, st, a);
}

template <int D>
static void dispatch(const CoreArgs& a, bool sample, bool td, bool fast, int num_cus, size_t lds, hipStream_t st) {
  if constexpr (D > 0) {
    // IRL env step (mfg_train_episode_irl): theta from the previous step's partial rows, their reduction in the same launch
    if (sample && td && a.step_nrows > 0) {
      if (fast) go<true, true, true, D, false, 1>(a, num_cus, lds, st);
      else go<true, true, false, D, false, 1>(a, num_cus, lds, st);
      return;
    }
    if (sample && td && a.step_nrows < 0) {
      if (fast) go<true, true, true, D, false, 2>(a, num_cus, lds, st);
      else go<true, true, false, D, false, 2>(a, num_cus, lds, st);
      return;
    }
    // per-step updates: the variant that also leaves the tile's batch sums (core_sums_ok / reduce_core_sums in mfg_kernels.hip)
    if (sample && td && a.part_rows) {
      if (fast) go<true, true, true, D, true>(a, num_cus, lds, st);
      else go<true, true, false, D, true>(a, num_cus, lds, st);
      return;
    }
    // a training rollout with nothing optional asked for: the instantiation with those options compiled out (same bits);
    // every other launch takes the general kernel below (mapping mode 3 forces it: the test hook)
    if (sample && td && fast && core_lean_ok(a) && core_mapping_get() != 3) {
      go_lean<D>(a, num_cus, lds, st);
      return;
    }
  }
  if (fast) {
    if (sample && td) go<true, true, true, D>(a, num_cus, lds, st);
    else if (sample) go<true, false, true, D>(a, num_cus, lds, st);
    else go<false, true, true, D>(a, num_cus, lds, st);
  } else {
    if (sample && td) go<true, true, false, D>(a, num_cus, lds, st);
    else if (sample) go<true, false, false, D>(a, num_cus, lds, st);
    else go<false, true, false, D>(a, num_cus, lds, st);
  }
}

int launch_core_small(const CoreArgs& a, bool sample, bool td, bool fast, int num_cus, hipStream_t st) {
  const int d = a.d;
  // d = 21 batches that under-fill the machine: one trajectory per wave, three lanes per matrix row (mfg_core_row3.hip) --
  // the same bits as the packed kernel below, a wave's serial chain ~2.2x shorter
  if (core_row3_wanted(a, sample, td, fast, num_cus)) return launch_core_row3(a, td, num_cus, st);
  const bool want_v = td && a.w != nullptr;
  const size_t lds = core_small_lds(d, want_v, sample);
  if (d == 21) dispatch<21>(a, sample, td, fast, num_cus, lds, st);
  else if (d == 15) dispatch<15>(a, sample, td, fast, num_cus, lds, st);
  else dispatch<0>(a, sample, td, fast, num_cus, lds, st);
  return MFG_OK;
}

}  // namespace mfg
