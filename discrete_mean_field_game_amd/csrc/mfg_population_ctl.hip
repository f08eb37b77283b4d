// The packed core kernel's population forms for a launch WITH a control block (k_core_pop_ctl, mfg_population_core.h), in a
// translation unit of their own so that they compile beside the plain forms of mfg_population.hip instead of behind them.
// Same flags as mfg_population.hip (csrc/Makefile).
#include "mfg_population_core.h"

namespace mfg {

int launch_core_pop_ctl(const CoreArgs& a, const PopArgs& p, bool fast, int num_cus, hipStream_t st) {
  return launch_core_pop_forms<true>(a, p, fast, num_cus, st);
}

}  // namespace mfg
