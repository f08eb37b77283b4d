// Host-side plumbing shared by the translation units that hold C entry points or launch rules: the error record behind
// mfg_last_error(), the argument-check macros, and the grid sizing.  Everything here is defined once, in mfg_kernels.hip
// (one thread-local error buffer, one per-device CU cache).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mfg_hip.h"

namespace mfg {

// records the printf-formatted message for mfg_last_error() (per thread) and returns `code`
int fail(int code, const char* fmt, ...);
// MFG_OK, or MFG_ELAUNCH with "<what>: <HIP's error string>" recorded, after the launches of an entry point
int check_launch(const char* what);
// CU count of the CURRENT device (cached per device: one context may drive several GPUs from one process)
int num_cus();
// blocks for `work_items` items at `per_block` items per block, capped at `blocks_per_cu` resident blocks per CU
int grid_for(int64_t work_items, int per_block, int blocks_per_cu);

static inline hipStream_t S(mfg_stream_t s) { return (hipStream_t)s; }

}  // namespace mfg

#define REQUIRE(cond, msg) \
  do {                     \
    if (!(cond)) return mfg::fail(MFG_EINVAL, "%s", msg); \
  } while (0)

#define CHECK_BD()                                        \
  REQUIRE(B >= 0, "B < 0");                               \
  REQUIRE(d >= 1, "d < 1");                               \
  if (d > MFG_MAX_D) return mfg::fail(MFG_EUNSUPPORTED, "%s: d=%lld > %lld", "shape", (long long)d, (long long)MFG_MAX_D); \
  if (B == 0) return MFG_OK;
