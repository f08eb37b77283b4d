// Host side of the MFG hot path for MI355X (gfx950 / CDNA4, wave64): the C ABI and what its entry points share.
// See include/mfg_hip.h for the contract and DESIGN.md for the layout / roofline notes.
//
// Here: the error record, the context registry and the status word, the h(z) table, the RCCL loader, launch_core and the
// training / evaluation drivers with their entry points.  The kernels live with their launch rules in translation units of
// their own: mfg_core_*.hip (fused rollout), mfg_step.hip (given-P step), mfg_batch_sums.hip (batch sums, critic values),
// mfg_launch_once.hip (elementwise and evaluation kernels), mfg_population*.hip / mfg_*_pop.hip (population forms),
// mfg_reward_*.hip (reward network).  mfg_host.h declares what those units use from this one.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <stdlib.h>

#include <dlfcn.h>

#include <atomic>
#include <mutex>
#include <unordered_map>

#include "../../include/mfg_hip.h"
#include "mfg_core.h"
#include "mfg_evaluate_pop.h"
#include "mfg_forecast_pop.h"
#include "mfg_agents.h"
#include "mfg_consistency_pop.h"
#include "mfg_irl_population.h"
#include "mfg_population.h"
#include "mfg_pop_evolve.h"
#include "mfg_reward_grad.h"
#include "mfg_pop_validate.h"
#include "mfg_batch_sums.h"
#include "mfg_host.h"
#include "mfg_launch_once.h"
#include "mfg_step.h"

using namespace mfg;

// ---------------------------------------------------------------------------------------------
// error plumbing (declared in mfg_host.h)
// ---------------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";

namespace mfg {
int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}
int set_error(int code, const char* msg) { return fail(code, "%s", msg); }
int check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(MFG_ELAUNCH, "%s: %s", what, hipGetErrorString(e));
  return MFG_OK;
}

// CU count of the CURRENT device (cached per device: one context may drive several GPUs from one process)
int num_cus() {
  static std::atomic<int> cus[64];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
  int c = cus[dev].load(std::memory_order_relaxed);
  if (!c) {
    hipDeviceProp_t p;
    c = (hipGetDeviceProperties(&p, dev) == hipSuccess && p.multiProcessorCount > 0) ? p.multiProcessorCount : 256;
    cus[dev].store(c, std::memory_order_relaxed);
  }
  return c;
}

int grid_for(int64_t work_items, int per_block, int blocks_per_cu) {
  int64_t g = (work_items + per_block - 1) / per_block;
  const int64_t cap = (int64_t)num_cus() * blocks_per_cu;
  if (g > cap) g = cap;
  if (g < 1) g = 1;
  return (int)g;
}
}  // namespace mfg

// ---- h(z) table (mfg_device.h): module-resident, fitted once per device in fp64 -------------------------
__device__ float4 g_htab[HTAB_N];

__global__ void k_init_htab(float4* __restrict__ tab) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= HTAB_N) return;
  double y[4];
  for (int q = 0; q < 4; ++q) {
    const double z = (double)HTAB_ZMIN + ((double)k + (double)q / 3.0) / (double)HTAB_PER_UNIT;
    double sp, sg;
    softplus_sigmoid(z, sp, sg);
    y[q] = digamma_pos(sp) * sg * INV_LN2;  // log2 units, see mfg_device.h
  }
  // cubic through f = 0, 1/3, 2/3, 1 (Newton forward differences, t = 3 f)
  const double d1 = y[1] - y[0], d2 = y[2] - 2.0 * y[1] + y[0], d3 = y[3] - 3.0 * y[2] + 3.0 * y[1] - y[0];
  tab[k] = make_float4((float)y[0], (float)(3.0 * (d1 - 0.5 * d2 + d3 / 3.0)), (float)(9.0 * (0.5 * d2 - 0.5 * d3)),
                       (float)(27.0 * d3 / 6.0));
}

// Device address of the table; the first call on a device fits it (one launch + one device sync, ever).
static const float4* htab_ptr() {
  static std::mutex mu;
  static const float4* ptr[64] = {nullptr};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return nullptr;
  std::lock_guard<std::mutex> lock(mu);
  if (!ptr[dev]) {
    void* p = nullptr;
    if (hipGetSymbolAddress(&p, HIP_SYMBOL(g_htab)) != hipSuccess) return nullptr;
    hipLaunchKernelGGL(k_init_htab, dim3((HTAB_N + 255) / 256), dim3(256), 0, 0, (float4*)p);
    if (hipDeviceSynchronize() != hipSuccess) return nullptr;
    ptr[dev] = (const float4*)p;
  }
  return ptr[dev];
}

// ---- device status word (mfg_status): one host-mapped 32-bit word per device.  Kernels OR condition bits into it through
// its device address (a plain store from one lane: the conditions are functions of theta alone, so every launch that sees
// the condition writes the same bits); the host reads it through the host address without synchronising.
struct StatusWord {
  unsigned* host = nullptr;
  unsigned* dev = nullptr;
};
// ---- contexts (mfg_ctx_t, include/mfg_hip.h): the mutable state a launch touches -- the status word, an RCCL communicator --
// owned by an opaque object instead of the process.  A thread binds a context (mfg_ctx_bind) and every entry point called
// from that thread acts on it; with none bound the device's default context (the process-wide word of ABI 14) is used.
struct mfg_ctx {
  int device = -1;
  StatusWord sw;
  void* comm = nullptr;  // adopted RCCL communicator (mfg_ctx_adopt_comm), destroyed with the context
  bool has_ctl = false;  // population control block (mfg_ctx_set_pop_control): the population training calls carry it
  mfg_pop_control_t ctl{};
  bool has_val = false;  // population validation block (mfg_ctx_set_pop_validate): held-out checks inside those calls
  mfg_pop_validate_t val{};
  bool has_evo = false;  // population evolve block (mfg_ctx_set_pop_evolve): exploit / explore steps behind those checks
  mfg_pop_evolve_t evo{};
  bool has_rig = false;  // reward input-gradient block (mfg_ctx_set_rn_input_grad): rides on mfg_reward_net_forward_pop
  mfg_rn_input_grad_t rig{};
};
// The binding is per THREAD, the object's lifetime is not: a context may be destroyed by another thread than the one(s) it is
// bound on (a garbage collector drops the last reference wherever it runs).  Every live context is therefore registered with
// a generation id, a thread's binding remembers (pointer, generation), and a destroy bumps a global epoch: the next entry
// point of a thread that finds the epoch moved re-validates its binding under the registry lock and, if its context is gone
// (or the address now belongs to a younger one), falls back to the device's default word instead of touching freed memory.
// The hot path (no destroy since the last look) is one relaxed-cost atomic load.
static thread_local mfg_ctx* g_ctx = nullptr;
static thread_local uint64_t g_ctx_gen = 0, g_ctx_seen_epoch = 0;
static std::mutex g_ctx_mu;
static std::unordered_map<mfg_ctx*, uint64_t> g_ctx_live;  // live contexts -> generation id (under g_ctx_mu)
static uint64_t g_ctx_next_gen = 1;                          // (under g_ctx_mu)
static std::atomic<uint64_t> g_ctx_epoch{1};                 // bumped by every mfg_ctx_destroy
static bool ctx_is_live(mfg_ctx* c) {
  std::lock_guard<std::mutex> lock(g_ctx_mu);
  return g_ctx_live.find(c) != g_ctx_live.end();
}
// the calling thread's bound context; NULL if none, or if it has been destroyed (by any thread) since it was bound
static mfg_ctx* bound_ctx() {
  if (!g_ctx) return nullptr;
  if (g_ctx_epoch.load(std::memory_order_acquire) != g_ctx_seen_epoch) {
    std::lock_guard<std::mutex> lock(g_ctx_mu);
    const auto it = g_ctx_live.find(g_ctx);
    if (it == g_ctx_live.end() || it->second != g_ctx_gen) g_ctx = nullptr;
    g_ctx_seen_epoch = g_ctx_epoch.load(std::memory_order_acquire);
  }
  return g_ctx;
}
extern "C" int mfg_dist_destroy(void* comm);
static bool alloc_status_word(StatusWord* out) {
  void* h = nullptr;
  void* d = nullptr;
  if (hipHostMalloc(&h, 64, hipHostMallocMapped) != hipSuccess) return false;
  memset(h, 0, 64);
  if (hipHostGetDevicePointer(&d, h, 0) != hipSuccess) {
    (void)hipHostFree(h);
    return false;
  }
  out->host = (unsigned*)h;
  out->dev = (unsigned*)d;
  return true;
}
static StatusWord status_word() {
  static std::mutex mu;
  static StatusWord sw[64];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return StatusWord{};
  if (mfg_ctx* c = bound_ctx()) return c->device == dev ? c->sw : StatusWord{};  // (a context of another device: refused by the callers)
  std::lock_guard<std::mutex> lock(mu);
  if (!sw[dev].host && !alloc_status_word(&sw[dev])) return StatusWord{};
  return sw[dev];
}
static int status_error(unsigned bits) {
  if (bits & MFG_STATUS_MIXED_RANGE)
    return fail(MFG_ERANGE, "%s", "an earlier mixed-precision launch ran with |theta| (1 + |shift|) > 86 (or theta not "
                                  "finite): the fp32 factors of the separable exponential left their range and that launch's "
                                  "outputs are NaN; use MFG_PRECISION_F64 / precision='f64' for such policies, then mfg_clear_status()");
  return fail(MFG_ERANGE, "device status word = 0x%x", bits);
}

// mfg_train_rollouts_dist: the sticky status word is read ONCE in front of the episode loop and once behind it, not per
// enqueue -- the host read races the device by a different number of episodes on every rank, and a rank that stops
// enqueueing leaves its peers' all-reduces without a partner (the private communicator has no watchdog).
static thread_local bool g_status_check_deferred = false;

// traj_offset + B <= 2^48: the id space of the Philox counter (MFG_TRAJ_ID_LIMIT, include/mfg_hip.h)
static bool traj_ids_ok(uint64_t traj_offset, int64_t B) {
  return traj_offset <= MFG_TRAJ_ID_LIMIT && (uint64_t)(B > 0 ? B : 0) <= MFG_TRAJ_ID_LIMIT - traj_offset;
}

// pop != NULL: the population form (mfg_population.h; d <= 64, packed lane mapping): sampling + TD the training kernel,
// sampling alone the evaluation kernel (mfg_evaluate_pop.h)
static int launch_core(const CoreArgs& a_in, bool sample, bool td, int precision, hipStream_t st, const PopArgs* pop = nullptr) {
  CoreArgs a = a_in;
  if (!traj_ids_ok(a.traj_offset, a.B))
    return fail(MFG_EINVAL, "trajectory ids traj_offset + B = %llu + %lld exceed 2^48 (MFG_TRAJ_ID_LIMIT)",
                (unsigned long long)a.traj_offset, (long long)a.B);
  {
    const StatusWord sw = status_word();
    if (!sw.host) return fail(MFG_ELAUNCH, "%s", "status word allocation failed");
    const unsigned bits = g_status_check_deferred ? 0u : *(volatile unsigned*)sw.host;
    // sticky until mfg_clear_status() -- for the launches the condition concerns: MFG_STATUS_MIXED_RANGE is a property of
    // mixed-precision SAMPLING (theta beyond the range of its fp32 factors); strict-precision launches and launches on given
    // actions have no such limit and go ahead whatever another instance / thread on this device ran into
    const unsigned blocking = (sample && precision == MFG_PRECISION_MIXED) ? bits : (bits & ~(unsigned)MFG_STATUS_MIXED_RANGE);
    if (blocking) return status_error(blocking);
    a.status = sw.dev;
  }
#ifdef MFG_TIMING
  {
    const char* e = getenv("MFG_TIMING_BUF");
    a.dbg = e ? (unsigned long long*)strtoull(e, nullptr, 16) : nullptr;
  }
#endif
  if (td && precision == MFG_PRECISION_MIXED) {
    a.htab = htab_ptr();
    if (!a.htab) return fail(MFG_ELAUNCH, "%s", "h(z) table initialisation failed");
  }
  int rc;
  if (pop) rc = !sample ? MFG_EUNSUPPORTED
                : td  ? launch_core_pop(a, *pop, precision == MFG_PRECISION_MIXED, num_cus(), st)
                      : launch_eval_rollout_pop(a, *pop, precision == MFG_PRECISION_MIXED, num_cus(), st);
  else if (a.d <= WAVE) rc = launch_core_small(a, sample, td, precision == MFG_PRECISION_MIXED, num_cus(), st);
  else if (precision == MFG_PRECISION_MIXED) rc = launch_core_large_mixed(a, sample, td, num_cus(), st);
  else rc = launch_core_large_f64(a, sample, td, num_cus(), st);
  if (rc != MFG_OK) return fail(rc, "%s: d=%lld > %lld", "core", (long long)a.d, (long long)MFG_MAX_D);
  return check_launch("core");
}

// Per-step updates at the packed sizes (T == 1, d = 21 / 15, in-kernel reward): the step kernel itself leaves one partial
// row of the batch sums per tile (k_core_small<..., SUMS>), so an update is [step kernel | row reduction (+ apply)]
// instead of [step kernel | gradient kernel with its own finish].  Used while every tile has its own resident block
// (MFG_CORE_SUMS_MAX_ROWS tiles = 6 144 trajectories at d = 21) and the workspace has room for the rows; otherwise the
// caller takes the two-kernel path.
constexpr int64_t MFG_CORE_SUMS_MAX_ROWS = 512;  // = blocks resident at the SUMS variant's two waves per SIMD (256 CUs x 2)
static int64_t core_sums_rows(int d, int64_t B) {
  if (!(d == 21 || d == 15)) return 0;
  const int TB = WAVES * (WAVE / d);
  const int64_t nt = (B + TB - 1) / TB;
  return nt <= MFG_CORE_SUMS_MAX_ROWS ? nt : 0;
}
static bool core_sums_ok(int d, int64_t B, int T, int reward_kind, const void* ws, size_t ws_bytes) {
  if (T != 1 || reward_kind == MFG_REWARD_EXTERNAL || !ws) return false;
  const int64_t nt = core_sums_rows(d, B);
  return nt > 0 && ws_bytes >= (size_t)(nt * (mfg_num_features(d) + 3) * 8) + MFG_WS_CONTROL_BYTES;
}
// the row reduction (+ optional parameter update) that follows a SUMS launch
static int reduce_core_sums(int d, int64_t B, double* G, int accumulate, void* ws, const ApplyArgs* apply, hipStream_t st,
                            const PopArgs* pop = nullptr) {
  const int64_t FO = mfg_num_features(d) + 3, nt = core_sums_rows(d, B);
  ReduceApply rap{};
  if (apply && !accumulate) {
    rap.on = 1;
    rap.lr_c = apply->lr_c;
    rap.lr_a = apply->lr_a;
    rap.count = (double)B;
    rap.w = apply->w;
    rap.theta = apply->theta;
    rap.reward_acc = apply->reward_acc;
  }
  if (pop) {
    if (accumulate) return fail(MFG_EUNSUPPORTED, "%s", "population: accumulated sums");
    launch_reduce_partials_pop((unsigned)((FO + RP_OUT - 1) / RP_OUT), (const double*)((char*)ws + MFG_WS_CONTROL_BYTES), nt, FO, G,
                               rap, *pop, st);
    return check_launch("core_sums_pop");
  }
  launch_reduce_partials((const double*)((char*)ws + MFG_WS_CONTROL_BYTES), nt, FO, accumulate, G, rap, st);
  return check_launch("core_sums");
}

// ---------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------
extern "C" {

const char* mfg_last_error(void) { return g_err; }
int mfg_abi_version(void) { return 18; }

int mfg_init(void) {
  if (!htab_ptr()) return fail(MFG_ELAUNCH, "%s", "mfg_init: no HIP device / table initialisation failed");
  if (!status_word().host) return fail(MFG_ELAUNCH, "%s", "mfg_init: status word allocation failed");
  return MFG_OK;
}

int mfg_set_core_mapping(int mode) { return core_mapping_set(mode); }

int mfg_status(unsigned* bits_host) {
  const StatusWord sw = status_word();
  if (!sw.host) return fail(MFG_ELAUNCH, "%s", "status word allocation failed");
  const unsigned bits = *(volatile unsigned*)sw.host;
  if (bits_host) *bits_host = bits;
  return bits ? status_error(bits) : MFG_OK;
}

int mfg_clear_status(void) {
  const StatusWord sw = status_word();
  if (!sw.host) return fail(MFG_ELAUNCH, "%s", "status word allocation failed");
  *(volatile unsigned*)sw.host = 0u;
  return MFG_OK;
}

int mfg_ctx_create(mfg_ctx_t** ctx_out) {
  REQUIRE(ctx_out, "null pointer");
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return fail(MFG_ELAUNCH, "%s", "mfg_ctx_create: no HIP device");
  if (!htab_ptr()) return fail(MFG_ELAUNCH, "%s", "mfg_ctx_create: table initialisation failed");  // (shared, immutable, per device)
  mfg_ctx* c = new (std::nothrow) mfg_ctx();
  if (!c) return fail(MFG_ELAUNCH, "%s", "mfg_ctx_create: out of memory");
  c->device = dev;
  if (!alloc_status_word(&c->sw)) {
    delete c;
    return fail(MFG_ELAUNCH, "%s", "mfg_ctx_create: status word allocation failed");
  }
  {
    std::lock_guard<std::mutex> lock(g_ctx_mu);
    g_ctx_live[c] = g_ctx_next_gen++;
  }
  *ctx_out = c;
  return MFG_OK;
}

int mfg_ctx_destroy(mfg_ctx_t* ctx) {
  if (!ctx) return MFG_OK;
  {
    // out of the registry first, then the epoch: a thread that still has it bound (this one or any other) drops the binding
    // at its next entry point (bound_ctx) instead of dereferencing the freed object
    std::lock_guard<std::mutex> lock(g_ctx_mu);
    if (g_ctx_live.erase(ctx) == 0) return fail(MFG_EINVAL, "%s", "mfg_ctx_destroy: not a live context (destroyed twice?)");
    g_ctx_epoch.fetch_add(1, std::memory_order_release);
  }
  if (g_ctx == ctx) g_ctx = nullptr;
  int rc = MFG_OK;
  if (ctx->comm) rc = mfg_dist_destroy(ctx->comm);
  if (ctx->sw.host) (void)hipHostFree(ctx->sw.host);
  delete ctx;
  return rc;
}

int mfg_ctx_bind(mfg_ctx_t* ctx) {
  uint64_t gen = 0, epoch = 0;
  if (ctx) {
    {
      std::lock_guard<std::mutex> lock(g_ctx_mu);
      const auto it = g_ctx_live.find(ctx);
      if (it == g_ctx_live.end()) return fail(MFG_EINVAL, "%s", "mfg_ctx_bind: not a live context (already destroyed?)");
      gen = it->second;
      epoch = g_ctx_epoch.load(std::memory_order_acquire);
    }
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev != ctx->device)
      return fail(MFG_EINVAL, "mfg_ctx_bind: the context belongs to device %d, the current device is %d", ctx->device, dev);
  }
  g_ctx = ctx;
  g_ctx_gen = gen;
  g_ctx_seen_epoch = epoch;
  return MFG_OK;
}

mfg_ctx_t* mfg_ctx_current(void) { return bound_ctx(); }

int mfg_ctx_status(mfg_ctx_t* ctx, unsigned* bits_host) {
  REQUIRE(ctx && ctx_is_live(ctx) && ctx->sw.host, "null or destroyed context");
  const unsigned bits = *(volatile unsigned*)ctx->sw.host;
  if (bits_host) *bits_host = bits;
  return bits ? status_error(bits) : MFG_OK;
}

int mfg_ctx_clear_status(mfg_ctx_t* ctx) {
  REQUIRE(ctx && ctx_is_live(ctx) && ctx->sw.host, "null or destroyed context");
  *(volatile unsigned*)ctx->sw.host = 0u;
  return MFG_OK;
}

int mfg_ctx_adopt_comm(mfg_ctx_t* ctx, void* comm) {
  REQUIRE(ctx && ctx_is_live(ctx), "null or destroyed context");
  ctx->comm = comm;
  return MFG_OK;
}

void* mfg_ctx_comm(mfg_ctx_t* ctx) { return (ctx && ctx_is_live(ctx)) ? ctx->comm : nullptr; }

static bool pop_control_complete(const mfg_pop_control_t& c) {
  return c.state && c.status && c.theta_prev && c.episodes_run && c.stop_criteria;
}

int mfg_ctx_set_pop_control(mfg_ctx_t* ctx, const mfg_pop_control_t* block) {
  REQUIRE(ctx && ctx_is_live(ctx), "null or destroyed context");
  if (!block) {
    ctx->has_ctl = false;
    ctx->ctl = mfg_pop_control_t{};
    return MFG_OK;
  }
  REQUIRE(pop_control_complete(*block), "population control block: null pointer");
  REQUIRE(block->K >= 1 && block->K <= MFG_POP_MAX_K, "population control block: K outside [1, MFG_POP_MAX_K]");
  ctx->ctl = *block;
  ctx->has_ctl = true;
  return MFG_OK;
}

static bool pop_validate_complete(const mfg_pop_validate_t& v) {
  return v.emp32 && v.emp64 && v.curve && v.checks && v.best_value && v.best_check && v.since_best && v.best_theta && v.best_w &&
         v.workspace;
}

int mfg_ctx_set_pop_validate(mfg_ctx_t* ctx, const mfg_pop_validate_t* block) {
  REQUIRE(ctx && ctx_is_live(ctx), "null or destroyed context");
  if (!block) {
    ctx->has_val = false;
    ctx->val = mfg_pop_validate_t{};
    return MFG_OK;
  }
  const mfg_pop_validate_t& v = *block;
  REQUIRE(pop_validate_complete(v), "population validation block: null pointer");
  REQUIRE((reinterpret_cast<uintptr_t>(v.workspace) & 7) == 0, "population validation block: workspace not 8-byte aligned");
  REQUIRE(v.K >= 1 && v.K <= MFG_POP_MAX_K, "population validation block: K outside [1, MFG_POP_MAX_K]");
  REQUIRE(v.period >= 1, "population validation block: period < 1");
  REQUIRE(v.max_checks >= 1, "population validation block: max_checks < 1");
  REQUIRE(v.patience >= 0, "population validation block: patience < 0");
  REQUIRE(v.with_score == 0 || v.with_score == 1, "population validation block: with_score is not 0 / 1");
  REQUIRE(v.column >= 0 && v.column < MFG_POP_VALIDATE_COLUMNS, "population validation block: column outside [0, 10)");
  REQUIRE(v.column < 8 || v.with_score, "population validation block: columns 8 / 9 (crps, energy) need with_score");
  REQUIRE(v.N >= 1, "population validation block: no held-out trajectories (N < 1)");
  REQUIRE(v.L >= 2, "population validation block: episode_length L < 2");
  REQUIRE(v.repeats >= 1, "population validation block: repeats < 1");
  REQUIRE(v.N * (int64_t)v.L <= 0x7FFFFFFF && v.N * (int64_t)v.repeats <= 0x7FFFFFFF,
          "population validation block: N L or N repeats too large");
  REQUIRE((uint64_t)v.first_step + (uint64_t)(v.L - 1) <= 0xFFFFFFFFull, "population validation block: Philox step counter would wrap");
  if (v.with_score && v.repeats > MFG_FORECAST_MAX_REPEATS)
    return fail(MFG_EUNSUPPORTED, "population validation block: repeats=%d > MFG_FORECAST_MAX_REPEATS=%d with with_score", v.repeats,
                MFG_FORECAST_MAX_REPEATS);
  ctx->val = v;
  ctx->has_val = true;
  return MFG_OK;
}

static bool pop_evolve_complete(const mfg_pop_evolve_t& e) {
  return e.lr_critic && e.lr_actor && e.order && e.active && e.rank && e.parent && e.lr_log;
}

int mfg_ctx_set_pop_evolve(mfg_ctx_t* ctx, const mfg_pop_evolve_t* block) {
  REQUIRE(ctx && ctx_is_live(ctx), "null or destroyed context");
  if (!block) {
    ctx->has_evo = false;
    ctx->evo = mfg_pop_evolve_t{};
    return MFG_OK;
  }
  const mfg_pop_evolve_t& e = *block;
  REQUIRE(pop_evolve_complete(e), "population evolve block: null pointer");
  REQUIRE(e.K >= 1 && e.K <= MFG_POP_MAX_K, "population evolve block: K outside [1, MFG_POP_MAX_K]");
  REQUIRE(e.every >= 1, "population evolve block: every < 1");
  REQUIRE(e.n_top >= 1 && e.n_bottom >= 1, "population evolve block: n_top < 1 or n_bottom < 1");
  REQUIRE((int64_t)e.n_top + (int64_t)e.n_bottom <= e.K, "population evolve block: n_top + n_bottom > K");
  REQUIRE(e.max_steps >= 1, "population evolve block: max_steps < 1");
  REQUIRE(std::isfinite(e.factor_down) && e.factor_down > 0.0 && std::isfinite(e.factor_up) && e.factor_up > 0.0,
          "population evolve block: a factor is not finite or <= 0");
  REQUIRE(std::isfinite(e.lr_critic_max) && e.lr_critic_min > 0.0 && e.lr_critic_min <= e.lr_critic_max,
          "population evolve block: lr_critic bounds need 0 < min <= max, finite");
  REQUIRE(std::isfinite(e.lr_actor_max) && e.lr_actor_min > 0.0 && e.lr_actor_min <= e.lr_actor_max,
          "population evolve block: lr_actor bounds need 0 < min <= max, finite");
  REQUIRE(e.perturb >= 0 && e.perturb <= 3, "population evolve block: perturb outside [0, 3]");
  ctx->evo = e;
  ctx->has_evo = true;
  return MFG_OK;
}

int mfg_ctx_set_rn_input_grad(mfg_ctx_t* ctx, const mfg_rn_input_grad_t* block) {
  REQUIRE(ctx && ctx_is_live(ctx), "null or destroyed context");
  if (!block) {
    ctx->has_rig = false;
    ctx->rig = mfg_rn_input_grad_t{};
    return MFG_OK;
  }
  const mfg_rn_input_grad_t& b = *block;
  REQUIRE(b.grad_state || b.grad_action || b.mean_state || b.mean_action, "reward input-gradient block: all four outputs are NULL");
  REQUIRE(b.K >= 1 && b.K <= MFG_POP_MAX_K, "reward input-gradient block: K outside [1, MFG_POP_MAX_K]");
  REQUIRE(b.N >= 1, "reward input-gradient block: no samples (N < 1)");
  REQUIRE((reinterpret_cast<uintptr_t>(b.workspace) & 7) == 0, "reward input-gradient block: workspace not 8-byte aligned");
  ctx->rig = b;
  ctx->has_rig = true;
  return MFG_OK;
}

int mfg_device_info(int* cu_count_host, char* arch_host, int arch_len) {
  int dev = 0;
  hipDeviceProp_t p;
  if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&p, dev) != hipSuccess)
    return fail(MFG_ELAUNCH, "%s", "no HIP device");
  if (cu_count_host) *cu_count_host = p.multiProcessorCount;
  if (arch_host && arch_len > 0) {
    strncpy(arch_host, p.gcnArchName, (size_t)arch_len - 1);
    arch_host[arch_len - 1] = 0;
  }
  return MFG_OK;
}

int64_t mfg_num_features(int d) { return (int64_t)d * (d + 1) / 2 + d + 1; }

int64_t mfg_feature_index(int i, int j, int d) {
  if (i > j) {
    const int t = i;
    i = j;
    j = t;
  }
  return (int64_t)i * d - ((int64_t)i * (i - 1)) / 2 + (j - i);
}

size_t mfg_workspace_bytes(int64_t N, int d) {
  if (N < 1 || d < 1) return 0;
  int chunk, nob;
  int64_t nsb;
  grad_geometry(N, d, &chunk, &nsb, &nob);
  const int64_t rows_sums = core_sums_rows(d, N);  // T = 1 updates with the sums fused into the step kernel: a row per tile
  if (rows_sums > nsb) nsb = rows_sums;
  if (d <= 32) {  // IRL steps with the sums fused into the reward-network launch: a row per block of eight samples, <= 512
    const int64_t rows_rn = (N + 7) / 8 < 512 ? (N + 7) / 8 : 512;
    if (rows_rn > nsb) nsb = rows_rn;
  }
  return (size_t)(nsb * (mfg_num_features(d) + 3) * 8) + MFG_WS_CONTROL_BYTES + value_buffer_bytes(N, d);
}

int mfg_draw_start(const float* mat_pi0, int64_t num_start, int64_t B, int d, uint64_t seed, uint32_t step, uint64_t traj_offset,
                   int32_t* idx, float* pi0, mfg_stream_t stream) {
  CHECK_BD();
  REQUIRE(num_start > 0 && num_start <= 0x7FFFFFFF, "empty / oversized start-state table");
  REQUIRE(idx || pi0, "nothing to write");
  REQUIRE(!pi0 || mat_pi0, "null start-state table");
  REQUIRE(traj_ids_ok(traj_offset, B), "trajectory ids traj_offset + B exceed 2^48 (MFG_TRAJ_ID_LIMIT)");
  launch_draw_start(mat_pi0, num_start, B, d, seed, step, traj_offset, idx, pi0, S(stream));
  return check_launch("draw_start");
}

int mfg_step_given_P(const float* pi, const float* P, int64_t B, int d, int reward_kind, float* pi_next, float* reward,
                     mfg_stream_t stream) {
  CHECK_BD();
  REQUIRE(pi && P && pi_next, "null pointer");
  REQUIRE(reward_kind >= 0 && reward_kind <= 2, "bad reward_kind");
  if (!reward) reward_kind = MFG_REWARD_EXTERNAL;
  return launch_step_given_P(pi, P, B, d, reward_kind, pi_next, reward, S(stream));
}

#define CHECK_PRECISION() REQUIRE(precision == MFG_PRECISION_F64 || precision == MFG_PRECISION_MIXED, "bad precision")

int mfg_sample_dirichlet(const float* pi, int64_t B, int d, const double* theta, double shift, double alpha_scale,
                         uint64_t seed, uint32_t step, uint64_t traj_offset, int precision, float* P,
                         mfg_stream_t stream) {
  CHECK_BD();
  CHECK_PRECISION();
  REQUIRE(pi && theta && P, "null pointer");
  CoreArgs a{};
  a.pi0 = pi;
  a.theta = theta;
  a.shift = shift;
  a.alpha_scale = alpha_scale;
  a.gamma = 1.0;
  a.B = B;
  a.d = d;
  a.T = 1;
  a.reward_kind = MFG_REWARD_EXTERNAL;
  a.seed = seed;
  a.first_step = step;
  a.traj_offset = traj_offset;
  a.P_out = P;
  return launch_core(a, true, false, precision, S(stream));
}

int mfg_score(const float* pi_alpha, const float* P, int64_t B, int d, const double* theta, double shift,
              int precision, double* g, mfg_stream_t stream) {
  CHECK_BD();
  CHECK_PRECISION();
  REQUIRE(pi_alpha && P && theta && g, "null pointer");
  CoreArgs a{};
  a.pi0 = pi_alpha;
  a.P_in = P;
  a.theta = theta;
  a.shift = shift;
  a.gamma = 1.0;
  a.B = B;
  a.d = d;
  a.T = 1;
  a.reward_kind = MFG_REWARD_EXTERNAL;
  a.g = g;
  return launch_core(a, false, true, precision, S(stream));
}

int mfg_td_pg_accumulate(const float* pi, const float* pi_next, const float* P, const float* reward, const double* w,
                         const double* theta, double shift, double gamma_or_discount, int64_t B, int d, int precision,
                         double* delta, double* g, double* G, int accumulate, void* workspace,
                         size_t workspace_bytes, mfg_stream_t stream) {
  CHECK_BD();
  CHECK_PRECISION();
  REQUIRE(pi && pi_next && P && reward && w && theta && delta && g, "null pointer");
  CoreArgs a{};
  a.pi0 = pi;
  a.P_in = P;
  a.pi_next_in = pi_next;
  a.reward_in = reward;
  a.theta = theta;
  a.w = w;
  a.shift = shift;
  a.gamma = gamma_or_discount;
  a.B = B;
  a.d = d;
  a.T = 1;
  a.reward_kind = MFG_REWARD_EXTERNAL;
  a.delta = delta;
  a.g = g;
  int rc = launch_core(a, false, true, precision, S(stream));
  if (rc != MFG_OK || !G) return rc;
  REQUIRE(workspace, "workspace is null");
  return launch_grad(pi, d, delta, g, reward, B, 1, d, G, accumulate, workspace, workspace_bytes, S(stream));
}

int mfg_apply_update(const double* G, int d, double lr_critic, double lr_actor, double* w, double* theta,
                     double* reward_acc, mfg_stream_t stream) {
  REQUIRE(G && w && theta && d >= 1, "null pointer");
  launch_apply_update(G, d, lr_critic, lr_actor, w, theta, reward_acc, S(stream));
  return check_launch("apply_update");
}

// whether a TD rollout can defer its values to k_value_mfma
static bool defer_values(int d, int64_t B, int T, const float* pi_traj, const void* ws, size_t ws_bytes) {
  if (!value_batch_ok(d) || !pi_traj || !ws || (((uintptr_t)pi_traj & 15) != 0)) return false;
  return ws_bytes >= mfg_workspace_bytes(B * T, d);
}

int mfg_rollout(const float* pi0, int64_t B, int d, int T, const double* theta, double shift, double alpha_scale,
                const double* w, double gamma, int reward_kind, uint64_t seed, uint32_t first_step, uint64_t traj_offset,
                int flags, float* pi_traj, float* pi_last, float* reward, double* delta, double* g, float* P_out,
                double* G, int accumulate, void* workspace, size_t workspace_bytes, mfg_stream_t stream) {
  CHECK_BD();
  REQUIRE(T >= 1, "T < 1");
  REQUIRE(pi0 && theta, "null pointer");
  REQUIRE(reward_kind >= 0 && reward_kind <= 2, "bad reward_kind");
  const bool td = (flags & MFG_ROLLOUT_TD) != 0;
  const bool ext = reward_kind == MFG_REWARD_EXTERNAL;
  REQUIRE(!(flags & MFG_ROLLOUT_WRITE_P) || P_out, "WRITE_P without P_out");
  REQUIRE(!td || (w && delta && g && pi_traj && (reward || ext)), "TD rollout needs w, delta, g, reward, pi_traj");
  REQUIRE(!(ext && td && G), "external reward: the batch sums need the reward, call mfg_grad_accumulate afterwards");
  if (ext) reward = nullptr;
  CoreArgs a{};
  a.pi0 = pi0;
  a.theta = theta;
  a.w = td ? w : nullptr;
  a.shift = shift;
  a.alpha_scale = alpha_scale;
  a.gamma = gamma;
  a.B = B;
  a.d = d;
  a.T = T;
  a.reward_kind = reward_kind;
  a.discount_pow = (flags & MFG_ROLLOUT_DISCOUNT_POW) ? 1 : 0;
  a.seed = seed;
  a.first_step = first_step;
  a.traj_offset = traj_offset;
  a.pi_traj = pi_traj;
  a.pi_next_out = pi_last;
  a.reward_out = reward;
  a.delta = delta;
  a.g = g;
  a.P_out = (flags & MFG_ROLLOUT_WRITE_P) ? P_out : nullptr;
  const int precision = (flags & MFG_ROLLOUT_F64) ? MFG_PRECISION_F64 : MFG_PRECISION_MIXED;
  const bool deferred = td && defer_values(d, B, T, pi_traj, workspace, workspace_bytes);
  if (deferred) a.w = nullptr;  // the kernel then leaves delta alone; values + delta follow on the matrix cores
  const bool sums_in_core = td && G && core_sums_ok(d, B, T, reward_kind, workspace, workspace_bytes);
  if (sums_in_core) a.part_rows = reinterpret_cast<double*>((char*)workspace + MFG_WS_CONTROL_BYTES);
  int rc = launch_core(a, true, td, precision, S(stream));
  if (rc != MFG_OK || !td) return rc;
  if (sums_in_core) return reduce_core_sums(d, B, G, accumulate, workspace, nullptr, S(stream));
  if (deferred) {
    rc = launch_values_and_delta(pi_traj, B, T, d, w, reward, gamma, a.discount_pow, delta, workspace, workspace_bytes, S(stream));
    if (rc != MFG_OK) return rc;
  }
  if (!G) return rc;
  REQUIRE(workspace, "workspace is null");
  return launch_grad(pi_traj, (int64_t)(T + 1) * d, delta, g, reward, B * T, T, d, G, accumulate, workspace,
                     workspace_bytes, S(stream));
}

// learning-rate multipliers of the reference schedule in episode number `episode` (mfg_ac2.py:511-522: 1/(episode+1) and
// 1/((episode+1) ln ln(episode+20)); ac_irl.py:697-708 with its 1-indexed episode); 1, 1 when `constant`.  The same
// double arithmetic as parallel.lr_scales of the host classes (libm log), so native and per-episode runs agree bit for bit.
static void lr_schedule(int64_t episode, int constant, double* sc, double* sa) {
  if (constant) {
    *sc = 1.0;
    *sa = 1.0;
    return;
  }
  const double e1 = (double)(episode + 1);
  *sc = 1.0 / e1;
  *sa = 1.0 / (e1 * log(log((double)(episode + 20))));
}

// the previous update of a multi-rank job, all-reduced but not applied yet (mfg_train_rollout_deferred)
struct DeferredUpdate {
  const double* G;
  double lr_c, lr_a;
  double* reward_acc;
  double *theta_out, *w_out;
};

// the external reward of an IRL rollout (reward_kind = MFG_REWARD_EXTERNAL): the core launch also writes the actions P and
// leaves delta = discount V(pi') - V(pi); ONE reward-network pass over all B T transitions follows, the states read in place
// from pi_traj (rows b (T+1) + t), and the reward joins delta in the gradient kernel
struct ExtReward {
  const mfg_reward_net_t* net;
  float* P;
  uint64_t key, sample_offset;  // dropout: Philox key (population: per learner, from `pop`) and first sample counter
  const RnPop* pop;
};

// one training update per episode: [rollout kernel (start rows: drawn in the kernel when idx == NULL, else gathered) |
// reward network (ext) | values + delta (large d) | batch sums | row reduction (+ update)]
static int train_rollout_impl(const float* mat_pi0, int64_t num_start, const int32_t* idx, int64_t B, int d, int T, double* theta,
                              double shift, double alpha_scale, double* w, double gamma, int reward_kind, uint64_t seed,
                              uint32_t first_step, uint64_t traj_offset, int flags, double lr_critic, double lr_actor,
                              float* pi_traj, float* pi_last, float* reward, double* delta, double* g, double* G,
                              double* reward_acc, void* workspace, size_t workspace_bytes, hipStream_t st,
                              const DeferredUpdate* du = nullptr, const PopArgs* pop = nullptr, const ExtReward* ext = nullptr) {
  REQUIRE(!du || !ext, "deferred update: needs an in-kernel reward");
  CoreArgs a{};
  if (du) {
    if (d <= WAVE) {
      // packed kernel: the update rides in the weight staging of this rollout
      a.pend_G = du->G;
      a.pend_lr_c = du->lr_c;
      a.pend_lr_a = du->lr_a;
      a.pend_reward_acc = du->reward_acc;
      a.theta_out = du->theta_out;
      a.w_out = du->w_out;
    } else {
      // wave-per-trajectory kernels read the weights from memory throughout: apply the update out of place first
      launch_apply_update_oop(du->G, d, du->lr_c, du->lr_a, w, theta, du->w_out, du->theta_out, du->reward_acc, st);
      theta = du->theta_out;
      w = du->w_out;
    }
  }
  a.pi0 = mat_pi0;
  a.start_idx = idx;
  a.start_draw = idx ? 0 : 1;
  a.num_start = num_start;
  a.theta = theta;
  a.w = w;
  a.shift = shift;
  a.alpha_scale = alpha_scale;
  a.gamma = gamma;
  a.B = B;
  a.d = d;
  a.T = T;
  a.reward_kind = reward_kind;
  a.discount_pow = (flags & MFG_ROLLOUT_DISCOUNT_POW) ? 1 : 0;
  a.seed = seed;
  a.first_step = first_step;
  a.traj_offset = traj_offset;
  a.pi_traj = pi_traj;
  a.pi_next_out = pi_last;
  a.reward_out = ext ? nullptr : reward;
  a.delta = delta;
  a.g = g;
  a.P_out = ext ? ext->P : nullptr;
  const int precision = (flags & MFG_ROLLOUT_F64) ? MFG_PRECISION_F64 : MFG_PRECISION_MIXED;
  const bool deferred = defer_values(d, B, T, pi_traj, workspace, workspace_bytes);
  if (deferred && pop) return fail(MFG_EUNSUPPORTED, "%s", "population: d > 64");
  if (deferred) a.w = nullptr;
  int rc = launch_core(a, true, true, precision, st, pop);
  if (rc != MFG_OK) return rc;
  if (ext) {
    rc = reward_net_forward_sums(pi_traj, ext->P, B * (int64_t)T, d, *ext->net, ext->key, ext->sample_offset, reward, nullptr,
                                 nullptr, st, T, ext->pop);
    if (rc != MFG_OK) return rc;
  }
  if (deferred) {
    rc = launch_values_and_delta(pi_traj, B, T, d, w, ext ? nullptr : reward, gamma, a.discount_pow, delta, workspace,
                                 workspace_bytes, st);
    if (rc != MFG_OK) return rc;
  }
  const ApplyArgs ap{lr_critic, lr_actor, w, theta, reward_acc};
  const bool want_apply = (flags & MFG_TRAIN_APPLY) != 0;
  bool applied = false;
  rc = launch_grad(pi_traj, (int64_t)(T + 1) * d, delta, g, reward, B * T, T, d, G, 0, workspace, workspace_bytes, st,
                   want_apply ? &ap : nullptr, &applied, ext != nullptr, pop);
  if (rc != MFG_OK) return rc;
  if (pop && want_apply && !applied) return fail(MFG_ELAUNCH, "%s", "population: update not applied");  // (not reached: d <= 64)
  if (want_apply && !applied) launch_apply_update(G, d, lr_critic, lr_actor, w, theta, reward_acc, st);
  return check_launch("train_rollout");
}

#define CHECK_TRAIN_ROLLOUT()                                                                                        \
  CHECK_BD();                                                                                                        \
  REQUIRE(T >= 1, "T < 1");                                                                                          \
  REQUIRE(mat_pi0 && num_start > 0 && num_start <= 0x7FFFFFFF, "null / empty / oversized start-state table");        \
  REQUIRE(theta && w && pi_traj && reward && delta && g && G && workspace, "null pointer");                          \
  REQUIRE(reward_kind == MFG_REWARD_MFG_AC2 || reward_kind == MFG_REWARD_SYNTHETIC, "needs an in-kernel reward")

int mfg_train_rollout(const float* mat_pi0, int64_t num_start, const int32_t* idx, int64_t B, int d, int T, double* theta,
                      double shift, double alpha_scale, double* w, double gamma, int reward_kind, uint64_t seed,
                      uint32_t first_step, uint64_t traj_offset, int flags, double lr_critic, double lr_actor,
                      float* pi_traj, float* pi_last, float* reward, double* delta, double* g, double* G,
                      double* reward_acc, void* workspace, size_t workspace_bytes, mfg_stream_t stream) {
  CHECK_TRAIN_ROLLOUT();
  return train_rollout_impl(mat_pi0, num_start, idx, B, d, T, theta, shift, alpha_scale, w, gamma, reward_kind, seed, first_step,
                            traj_offset, flags, lr_critic, lr_actor, pi_traj, pi_last, reward, delta, g, G, reward_acc, workspace,
                            workspace_bytes, S(stream));
}

int mfg_train_rollouts(const float* mat_pi0, int64_t num_start, int64_t B, int d, int T, int64_t episodes, int64_t first_episode,
                       int constant, double* theta, double shift, double alpha_scale, double* w, double gamma, int reward_kind,
                       uint64_t seed, uint32_t first_step, uint64_t traj_offset, int flags, double lr_critic, double lr_actor,
                       float* pi_traj, float* pi_last, float* reward, double* delta, double* g, double* G, double* reward_acc,
                       void* workspace, size_t workspace_bytes, mfg_stream_t stream) {
  CHECK_TRAIN_ROLLOUT();
  REQUIRE(episodes >= 0 && first_episode >= 0, "bad episode range");
  REQUIRE((uint64_t)first_step + (uint64_t)episodes * (uint64_t)T <= 0xFFFFFFFFull, "Philox step counter would wrap");
  for (int64_t k = 0; k < episodes; ++k) {
    double sc, sa;
    lr_schedule(first_episode + k, constant, &sc, &sa);
    const int rc = train_rollout_impl(mat_pi0, num_start, nullptr, B, d, T, theta, shift, alpha_scale, w, gamma, reward_kind, seed,
                                      first_step + (uint32_t)(k * T), traj_offset, flags | MFG_TRAIN_APPLY, lr_critic * sc,
                                      lr_actor * sa, pi_traj, pi_last, reward, delta, g, G, reward_acc ? reward_acc + k : nullptr,
                                      workspace, workspace_bytes, S(stream));
    if (rc != MFG_OK) return rc;
  }
  return MFG_OK;
}

int mfg_train_rollout_deferred(const float* mat_pi0, int64_t num_start, const int32_t* idx, int64_t B, int d, int T,
                               const double* theta, const double* w, const double* G_pending, double lr_critic_pending,
                               double lr_actor_pending, double* reward_acc_pending, double* theta_out, double* w_out, double shift,
                               double alpha_scale, double gamma, int reward_kind, uint64_t seed, uint32_t first_step,
                               uint64_t traj_offset, int flags, float* pi_traj, float* pi_last, float* reward, double* delta,
                               double* g, double* G, void* workspace, size_t workspace_bytes, mfg_stream_t stream) {
  CHECK_TRAIN_ROLLOUT();
  REQUIRE(!(flags & MFG_TRAIN_APPLY), "deferred update: MFG_TRAIN_APPLY makes no sense here");
  REQUIRE(!G_pending || (theta_out && w_out && theta_out != theta && w_out != w), "pending update needs separate output parameters");
  const DeferredUpdate du{G_pending, lr_critic_pending, lr_actor_pending, reward_acc_pending, theta_out, w_out};
  return train_rollout_impl(mat_pi0, num_start, idx, B, d, T, const_cast<double*>(theta), shift, alpha_scale, const_cast<double*>(w),
                            gamma, reward_kind, seed, first_step, traj_offset, flags, 0.0, 0.0, pi_traj, pi_last, reward, delta, g,
                            G, nullptr, workspace, workspace_bytes, S(stream), G_pending ? &du : nullptr);
}

// ---------------------------------------------------------------------------------------------
// Multi-GPU episode loop, native: RCCL called from this library (one all-reduce of G per update).
// The RCCL entry points are resolved at run time from the librccl.so the process already holds (PyTorch's, so that one RCCL
// instance serves the job); the library has no link-time dependency on it and reports MFG_EUNSUPPORTED where it is absent.
// ---------------------------------------------------------------------------------------------
}  // extern "C" (the helpers below have C++ linkage)
namespace mfg {
// (mfg_reward_grad.h) the reward input-gradient block mfg_reward_net_forward_pop runs under: that of the bound context
const mfg_rn_input_grad_t* bound_rn_input_grad() {
  const mfg_ctx* c = bound_ctx();
  return (c && c->has_rig) ? &c->rig : nullptr;
}
}  // namespace mfg
namespace {
struct RcclApi {
  int (*GetUniqueId)(void*) = nullptr;
  int (*CommInitRank)(void**, int, mfg_rccl_id_t, int) = nullptr;   // ncclUniqueId is passed BY VALUE (128 bytes)
  int (*CommDestroy)(void*) = nullptr;
  int (*CommAbort)(void*) = nullptr;
  int (*AllReduce)(const void*, void*, size_t, int, int, void*, hipStream_t) = nullptr;
  const char* (*GetErrorString)(int) = nullptr;
  bool ok = false;
};
const RcclApi& rccl() {
  static RcclApi api = [] {
    RcclApi a;
    void* h = dlopen("librccl.so", RTLD_NOW | RTLD_NOLOAD);          // already in the process (torch)?
    if (!h) h = dlopen("librccl.so.1", RTLD_NOW | RTLD_NOLOAD);
    if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);        // a stand-alone host program: load the system's
    if (!h) h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!h) return a;
    a.GetUniqueId = reinterpret_cast<int (*)(void*)>(dlsym(h, "ncclGetUniqueId"));
    a.CommInitRank = reinterpret_cast<int (*)(void**, int, mfg_rccl_id_t, int)>(dlsym(h, "ncclCommInitRank"));
    a.CommDestroy = reinterpret_cast<int (*)(void*)>(dlsym(h, "ncclCommDestroy"));
    a.CommAbort = reinterpret_cast<int (*)(void*)>(dlsym(h, "ncclCommAbort"));
    a.AllReduce = reinterpret_cast<int (*)(const void*, void*, size_t, int, int, void*, hipStream_t)>(dlsym(h, "ncclAllReduce"));
    a.GetErrorString = reinterpret_cast<const char* (*)(int)>(dlsym(h, "ncclGetErrorString"));
    a.ok = a.GetUniqueId && a.CommInitRank && a.CommDestroy && a.AllReduce;
    return a;
  }();
  return api;
}
// the entry points, or NULL with the refusal recorded (MFG_EUNSUPPORTED)
const RcclApi* rccl_or_fail() {
  const RcclApi& r = rccl();
  if (!r.ok) (void)fail(MFG_EUNSUPPORTED, "%s", "librccl.so is not available in this process");
  return r.ok ? &r : nullptr;
}
int rccl_fail(const char* what, int rc) {
  const RcclApi& r = rccl();
  return fail(MFG_ELAUNCH, "%s: RCCL error %d (%s)", what, rc, r.GetErrorString ? r.GetErrorString(rc) : "?");
}
constexpr int RCCL_SUM = 0, RCCL_FLOAT64 = 8;  // ncclSum, ncclFloat64 (rccl.h)
}  // namespace
extern "C" {

int mfg_dist_available(void) { return rccl().ok ? 1 : 0; }

int mfg_dist_unique_id(mfg_rccl_id_t* id_host) {
  REQUIRE(id_host, "null pointer");
  const RcclApi* r = rccl_or_fail();
  if (!r) return MFG_EUNSUPPORTED;
  const int rc = r->GetUniqueId(id_host);
  return rc == 0 ? MFG_OK : rccl_fail("ncclGetUniqueId", rc);
}

int mfg_dist_init(const mfg_rccl_id_t* id_host, int nranks, int rank, void** comm_out) {
  REQUIRE(id_host && comm_out && nranks >= 1 && rank >= 0 && rank < nranks, "bad arguments");
  const RcclApi* r = rccl_or_fail();
  if (!r) return MFG_EUNSUPPORTED;
  void* comm = nullptr;
  const int rc = r->CommInitRank(&comm, nranks, *id_host, rank);   // collective: every rank of the job calls it (current device)
  if (rc != 0) return rccl_fail("ncclCommInitRank", rc);
  *comm_out = comm;
  return MFG_OK;
}

int mfg_dist_destroy(void* comm) {
  if (!comm) return MFG_OK;
  const RcclApi* r = rccl_or_fail();
  if (!r) return MFG_EUNSUPPORTED;
  const int rc = r->CommDestroy(comm);
  return rc == 0 ? MFG_OK : rccl_fail("ncclCommDestroy", rc);
}

int mfg_dist_abort(void* comm) {
  if (!comm) return MFG_OK;
  const RcclApi& r = rccl();
  if (!r.ok || !r.CommAbort) return fail(MFG_EUNSUPPORTED, "%s", "ncclCommAbort is not available in this process");
  const int rc = r.CommAbort(comm);
  return rc == 0 ? MFG_OK : rccl_fail("ncclCommAbort", rc);
}

int mfg_dist_all_reduce(void* comm, double* G, int64_t n, mfg_stream_t stream) {
  REQUIRE(comm && G && n >= 1, "bad arguments");
  const RcclApi* r = rccl_or_fail();
  if (!r) return MFG_EUNSUPPORTED;
  const int rc = r->AllReduce(G, G, (size_t)n, RCCL_FLOAT64, RCCL_SUM, comm, S(stream));
  return rc == 0 ? MFG_OK : rccl_fail("ncclAllReduce", rc);
}

int mfg_train_rollouts_dist(void* comm, const float* mat_pi0, int64_t num_start, int64_t B, int d, int T, int64_t episodes,
                            int64_t first_episode, int constant, double* theta, double* w, double* theta_alt, double* w_alt,
                            double shift, double alpha_scale, double gamma, int reward_kind, uint64_t seed, uint32_t first_step,
                            uint64_t traj_offset, int flags, double lr_critic, double lr_actor, float* pi_traj, float* pi_last,
                            float* reward, double* delta, double* g, double* G, double* reward_acc, void* workspace,
                            size_t workspace_bytes, mfg_stream_t stream) {
  CHECK_TRAIN_ROLLOUT();
  REQUIRE(comm && theta_alt && w_alt && theta_alt != theta && w_alt != w, "needs a communicator and a second parameter set");
  REQUIRE(episodes >= 0 && first_episode >= 0, "bad episode range");
  REQUIRE(!(flags & MFG_TRAIN_APPLY), "MFG_TRAIN_APPLY makes no sense here");
  REQUIRE((uint64_t)first_step + (uint64_t)episodes * (uint64_t)T <= 0xFFFFFFFFull, "Philox step counter would wrap");
  const RcclApi* r = rccl_or_fail();
  if (!r) return MFG_EUNSUPPORTED;
  if (episodes == 0) return MFG_OK;
  const int64_t F = mfg_num_features(d);
  hipStream_t st = S(stream);
  // Every rank must enqueue the SAME number of all-reduces.  The sticky status word is therefore examined here, before the
  // first enqueue (a condition raised by an earlier call: every rank that shares the history refuses alike), and again
  // behind the loop; inside the loop launches go ahead whatever the device reports meanwhile (the outputs of a launch in the
  // reported condition are NaN on every rank alike, theta is replicated).  A rank-local failure inside the loop (a launch
  // error) aborts the communicator, so the peers' pending collectives fail instead of waiting for this rank for ever.
  {
    const bool mixed = !(flags & MFG_ROLLOUT_F64);
    unsigned bits = 0;
    if (mfg_status(&bits) != MFG_OK && mixed && (bits & MFG_STATUS_MIXED_RANGE)) return MFG_ERANGE;
  }
  struct DeferGuard {
    DeferGuard() { g_status_check_deferred = true; }
    ~DeferGuard() { g_status_check_deferred = false; }
  } defer_guard;
  double *tc = theta, *wc = w, *tn = theta_alt, *wn = w_alt;   // current / next parameter set
  double plc = 0.0, pla = 0.0;
  double* pacc = nullptr;
  bool pending = false;
  for (int64_t k = 0; k < episodes; ++k) {
    const DeferredUpdate du{G, plc, pla, pacc, tn, wn};
    int rc = train_rollout_impl(mat_pi0, num_start, nullptr, B, d, T, tc, shift, alpha_scale, wc, gamma, reward_kind, seed,
                                first_step + (uint32_t)(k * T), traj_offset, flags, 0.0, 0.0, pi_traj, pi_last, reward, delta, g, G,
                                nullptr, workspace, workspace_bytes, st, pending ? &du : nullptr);
    if (rc != MFG_OK) {
      // (the communicator is dead afterwards: MFG_ECOMM tells the caller to forget the handle; mfg_last_error keeps the cause)
      if (r->CommAbort) {
        (void)r->CommAbort(comm);
        return MFG_ECOMM;
      }
      return rc;
    }
    if (pending) {  // the rollout left the updated parameters in the other set
      double* t = tc; tc = tn; tn = t;
      t = wc; wc = wn; wn = t;
    }
    rc = r->AllReduce(G, G, (size_t)(F + 3), RCCL_FLOAT64, RCCL_SUM, comm, st);   // the ONE exchange of the update
    if (rc != 0) {
      (void)rccl_fail("ncclAllReduce", rc);
      if (r->CommAbort) {
        (void)r->CommAbort(comm);
        return MFG_ECOMM;
      }
      return MFG_ELAUNCH;
    }
    double sc, sa;
    lr_schedule(first_episode + k, constant, &sc, &sa);
    plc = lr_critic * sc;
    pla = lr_actor * sa;
    pacc = reward_acc ? reward_acc + k : nullptr;
    pending = true;
  }
  // the last update, and the parameters back in the caller's primary set
  launch_apply_update(G, d, plc, pla, wc, tc, pacc, st);
  if (tc != theta) {
    if (hipMemcpyAsync(theta, tc, sizeof(double), hipMemcpyDeviceToDevice, st) != hipSuccess ||
        hipMemcpyAsync(w, wc, (size_t)F * sizeof(double), hipMemcpyDeviceToDevice, st) != hipSuccess)
      return fail(MFG_ELAUNCH, "%s", "train_rollouts_dist: parameter copy failed");
  }
  const int lrc = check_launch("train_rollouts_dist");
  if (lrc != MFG_OK) return lrc;
  if (!(flags & MFG_ROLLOUT_F64)) {   // what the device has reported so far (everything is enqueued: symmetric by construction)
    unsigned bits = 0;
    if (mfg_status(&bits) != MFG_OK && (bits & MFG_STATUS_MIXED_RANGE)) return MFG_ERANGE;
  }
  return MFG_OK;
}

int mfg_grad_accumulate(const float* pi, int64_t stride_b, double* delta, const double* g, const float* reward, int64_t B,
                        int T, int d, int add_reward, double* G, int accumulate, void* workspace, size_t workspace_bytes,
                        mfg_stream_t stream) {
  CHECK_BD();
  REQUIRE(T >= 1 && stride_b >= (int64_t)T * d, "bad T / stride_b");
  REQUIRE(pi && delta && G && workspace, "null pointer");
  REQUIRE(!add_reward || reward, "add_reward without reward");
  return launch_grad(pi, stride_b, delta, g, reward, B * T, T, d, G, accumulate, workspace, workspace_bytes, S(stream),
                     nullptr, nullptr, add_reward != 0);
}

int mfg_grad_apply(const float* pi, int64_t stride_b, double* delta, const double* g, const float* reward, int64_t B, int T,
                   int d, int add_reward, double* G, double lr_critic, double lr_actor, double* w, double* theta,
                   double* reward_acc, void* workspace, size_t workspace_bytes, mfg_stream_t stream) {
  CHECK_BD();
  REQUIRE(T >= 1 && stride_b >= (int64_t)T * d, "bad T / stride_b");
  REQUIRE(pi && delta && G && workspace && w && theta, "null pointer");
  REQUIRE(!add_reward || reward, "add_reward without reward");
  const ApplyArgs ap{lr_critic, lr_actor, w, theta, reward_acc};
  bool applied = false;
  int rc = launch_grad(pi, stride_b, delta, g, reward, B * T, T, d, G, 0, workspace, workspace_bytes, S(stream), &ap, &applied,
                       add_reward != 0);
  if (rc != MFG_OK) return rc;
  if (!applied) launch_apply_update(G, d, lr_critic, lr_actor, w, theta, reward_acc, S(stream));
  return check_launch("grad_apply");
}

static int train_episode_impl(float* pi_io, float* pi_scratch, int64_t B, int d, int T, double* theta, double shift,
                              double alpha_scale, double* w, double gamma, int reward_kind, uint64_t seed, uint32_t first_step,
                              uint64_t traj_offset, int precision, double lr_critic, double lr_actor, float* reward,
                              double* delta, double* g, double* G, double* reward_acc, void* workspace, size_t workspace_bytes,
                              hipStream_t st, const PopArgs* pop = nullptr) {
  float* cur = pi_io;
  float* nxt = pi_scratch;
  for (int s = 0; s < T; ++s) {
    CoreArgs a{};
    a.pi0 = cur;
    a.theta = theta;
    a.w = w;
    a.shift = shift;
    a.alpha_scale = alpha_scale;
    a.gamma = gamma;
    a.B = B;
    a.d = d;
    a.T = 1;
    a.reward_kind = reward_kind;
    a.seed = seed;
    a.first_step = first_step + (uint32_t)s;
    a.traj_offset = traj_offset;
    a.pi_next_out = nxt;
    a.reward_out = reward;
    a.delta = delta;
    a.g = g;
    const bool sums_in_core = core_sums_ok(d, B, 1, reward_kind, workspace, workspace_bytes);
    if (sums_in_core) a.part_rows = reinterpret_cast<double*>((char*)workspace + MFG_WS_CONTROL_BYTES);
    int rc = launch_core(a, true, true, precision, st, pop);
    if (rc != MFG_OK) return rc;
    const ApplyArgs ap{lr_critic, lr_actor, w, theta, reward_acc};
    bool applied = false;
    if (sums_in_core) {
      rc = reduce_core_sums(d, B, G, 0, workspace, &ap, st, pop);
      applied = true;
    } else {
      rc = launch_grad(cur, d, delta, g, reward, B, 1, d, G, 0, workspace, workspace_bytes, st, &ap, &applied, false, pop);
    }
    if (rc != MFG_OK) return rc;
    if (pop && !applied) return fail(MFG_ELAUNCH, "%s", "population: update not applied");  // (not reached: d <= 64)
    if (!applied) launch_apply_update(G, d, lr_critic, lr_actor, w, theta, reward_acc, st);
    float* t = cur;
    cur = nxt;
    nxt = t;
  }
  if (cur != pi_io && hipMemcpyAsync(pi_io, cur, (size_t)B * d * sizeof(float) * (pop ? pop->K : 1), hipMemcpyDeviceToDevice,
                                     st) != hipSuccess)
    return fail(MFG_ELAUNCH, "%s", "train_episode: final state copy failed");
  return check_launch("train_episode");
}


#define CHECK_TRAIN_EPISODE()                                                                                      \
  CHECK_BD();                                                                                                      \
  CHECK_PRECISION();                                                                                               \
  REQUIRE(T >= 1, "T < 1");                                                                                        \
  REQUIRE(pi_io && pi_scratch && theta && w && reward && delta && g && G && workspace, "null pointer");            \
  REQUIRE(reward_kind == MFG_REWARD_MFG_AC2 || reward_kind == MFG_REWARD_SYNTHETIC, "needs an in-kernel reward")

int mfg_train_episode(float* pi_io, float* pi_scratch, int64_t B, int d, int T, double* theta, double shift,
                      double alpha_scale, double* w, double gamma, int reward_kind, uint64_t seed, uint32_t first_step,
                      uint64_t traj_offset, int precision, double lr_critic, double lr_actor, float* reward, double* delta,
                      double* g, double* G, double* reward_acc, void* workspace, size_t workspace_bytes,
                      mfg_stream_t stream) {
  CHECK_TRAIN_EPISODE();
  return train_episode_impl(pi_io, pi_scratch, B, d, T, theta, shift, alpha_scale, w, gamma, reward_kind, seed, first_step,
                            traj_offset, precision, lr_critic, lr_actor, reward, delta, g, G, reward_acc, workspace,
                            workspace_bytes, S(stream));
}

int mfg_train_episodes(const float* mat_pi0, int64_t num_start, float* pi_io, float* pi_scratch, int64_t B, int d, int T,
                       int64_t episodes, int64_t first_episode, int constant, double* theta, double shift, double alpha_scale,
                       double* w, double gamma, int reward_kind, uint64_t seed, uint32_t first_step, uint64_t traj_offset,
                       int precision, double lr_critic, double lr_actor, float* reward, double* delta, double* g, double* G,
                       double* reward_acc, void* workspace, size_t workspace_bytes, mfg_stream_t stream) {
  CHECK_TRAIN_EPISODE();
  REQUIRE(mat_pi0 && num_start > 0 && num_start <= 0x7FFFFFFF, "null / empty / oversized start-state table");
  REQUIRE(episodes >= 0 && first_episode >= 0, "bad episode range");
  REQUIRE((uint64_t)first_step + (uint64_t)episodes * (uint64_t)T <= 0xFFFFFFFFull, "Philox step counter would wrap");
  for (int64_t k = 0; k < episodes; ++k) {
    const uint32_t step0 = first_step + (uint32_t)(k * T);
    launch_draw_start(mat_pi0, num_start, B, d, seed, step0, traj_offset, nullptr, pi_io, S(stream));
    double sc, sa;
    lr_schedule(first_episode + k, constant, &sc, &sa);
    const int rc = train_episode_impl(pi_io, pi_scratch, B, d, T, theta, shift, alpha_scale, w, gamma, reward_kind, seed, step0,
                                      traj_offset, precision, lr_critic * sc, lr_actor * sa, reward, delta, g, G,
                                      reward_acc ? reward_acc + k : nullptr, workspace, workspace_bytes, S(stream));
    if (rc != MFG_OK) return rc;
  }
  return MFG_OK;
}

// ---- populations (mfg_population.h): K independent learners in the launches of one ----------------------------------------
// workspace of one learner's slice that the update of a population episode needs: the SUMS rows (step mode at the packed sizes)
// or the partial rows of the gradient kernels over N samples -- checked before anything is launched
static size_t pop_workspace_need(int d, int64_t N, bool sums_rows) {
  const int64_t FO = mfg_num_features(d) + 3;
  if (sums_rows) return (size_t)(core_sums_rows(d, N) * FO * 8) + MFG_WS_CONTROL_BYTES;
  int chunk, nob;
  int64_t nsb;
  grad_geometry(N, d, &chunk, &nsb, &nob);
  return (size_t)(nsb * FO * 8) + MFG_WS_CONTROL_BYTES;
}

// the checks every population training call shares (shape_check: the call's own limits on d / B T, right after the shape
// checks; extra_ptrs: its own pointers, checked with the shared ones)
#define CHECK_POP(shape_check, extra_ptrs)                                                                             \
  REQUIRE(K >= 1 && K <= MFG_POP_MAX_K, "population size K outside [1, MFG_POP_MAX_K]");                              \
  CHECK_BD();                                                                                                           \
  shape_check;                                                                                                          \
  REQUIRE(T >= 1, "T < 1");                                                                                             \
  REQUIRE(mat_pi0 && num_start > 0 && num_start <= 0x7FFFFFFF, "null / empty / oversized start-state table");           \
  REQUIRE(theta && shift && alpha_scale && w && seed && lr_critic && lr_actor && reward && delta && g && G && workspace && \
              (extra_ptrs),                                                                                             \
          "null pointer");                                                                                              \
  REQUIRE(workspace_bytes % 256 == 0, "population: workspace_bytes (one learner's slice) must be a multiple of 256");    \
  REQUIRE(episodes >= 0 && first_episode >= 0, "bad episode range");                                                    \
  REQUIRE((uint64_t)first_step + (uint64_t)episodes * (uint64_t)T <= 0xFFFFFFFFull, "Philox step counter would wrap");   \
  REQUIRE(traj_ids_ok(traj_offset, B), "trajectory ids traj_offset + B exceed 2^48 (MFG_TRAJ_ID_LIMIT)")

// the in-kernel-reward populations (d <= 64)
#define CHECK_AC_POP()                                                                                                  \
  CHECK_POP(if (d > WAVE)                                                                                               \
              return fail(MFG_EUNSUPPORTED, "population: d=%d > 64 (one wave per trajectory fills the machine)", d),    \
            true);                                                                                                      \
  REQUIRE(reward_kind == MFG_REWARD_MFG_AC2 || reward_kind == MFG_REWARD_SYNTHETIC, "needs an in-kernel reward")

// The control block a population training call runs under -- that of the bound context, none without one -- and the arrays
// k_pop_retire reads.  begin() checks the block before anything is launched, hands the learners' states to the launches (p.state,
// p.status) and enqueues the check ahead of the first episode (also when the call has no episode); retire() enqueues the step
// after an episode's closing update.  Without a block neither launches anything and p stays as it was.
struct PopControl {
  const mfg_pop_control_t* ctl = nullptr;
  const double *theta = nullptr, *w = nullptr, *shift = nullptr;
  int64_t F = 0;
  bool mixed = false;
  hipStream_t st = nullptr;

  int begin(PopArgs& p, const double* theta_, const double* w_, const double* shift_, bool mixed_, hipStream_t st_) {
    const mfg_ctx* c = bound_ctx();
    if (!c || !c->has_ctl) return MFG_OK;
    REQUIRE(pop_control_complete(c->ctl), "population control block: null pointer");
    REQUIRE(c->ctl.K == p.K, "population control block: set for another population size K");
    ctl = &c->ctl;
    theta = theta_, w = w_, shift = shift_, F = p.F, mixed = mixed_, st = st_;
    p.state = ctl->state;
    p.status = ctl->status;
    launch_pop_retire(*ctl, theta, w, F, shift, mixed, false, st);
    return MFG_OK;
  }
  void retire() const {
    if (ctl) launch_pop_retire(*ctl, theta, w, F, shift, mixed, true, st);
  }
};

static int evaluate_pop_launches(const float* emp32, const double* emp64, int64_t N, int L, int d, int K, const double* theta,
                                 const double* shift, const double* alpha_scale, const uint64_t* seed, uint32_t first_step,
                                 int repeats, int precision, double* metrics, float* pi_traj, void* workspace,
                                 const int32_t* state, unsigned* status, const float** traj_out, hipStream_t st);

// The validation block a population training call runs under -- that of the bound context, none without one
// (mfg_ctx_set_pop_validate, mfg_pop_validate.h).  begin() checks the block against the call before ANYTHING is launched (so ahead
// of PopControl::begin); check(k, p) enqueues the held-out check behind episode k's closing update and retire step when one
// is due: the launches of mfg_evaluate_pop on the call's current theta, with with_score those of mfg_forecast_score on the
// members just rolled out, and k_pop_validate_select.  p carries the control block's states after PopControl::begin.  Without a
// block neither does anything.
struct PopValidate {
  const mfg_pop_validate_t* v = nullptr;
  PopValidateLayout lay{};
  const double *theta = nullptr, *w = nullptr;
  int d = 0, precision = 0;
  hipStream_t st = nullptr;

  int begin(int K, int d_, const double* theta_, const double* w_, int precision_, hipStream_t st_) {
    const mfg_ctx* c = bound_ctx();
    if (!c || !c->has_val) return MFG_OK;
    REQUIRE(pop_validate_complete(c->val), "population validation block: null pointer");
    REQUIRE(c->val.K == K, "population validation block: set for another population size K");
    REQUIRE(c->val.patience == 0 || c->has_ctl,
            "population validation block: patience > 0 needs a population control block (mfg_ctx_set_pop_control)");
    lay = pop_validate_layout(c->val.N, c->val.L, d_, K, c->val.repeats, c->val.with_score != 0);
    if (c->val.workspace_bytes < lay.bytes)
      return fail(MFG_EWORKSPACE, "population validation workspace: need %lld bytes, have %lld", (long long)lay.bytes,
                  (long long)c->val.workspace_bytes);
    v = &c->val;
    theta = theta_, w = w_, d = d_, precision = precision_, st = st_;
    return MFG_OK;
  }
  int check(int64_t k, const PopArgs& p) const {
    if (!v || (k + 1) % v->period != 0) return MFG_OK;
    char* ws = reinterpret_cast<char*>(v->workspace);
    double* metrics = reinterpret_cast<double*>(ws + lay.metrics);
    const float* traj = nullptr;
    int rc = evaluate_pop_launches(v->emp32, v->emp64, v->N, v->L, d, p.K, theta, p.shift, p.alpha_scale, p.seed, v->first_step,
                                   v->repeats, precision, metrics, nullptr, ws, p.state, p.status, &traj, st);
    if (rc != MFG_OK) return rc;
    double* summary = nullptr;
    if (v->with_score) {
      summary = reinterpret_cast<double*>(ws + lay.summary);
      rc = launch_forecast_score(traj, v->N, v->L, d, p.K, v->repeats, v->emp32, v->emp64, reinterpret_cast<double*>(ws + lay.crps),
                                 reinterpret_cast<int32_t*>(ws + lay.less), reinterpret_cast<int32_t*>(ws + lay.equal),
                                 reinterpret_cast<double*>(ws + lay.energy), summary,
                                 reinterpret_cast<double*>(ws + lay.score_ws), st, p.state);
      if (rc != MFG_OK) return fail(rc, "%s", "population validation: score LDS request beyond the budget");
    }
    launch_pop_validate_select(*v, const_cast<int32_t*>(p.state), metrics, summary, theta, w, p.F, st);
    return check_launch("pop_validate");
  }
};

// The evolve block a forward population training call runs under -- that of the bound context, none without one
// (mfg_ctx_set_pop_evolve, mfg_pop_evolve.h).  begin() checks the block against the call and its validation block before ANYTHING
// is launched (after PopValidate::begin, ahead of PopControl::begin); step(k, p) enqueues the two launches of a step behind
// pv.check(k, p) when the check that just ran is an `every`-th one.  Without a block neither does anything.
struct PopEvolve {
  const mfg_pop_evolve_t* e = nullptr;
  const PopValidate* pv = nullptr;
  double *theta = nullptr, *w = nullptr;
  hipStream_t st = nullptr;

  int begin(const PopValidate& pv_, int K, int64_t episodes, double* theta_, double* w_, const double* lr_critic,
            const double* lr_actor, hipStream_t st_) {
    const mfg_ctx* c = bound_ctx();
    if (!c || !c->has_evo) return MFG_OK;
    REQUIRE(pop_evolve_complete(c->evo), "population evolve block: null pointer");
    REQUIRE(c->evo.K == K, "population evolve block: set for another population size K");
    REQUIRE(pv_.v, "population evolve block: needs a population validation block (mfg_ctx_set_pop_validate)");
    REQUIRE(c->evo.lr_critic == lr_critic && c->evo.lr_actor == lr_actor,
            "population evolve block: lr_critic / lr_actor are not the call's arrays");
    REQUIRE((episodes / pv_.v->period) / c->evo.every <= c->evo.max_steps,
            "population evolve block: max_steps < (episodes / period) / every");
    e = &c->evo;
    pv = &pv_;
    theta = theta_, w = w_, st = st_;
    return MFG_OK;
  }
  int step(int64_t k, const PopArgs& p) const {
    if (!e || (k + 1) % pv->v->period != 0) return MFG_OK;
    const int64_t checks = (k + 1) / pv->v->period;  // (the check that just ran is number checks - 1 of the call)
    if (checks % e->every != 0) return MFG_OK;
    char* ws = reinterpret_cast<char*>(pv->v->workspace);
    PopEvolveArgs a{};
    a.state = p.state;
    const mfg_ctx* c = bound_ctx();
    a.theta_prev = (p.state && c && c->has_ctl) ? c->ctl.theta_prev : nullptr;
    a.metrics = reinterpret_cast<const double*>(ws + pv->lay.metrics);
    a.summary = pv->v->with_score ? reinterpret_cast<const double*>(ws + pv->lay.summary) : nullptr;
    a.theta = theta;
    a.w = w;
    a.F = p.F;
    a.step = (int32_t)(checks / e->every - 1);
    launch_pop_evolve(*e, *pv->v, a, st);
    return check_launch("pop_evolve");
  }
};

// the argument block of a population call (the call sets the strides that depend on its flow: s_pi0, s_gpi, s_n, s_P)
static PopArgs pop_args(int K, int64_t B, int d, int64_t T, int64_t episodes, const uint64_t* seed, const double* shift,
                        const double* alpha_scale, const double* lr_critic, const double* lr_actor, size_t workspace_bytes) {
  PopArgs p{};
  p.K = K;
  p.F = mfg_num_features(d);
  p.s_traj = B * (T + 1) * d;
  p.s_state = B * d;
  p.s_acc = episodes;
  p.s_ws = (int64_t)workspace_bytes;
  p.s_theta_b = sizeof(double);
  p.seed = seed;
  p.shift = shift;
  p.alpha_scale = alpha_scale;
  p.lr_c = lr_critic;
  p.lr_a = lr_actor;
  return p;
}

int mfg_train_episodes_pop(const float* mat_pi0, int64_t num_start, float* pi_io, float* pi_scratch, int64_t B, int K, int d, int T,
                           int64_t episodes, int64_t first_episode, int constant, double* theta, const double* shift,
                           const double* alpha_scale, double* w, double gamma, int reward_kind, const uint64_t* seed,
                           uint32_t first_step, uint64_t traj_offset, int precision, const double* lr_critic,
                           const double* lr_actor, float* reward, double* delta, double* g, double* G, double* reward_acc,
                           void* workspace, size_t workspace_bytes, mfg_stream_t stream) {
  CHECK_AC_POP();
  CHECK_PRECISION();
  REQUIRE(pi_io && pi_scratch, "null pointer");
  const bool sums = core_sums_ok(d, B, 1, reward_kind, workspace, workspace_bytes);
  const size_t need = pop_workspace_need(d, B, sums);
  if (workspace_bytes < need)
    return fail(MFG_EWORKSPACE, "population workspace: need %lld bytes per learner, have %lld", (long long)need,
                (long long)workspace_bytes);
  PopArgs p = pop_args(K, B, d, 1, episodes, seed, shift, alpha_scale, lr_critic, lr_actor, workspace_bytes);
  p.s_pi0 = p.s_gpi = B * d;  // (the env step reads and the batch sums read the learner's current states)
  p.s_n = B;
  PopValidate pv;
  if (const int rc = pv.begin(K, d, theta, w, precision, S(stream)); rc != MFG_OK) return rc;
  PopEvolve pe;
  if (const int rc = pe.begin(pv, K, episodes, theta, w, lr_critic, lr_actor, S(stream)); rc != MFG_OK) return rc;
  PopControl pc;
  if (const int rc = pc.begin(p, theta, w, shift, precision == MFG_PRECISION_MIXED, S(stream)); rc != MFG_OK) return rc;
  for (int64_t k = 0; k < episodes; ++k) {
    const uint32_t step0 = first_step + (uint32_t)(k * T);
    launch_draw_start_pop(grid_for(B * d, 256, 8), mat_pi0, num_start, B, d, step0, traj_offset, pi_io, p, S(stream));
    lr_schedule(first_episode + k, constant, &p.sc, &p.sa);
    const int rc = train_episode_impl(pi_io, pi_scratch, B, d, T, theta, 0.0, 0.0, w, gamma, reward_kind, 0, step0, traj_offset,
                                      precision, 0.0, 0.0, reward, delta, g, G, reward_acc ? reward_acc + k : nullptr, workspace,
                                      workspace_bytes, S(stream), &p);
    if (rc != MFG_OK) return rc;
    pc.retire();
    if (const int rv = pv.check(k, p); rv != MFG_OK) return rv;
    if (const int rv = pe.step(k, p); rv != MFG_OK) return rv;
  }
  return MFG_OK;
}

// ---- the resident form of the step-mode population episodes (mfg_pop_resident.hip): one workgroup per learner ----
int mfg_pop_resident_supported(int d, int64_t B, int reward_kind) {
  if (reward_kind != MFG_REWARD_MFG_AC2 && reward_kind != MFG_REWARD_SYNTHETIC) return 0;
  if (B < 1) return 0;
  const int64_t nt = core_sums_rows(d, B);  // (d = 21 / 15: the tiles of the SUMS step; 0 otherwise)
  return nt >= 1 && nt <= MFG_POP_RESIDENT_MAX_TILES;
}

int mfg_train_episodes_pop_resident(const float* mat_pi0, int64_t num_start, float* pi_io, float* pi_scratch, int64_t B, int K,
                                    int d, int T, int64_t episodes, int64_t first_episode, int constant, double* theta,
                                    const double* shift, const double* alpha_scale, double* w, double gamma, int reward_kind,
                                    const uint64_t* seed, uint32_t first_step, uint64_t traj_offset, int precision,
                                    const double* lr_critic, const double* lr_actor, float* reward, double* delta, double* g,
                                    double* G, double* reward_acc, void* workspace, size_t workspace_bytes, mfg_stream_t stream) {
  CHECK_AC_POP();
  CHECK_PRECISION();
  REQUIRE(pi_io && pi_scratch, "null pointer");
  if (!mfg_pop_resident_supported(d, B, reward_kind))
    return fail(MFG_EUNSUPPORTED, "resident population: d=%d, B=%lld is not d = 21 / 15 with at most %d tiles per learner", d,
                (long long)B, MFG_POP_RESIDENT_MAX_TILES);
  if (const mfg_ctx* c = bound_ctx(); c && c->has_ctl)
    return fail(MFG_EUNSUPPORTED, "%s", "resident population: the bound context carries a population control block "
                                        "(mfg_train_episodes_pop retires learners)");
  if (const mfg_ctx* c = bound_ctx(); c && c->has_val)
    return fail(MFG_EUNSUPPORTED, "%s", "resident population: the bound context carries a population validation block "
                                        "(mfg_train_episodes_pop runs the held-out checks)");
  if (const mfg_ctx* c = bound_ctx(); c && c->has_evo)
    return fail(MFG_EUNSUPPORTED, "%s", "resident population: the bound context carries a population evolve block (the "
                                        "resident kernel reads its learning rates once per launch; mfg_train_episodes_pop "
                                        "runs the exploit / explore steps)");
  const size_t need = pop_workspace_need(d, B, true);
  if (workspace_bytes < need)
    return fail(MFG_EWORKSPACE, "population workspace: need %lld bytes per learner, have %lld", (long long)need,
                (long long)workspace_bytes);
  const bool mixed = precision == MFG_PRECISION_MIXED;
  PopArgs p = pop_args(K, B, d, 1, episodes, seed, shift, alpha_scale, lr_critic, lr_actor, workspace_bytes);
  p.s_pi0 = p.s_gpi = B * d;
  p.s_n = B;
  CoreArgs a{};
  a.gamma = gamma;
  a.B = B;
  a.d = d;
  a.T = 1;  // (one env step per call of the step body)
  a.reward_kind = reward_kind;
  a.traj_offset = traj_offset;
  a.reward_out = reward;
  a.delta = delta;
  a.g = g;
  a.part_rows = reinterpret_cast<double*>((char*)workspace + MFG_WS_CONTROL_BYTES);
  if (mixed) {
    a.htab = htab_ptr();
    if (!a.htab) return fail(MFG_ELAUNCH, "%s", "h(z) table initialisation failed");
  }
  PopResidentArgs r{};
  r.mat_pi0 = mat_pi0;
  r.num_start = num_start;
  r.pi_io = pi_io;
  r.pi_scratch = pi_scratch;
  r.theta = theta;
  r.w = w;
  r.G = G;
  r.T = T;
  for (int64_t k0 = 0; k0 < episodes; k0 += MFG_POP_RESIDENT_EPISODES) {
    {  // (as launch_core: the sticky range report of an earlier mixed-precision launch refuses this one)
      const StatusWord sw = status_word();
      if (!sw.host) return fail(MFG_ELAUNCH, "%s", "status word allocation failed");
      const unsigned bits = g_status_check_deferred ? 0u : *(volatile unsigned*)sw.host;
      const unsigned blocking = mixed ? bits : (bits & ~(unsigned)MFG_STATUS_MIXED_RANGE);
      if (blocking) return status_error(blocking);
      a.status = sw.dev;
    }
    const int64_t n = episodes - k0 < MFG_POP_RESIDENT_EPISODES ? episodes - k0 : MFG_POP_RESIDENT_EPISODES;
    r.episodes = (int)n;
    r.first_step = first_step + (uint32_t)(k0 * T);
    r.reward_acc = reward_acc ? reward_acc + k0 : nullptr;
    for (int64_t e = 0; e < n; ++e) lr_schedule(first_episode + k0 + e, constant, &r.sc[e], &r.sa[e]);
    if (const int rc = launch_pop_resident(a, p, r, mixed, S(stream)); rc != MFG_OK)
      return fail(rc, "%s", "resident population: no kernel for this d");
    if (const int rc = check_launch("pop_resident"); rc != MFG_OK) return rc;
  }
  return MFG_OK;
}

int mfg_train_rollouts_pop(const float* mat_pi0, int64_t num_start, int64_t B, int K, int d, int T, int64_t episodes,
                           int64_t first_episode, int constant, double* theta, const double* shift, const double* alpha_scale,
                           double* w, double gamma, int reward_kind, const uint64_t* seed, uint32_t first_step,
                           uint64_t traj_offset, int flags, const double* lr_critic, const double* lr_actor, float* pi_traj,
                           float* pi_last, float* reward, double* delta, double* g, double* G, double* reward_acc,
                           void* workspace, size_t workspace_bytes, mfg_stream_t stream) {
  CHECK_AC_POP();
  REQUIRE(pi_traj, "null pointer");
  const size_t need = pop_workspace_need(d, B * T, false);
  if (workspace_bytes < need)
    return fail(MFG_EWORKSPACE, "population workspace: need %lld bytes per learner, have %lld", (long long)need,
                (long long)workspace_bytes);
  PopArgs p = pop_args(K, B, d, T, episodes, seed, shift, alpha_scale, lr_critic, lr_actor, workspace_bytes);
  p.s_pi0 = 0;  // (the shared start-state table: the rows are drawn in the kernel)
  p.s_gpi = p.s_traj;
  p.s_n = B * T;
  PopValidate pv;
  if (const int rc = pv.begin(K, d, theta, w, (flags & MFG_ROLLOUT_F64) ? MFG_PRECISION_F64 : MFG_PRECISION_MIXED, S(stream));
      rc != MFG_OK)
    return rc;
  PopEvolve pe;
  if (const int rc = pe.begin(pv, K, episodes, theta, w, lr_critic, lr_actor, S(stream)); rc != MFG_OK) return rc;
  PopControl pc;
  if (const int rc = pc.begin(p, theta, w, shift, !(flags & MFG_ROLLOUT_F64), S(stream)); rc != MFG_OK) return rc;
  for (int64_t k = 0; k < episodes; ++k) {
    lr_schedule(first_episode + k, constant, &p.sc, &p.sa);
    const int rc = train_rollout_impl(mat_pi0, num_start, nullptr, B, d, T, theta, 0.0, 0.0, w, gamma, reward_kind, 0,
                                      first_step + (uint32_t)(k * T), traj_offset, flags | MFG_TRAIN_APPLY, 0.0, 0.0, pi_traj,
                                      pi_last, reward, delta, g, G, reward_acc ? reward_acc + k : nullptr, workspace,
                                      workspace_bytes, S(stream), nullptr, &p);
    if (rc != MFG_OK) return rc;
    pc.retire();
    if (const int rv = pv.check(k, p); rv != MFG_OK) return rv;
    if (const int rv = pe.step(k, p); rv != MFG_OK) return rv;
  }
  return MFG_OK;
}

// ---- population evaluation (mfg_evaluate_pop.h): the test rollouts and metrics of K policies in two launches -----------------
size_t mfg_evaluate_pop_workspace_bytes(int64_t N, int L, int d, int K, int repeats, int traj_given) {
  if (N < 1 || L < 1 || d < 1 || K < 1 || repeats < 1) return 0;
  return eval_pop_workspace_bytes(N, L, d, K, repeats, traj_given != 0);
}

// the two launches of mfg_evaluate_pop on checked arguments; state / status: NULL, or those of a control block (a validation
// check inside a training call: retired learners are skipped, range reports go to the learner).  *traj_out: where the members are.
static int evaluate_pop_launches(const float* emp32, const double* emp64, int64_t N, int L, int d, int K, const double* theta,
                                 const double* shift, const double* alpha_scale, const uint64_t* seed, uint32_t first_step,
                                 int repeats, int precision, double* metrics, float* pi_traj, void* workspace,
                                 const int32_t* state, unsigned* status, const float** traj_out, hipStream_t st) {
  const int64_t NR = N * repeats;
  PopArgs p = pop_args(K, NR, d, L - 1, 0, seed, shift, alpha_scale, nullptr, nullptr, 0);
  p.N = N;
  p.L = L;
  p.s_idx = eval_pop_idx_stride(NR);
  p.idx = reinterpret_cast<int32_t*>(workspace);
  p.state = state;
  p.status = status;
  double* per_traj = reinterpret_cast<double*>(reinterpret_cast<char*>(workspace) + (size_t)K * p.s_idx * 4);
  float* traj = pi_traj ? pi_traj : reinterpret_cast<float*>(per_traj + (size_t)K * NR * 4);
  if (traj_out) *traj_out = traj;
  CoreArgs a{};
  a.pi0 = emp32;  // viewed as [N L, d]; row (j mod N) L is the start state of trajectory j
  a.num_start = N * L;
  a.theta = theta;
  a.gamma = 1.0;
  a.B = NR;
  a.d = d;
  a.T = L - 1;
  a.reward_kind = MFG_REWARD_EXTERNAL;  // (states only: no reward is formed)
  a.first_step = first_step;
  a.pi_traj = traj;
  const int rc = launch_core(a, true, false, precision, st, &p);
  if (rc != MFG_OK) return rc;
  launch_eval_metrics_pop(traj, emp32, emp64, N, L, d, NR, K, per_traj, metrics, st, state);
  return check_launch("evaluate_pop metrics");
}

int mfg_evaluate_pop(const float* emp32, const double* emp64, int64_t N, int L, int d, int K, const double* theta,
                     const double* shift, const double* alpha_scale, const uint64_t* seed, uint32_t first_step, int repeats,
                     int precision, double* metrics, float* pi_traj, void* workspace, size_t workspace_bytes,
                     mfg_stream_t stream) {
  REQUIRE(K >= 1 && K <= MFG_POP_MAX_K, "population size K outside [1, MFG_POP_MAX_K]");
  REQUIRE(d >= 1, "d < 1");
  if (d > WAVE) return fail(MFG_EUNSUPPORTED, "population evaluation: d=%d > 64 (as for the populations)", d);
  REQUIRE(L >= 2, "episode_length L < 2");
  REQUIRE(N >= 1, "no test trajectories (N < 1)");
  REQUIRE(repeats >= 1, "repeats < 1");
  REQUIRE(N * (int64_t)L <= 0x7FFFFFFF && N * (int64_t)repeats <= 0x7FFFFFFF, "N L or N repeats too large");
  REQUIRE(emp32 && emp64 && theta && shift && alpha_scale && seed && metrics && workspace, "null pointer");
  CHECK_PRECISION();
  REQUIRE((uint64_t)first_step + (uint64_t)(L - 1) <= 0xFFFFFFFFull, "Philox step counter would wrap");
  const size_t need = eval_pop_workspace_bytes(N, L, d, K, repeats, pi_traj != nullptr);
  if (workspace_bytes < need)
    return fail(MFG_EWORKSPACE, "population evaluation workspace: need %lld bytes, have %lld", (long long)need,
                (long long)workspace_bytes);
  return evaluate_pop_launches(emp32, emp64, N, L, d, K, theta, shift, alpha_scale, seed, first_step, repeats, precision, metrics,
                               pi_traj, workspace, nullptr, nullptr, nullptr, S(stream));
}

// ---- ensemble forecast (mfg_forecast_pop.h): R rollouts per start state of K policies, reduced in at most three launches ------
size_t mfg_forecast_pop_workspace_bytes(int64_t N, int H, int d, int K, int repeats, int traj_given) {
  if (N < 1 || H < 1 || d < 1 || K < 1 || repeats < 1) return 0;
  return forecast_pop_workspace_bytes(N, H, d, K, repeats, traj_given != 0);
}

int mfg_forecast_pop(const float* start32, int64_t N, int H, int d, int K, const double* theta, const double* shift,
                     const double* alpha_scale, const uint64_t* seed, uint32_t first_step, int repeats, int precision,
                     const int32_t* ranks, int Q, const float* emp32, const double* emp64, double* mean, double* std, float* quant,
                     double* curves, float* pi_traj, void* workspace, size_t workspace_bytes, mfg_stream_t stream) {
  REQUIRE(K >= 1 && K <= MFG_POP_MAX_K, "population size K outside [1, MFG_POP_MAX_K]");
  REQUIRE(d >= 1, "d < 1");
  if (d > WAVE) return fail(MFG_EUNSUPPORTED, "ensemble forecast: d=%d > 64 (as for the populations)", d);
  REQUIRE(H >= 2, "horizon H < 2");
  REQUIRE(N >= 1, "no start states (N < 1)");
  REQUIRE(repeats >= 1, "repeats < 1");
  REQUIRE(N * (int64_t)H <= 0x7FFFFFFF && N * (int64_t)repeats <= 0x7FFFFFFF, "N H or N repeats too large");
  REQUIRE(start32 && theta && shift && alpha_scale && seed && mean && std && workspace, "null pointer");
  CHECK_PRECISION();
  REQUIRE((uint64_t)first_step + (uint64_t)(H - 1) <= 0xFFFFFFFFull, "Philox step counter would wrap");
  REQUIRE(Q >= 0 && Q <= MFG_FORECAST_MAX_RANKS, "number of ranks Q outside [0, MFG_FORECAST_MAX_RANKS]");
  REQUIRE(Q == 0 || (ranks && quant), "ranks / quant: null pointer with Q > 0");
  ForecastRanks fr{};
  for (int q = 0; q < Q; ++q) {
    REQUIRE(ranks[q] >= 0 && ranks[q] < repeats, "a rank outside [0, repeats)");
    fr.r[q] = ranks[q];
  }
  REQUIRE((emp32 != nullptr) == (emp64 != nullptr), "emp32 and emp64: both or neither");
  REQUIRE((curves != nullptr) == (emp32 != nullptr), "curves is given exactly when emp32 / emp64 are");
  if (repeats > MFG_FORECAST_MAX_REPEATS)
    return fail(MFG_EUNSUPPORTED, "ensemble forecast: repeats=%d > MFG_FORECAST_MAX_REPEATS=%d", repeats,
                MFG_FORECAST_MAX_REPEATS);
  const size_t need = forecast_pop_workspace_bytes(N, H, d, K, repeats, pi_traj != nullptr);
  if (workspace_bytes < need)
    return fail(MFG_EWORKSPACE, "ensemble forecast workspace: need %lld bytes, have %lld", (long long)need,
                (long long)workspace_bytes);
  const int64_t NR = N * repeats;
  PopArgs p = pop_args(K, NR, d, H - 1, 0, seed, shift, alpha_scale, nullptr, nullptr, 0);
  p.N = N;
  p.L = 1;  // (the start-index table's row stride: member j starts at row j mod N of start32 [N, d])
  p.s_idx = eval_pop_idx_stride(NR);
  p.idx = reinterpret_cast<int32_t*>(workspace);
  double* per_step = reinterpret_cast<double*>(reinterpret_cast<char*>(workspace) + (size_t)K * p.s_idx * 4);
  float* traj = pi_traj ? pi_traj : reinterpret_cast<float*>(per_step + (size_t)K * H * NR * 2);
  CoreArgs a{};
  a.pi0 = start32;
  a.num_start = N;
  a.theta = theta;
  a.gamma = 1.0;
  a.B = NR;
  a.d = d;
  a.T = H - 1;
  a.reward_kind = MFG_REWARD_EXTERNAL;  // (states only: no reward is formed)
  a.first_step = first_step;
  a.pi_traj = traj;
  int rc = launch_core(a, true, false, precision, S(stream), &p);
  if (rc != MFG_OK) return rc;
  rc = launch_forecast_reduce(traj, N, H, d, K, repeats, fr, Q, mean, std, quant, S(stream));
  if (rc != MFG_OK) return fail(rc, "%s", "forecast reduce: LDS request beyond the budget");
  if ((rc = check_launch("forecast_pop reduce")) != MFG_OK) return rc;
  if (!emp32) return MFG_OK;
  launch_forecast_curves(traj, emp32, emp64, N, H, d, NR, K, per_step, curves, S(stream));
  return check_launch("forecast_pop curves");
}

// ---- finite-population forecast (mfg_agents.h): the sampling kernel and k_agents_step in turn, then the forecast's reductions ----
size_t mfg_forecast_agents_pop_workspace_bytes(int64_t N, int H, int d, int K, int repeats, int traj_given, int counts_given) {
  if (N < 1 || H < 1 || d < 1 || K < 1 || repeats < 1) return 0;
  return forecast_agents_workspace_bytes(N, H, d, K, repeats, traj_given != 0, counts_given != 0);
}

int mfg_forecast_agents_pop(const int32_t* counts0, int64_t N, int H, int d, int K, int agents, const double* theta,
                            const double* shift, const double* alpha_scale, const uint64_t* seed, uint32_t first_step, int repeats,
                            int precision, const int32_t* ranks, int Q, const float* emp32, const double* emp64, double* mean,
                            double* std, float* quant, double* curves, float* pi_traj, int32_t* counts_traj, float* actions,
                            void* workspace, size_t workspace_bytes, mfg_stream_t stream) {
  REQUIRE(K >= 1 && K <= MFG_POP_MAX_K, "population size K outside [1, MFG_POP_MAX_K]");
  REQUIRE(d >= 1, "d < 1");
  if (d > WAVE) return fail(MFG_EUNSUPPORTED, "finite-population forecast: d=%d > 64 (as for the populations)", d);
  REQUIRE(H >= 2, "horizon H < 2");
  REQUIRE(N >= 1, "no start states (N < 1)");
  REQUIRE(repeats >= 1, "repeats < 1");
  REQUIRE(agents >= 1 && agents <= MFG_AGENTS_MAX, "agents outside [1, MFG_AGENTS_MAX]");
  REQUIRE(N * (int64_t)H <= 0x7FFFFFFF && N * (int64_t)repeats <= 0x7FFFFFFF, "N H or N repeats too large");
  REQUIRE(counts0 && theta && shift && alpha_scale && seed && mean && std && workspace, "null pointer");
  CHECK_PRECISION();
  REQUIRE((uint64_t)first_step + (uint64_t)(H - 1) <= 0xFFFFFFFFull, "Philox step counter would wrap");
  REQUIRE(Q >= 0 && Q <= MFG_FORECAST_MAX_RANKS, "number of ranks Q outside [0, MFG_FORECAST_MAX_RANKS]");
  REQUIRE(Q == 0 || (ranks && quant), "ranks / quant: null pointer with Q > 0");
  ForecastRanks fr{};
  for (int q = 0; q < Q; ++q) {
    REQUIRE(ranks[q] >= 0 && ranks[q] < repeats, "a rank outside [0, repeats)");
    fr.r[q] = ranks[q];
  }
  REQUIRE((emp32 != nullptr) == (emp64 != nullptr), "emp32 and emp64: both or neither");
  REQUIRE((curves != nullptr) == (emp32 != nullptr), "curves is given exactly when emp32 / emp64 are");
  if (repeats > MFG_FORECAST_MAX_REPEATS)
    return fail(MFG_EUNSUPPORTED, "finite-population forecast: repeats=%d > MFG_FORECAST_MAX_REPEATS=%d", repeats,
                MFG_FORECAST_MAX_REPEATS);
  const size_t need = forecast_agents_workspace_bytes(N, H, d, K, repeats, pi_traj != nullptr, counts_traj != nullptr);
  if (workspace_bytes < need)
    return fail(MFG_EWORKSPACE, "finite-population forecast workspace: need %lld bytes, have %lld", (long long)need,
                (long long)workspace_bytes);
  REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, "workspace not 8-byte aligned");
  const int64_t NR = N * repeats;
  PopArgs p = pop_args(K, NR, d, 1, 0, seed, shift, alpha_scale, nullptr, nullptr, 0);
  p.N = NR;  // (member j reads row j of its learner's current rows: the start-index table is the identity)
  p.L = 1;
  p.s_idx = eval_pop_idx_stride(NR);
  p.idx = reinterpret_cast<int32_t*>(workspace);
  p.s_pi0 = NR * d;
  p.s_P = NR * d * d;
  char* at = reinterpret_cast<char*>(workspace) + (size_t)K * p.s_idx * 4;
  double* per_step = reinterpret_cast<double*>(at);
  at += (size_t)K * H * NR * 2 * 8;
  float* cur = reinterpret_cast<float*>(at);
  at += agents_pad8((size_t)K * NR * d * 4);
  float* P_step = reinterpret_cast<float*>(at);
  at += agents_pad8((size_t)K * NR * d * d * 4);
  float* traj = pi_traj;
  if (!traj) {
    traj = reinterpret_cast<float*>(at);
    at += agents_pad8((size_t)K * NR * H * d * 4);
  }
  int32_t* ctraj = counts_traj ? counts_traj : reinterpret_cast<int32_t*>(at);
  // The sticky status word is examined ONCE, here, before anything is launched (launch_core's rule: a range report of an
  // earlier mixed-precision launch refuses a mixed-precision call).  The H - 1 sampling launches below then go ahead whatever
  // the device reports meanwhile, as the one launch of mfg_forecast_pop does: a policy that leaves the range in this call has
  // unspecified actions (each of its members fails or stays a histogram of its agents), the other policies are complete,
  // the call returns MFG_OK and the NEXT call is refused -- whatever the host's timing.
  {
    const StatusWord sw = status_word();
    if (!sw.host) return fail(MFG_ELAUNCH, "%s", "status word allocation failed");
    const unsigned bits = g_status_check_deferred ? 0u : *(volatile unsigned*)sw.host;
    const unsigned blocking = precision == MFG_PRECISION_MIXED ? bits : (bits & ~(unsigned)MFG_STATUS_MIXED_RANGE);
    if (blocking) return status_error(blocking);
  }
  struct DeferGuard {
    const bool was = g_status_check_deferred;
    DeferGuard() { g_status_check_deferred = true; }
    ~DeferGuard() { g_status_check_deferred = was; }
  } defer_guard;
  launch_agents_init(counts0, N, NR, H, d, K, agents, ctraj, traj, cur, S(stream));
  int rc = check_launch("forecast_agents_pop init");
  if (rc != MFG_OK) return rc;
  CoreArgs a{};
  a.pi0 = cur;
  a.num_start = NR;
  a.theta = theta;
  a.gamma = 1.0;
  a.B = NR;
  a.d = d;
  a.T = 1;
  a.reward_kind = MFG_REWARD_EXTERNAL;  // (actions only: no reward is formed)
  a.P_out = P_step;
  AgentsArgs g{};
  g.cs_k = g.ns_k = g.ps_k = NR * H * d;
  g.cs_m = g.ns_m = g.ps_m = (int64_t)H * d;
  g.P = P_step;
  g.pi_cur = cur;
  g.as_k = NR * (int64_t)(H - 1) * d * d;
  g.as_m = (int64_t)(H - 1) * d * d;
  g.seed = seed;
  g.B = NR;
  g.d = d;
  g.agents = agents;
  for (int t = 0; t < H - 1; ++t) {
    a.first_step = first_step + (uint32_t)t;
    if ((rc = launch_core(a, true, false, precision, S(stream), &p)) != MFG_OK) return rc;
    g.counts = ctraj + (int64_t)t * d;
    g.counts_next = ctraj + (int64_t)(t + 1) * d;
    g.pi_next = traj + (int64_t)(t + 1) * d;
    g.P_copy = actions ? actions + (int64_t)t * d * d : nullptr;
    g.step = a.first_step;
    launch_agents_step(g, K, S(stream));
    if ((rc = check_launch("forecast_agents_pop step")) != MFG_OK) return rc;
  }
  rc = launch_forecast_reduce(traj, N, H, d, K, repeats, fr, Q, mean, std, quant, S(stream));
  if (rc != MFG_OK) return fail(rc, "%s", "forecast reduce: LDS request beyond the budget");
  if ((rc = check_launch("forecast_agents_pop reduce")) != MFG_OK) return rc;
  if (!emp32) return MFG_OK;
  launch_forecast_curves(traj, emp32, emp64, N, H, d, NR, K, per_step, curves, S(stream));
  return check_launch("forecast_agents_pop curves");
}

// ---- backward-equation check (mfg_consistency_pop.h): the scan and the reduction of K groups; with the rollouts three launches ----
size_t mfg_consistency_given_workspace_bytes(int K, int64_t M, int T, int steps_given) {
  if (K < 1 || M < 1 || T < 1) return 0;
  return consistency_given_workspace_bytes(K, M, T, steps_given != 0);
}

// the two launches both entries share: B = K M trajectories' actions -> steps (given, or `scratch`), V if asked for, metrics
static int consistency_launches(const float* P, int K, int64_t M, int T, int d, double* metrics, double* steps, double* V,
                                hipStream_t st) {
  launch_consistency_backward(P, (int64_t)K * M, T, d, V, steps, num_cus(), st);
  if (const int rc = check_launch("consistency backward"); rc != MFG_OK) return rc;
  launch_consistency_reduce(steps, K, M * T, metrics, st);
  return check_launch("consistency reduce");
}

int mfg_consistency_given(const float* P, int K, int64_t M, int T, int d, double* metrics, double* steps, double* V,
                          void* workspace, size_t workspace_bytes, mfg_stream_t stream) {
  REQUIRE(K >= 1 && K <= MFG_POP_MAX_K, "number of groups K outside [1, MFG_POP_MAX_K]");
  REQUIRE(d >= 1, "d < 1");
  if (d > WAVE) return fail(MFG_EUNSUPPORTED, "backward-equation check: d=%d > 64 (as for the populations)", d);
  REQUIRE(T >= 1, "T < 1 (hours H < 2)");
  REQUIRE(M >= 1, "no trajectories (M < 1)");
  REQUIRE(M * (int64_t)T <= 0x7FFFFFFF, "M T too large");
  REQUIRE(P && metrics && (steps || workspace), "null pointer");
  const size_t need = consistency_given_workspace_bytes(K, M, T, steps != nullptr);
  if (workspace_bytes < need)
    return fail(MFG_EWORKSPACE, "backward-equation check workspace: need %lld bytes, have %lld", (long long)need,
                (long long)workspace_bytes);
  return consistency_launches(P, K, M, T, d, metrics, steps ? steps : reinterpret_cast<double*>(workspace), V, S(stream));
}

size_t mfg_consistency_pop_workspace_bytes(int64_t N, int H, int d, int K, int repeats, int steps_given, int actions_given,
                                           int traj_given) {
  if (N < 1 || H < 2 || d < 1 || K < 1 || repeats < 1) return 0;
  return consistency_pop_workspace_bytes(N, H, d, K, repeats, steps_given != 0, actions_given != 0, traj_given != 0);
}

int mfg_consistency_pop(const float* start32, int64_t N, int H, int d, int K, const double* theta, const double* shift,
                        const double* alpha_scale, const uint64_t* seed, uint32_t first_step, int repeats, int precision,
                        double* metrics, double* steps, double* V, float* actions, float* pi_traj, void* workspace,
                        size_t workspace_bytes, mfg_stream_t stream) {
  REQUIRE(K >= 1 && K <= MFG_POP_MAX_K, "population size K outside [1, MFG_POP_MAX_K]");
  REQUIRE(d >= 1, "d < 1");
  if (d > WAVE) return fail(MFG_EUNSUPPORTED, "backward-equation check: d=%d > 64 (as for the populations)", d);
  REQUIRE(H >= 2, "hours H < 2");
  REQUIRE(N >= 1, "no start states (N < 1)");
  REQUIRE(repeats >= 1, "repeats < 1");
  REQUIRE(N * (int64_t)H <= 0x7FFFFFFF && N * (int64_t)repeats <= 0x7FFFFFFF &&
              N * (int64_t)repeats * (H - 1) <= 0x7FFFFFFF,
          "N H or N repeats (H - 1) too large");
  REQUIRE(start32 && theta && shift && alpha_scale && seed && metrics && workspace, "null pointer");
  CHECK_PRECISION();
  REQUIRE((uint64_t)first_step + (uint64_t)(H - 1) <= 0xFFFFFFFFull, "Philox step counter would wrap");
  const size_t need = consistency_pop_workspace_bytes(N, H, d, K, repeats, steps != nullptr, actions != nullptr, pi_traj != nullptr);
  if (workspace_bytes < need)
    return fail(MFG_EWORKSPACE, "backward-equation check workspace: need %lld bytes, have %lld", (long long)need,
                (long long)workspace_bytes);
  const int64_t NR = N * repeats;
  const int T = H - 1;
  PopArgs p = pop_args(K, NR, d, T, 0, seed, shift, alpha_scale, nullptr, nullptr, 0);
  p.N = N;
  p.L = 1;  // (member j starts at row j mod N of start32 [N, d], as in a forecast)
  p.s_idx = eval_pop_idx_stride(NR);
  p.idx = reinterpret_cast<int32_t*>(workspace);
  p.s_P = NR * T * d * d;
  char* at = reinterpret_cast<char*>(workspace) + (size_t)K * p.s_idx * 4;
  double* per_step = steps;
  if (!per_step) {
    per_step = reinterpret_cast<double*>(at);
    at += consistency_given_workspace_bytes(K, NR, T, false);
  }
  float* traj = pi_traj;
  if (!traj) {
    traj = reinterpret_cast<float*>(at);
    at += ((size_t)K * NR * H * d * 4 + 7) / 8 * 8;
  }
  float* acts = actions ? actions : reinterpret_cast<float*>(at);
  CoreArgs a{};
  a.pi0 = start32;
  a.num_start = N;
  a.theta = theta;
  a.gamma = 1.0;
  a.B = NR;
  a.d = d;
  a.T = T;
  a.reward_kind = MFG_REWARD_EXTERNAL;  // (states and actions only: no reward is formed)
  a.first_step = first_step;
  a.pi_traj = traj;
  a.P_out = acts;
  if (const int rc = launch_core(a, true, false, precision, S(stream), &p); rc != MFG_OK) return rc;
  return consistency_launches(acts, K, NR, T, d, metrics, per_step, V, S(stream));
}

// ---- IRL forward learners (AC_IRL.train): the reward comes from the reward network, launched between the core kernel and the
// update.  One driver per flow serves the single learner and the population of K (mfg_population.h, mfg_irl_population.h):
// train_rollout_impl with an ExtReward (rollout mode) and train_episode_irl_step (step mode, two launches per env step) ----
// the checks the single-learner calls share (pre_check: the call's own, right after the shape checks; extra_ptrs: its pointers)
#define CHECK_IRL(pre_check, extra_ptrs)                                                                                 \
  CHECK_BD();                                                                                                            \
  pre_check;                                                                                                             \
  REQUIRE(T >= 1, "T < 1");                                                                                              \
  REQUIRE(theta && w && net && P && reward && delta && g && G && workspace && (extra_ptrs), "null pointer")

// the IRL populations: B T samples per learner (checked ahead of T >= 1, which changes nothing: a T < 1 keeps B T small), the
// reward network's settings and the matrix-core kernel's geometry
#define CHECK_IRL_POP()                                                                                                  \
  REQUIRE(net_stride >= 0, "net_stride < 0");                                                                            \
  CHECK_POP(REQUIRE(B * (int64_t)T <= 0x7FFFFFFF, "B * T too large"), net && rn_seed && P);                             \
  REQUIRE(net->keep_prob > 0.0f && net->keep_prob <= 1.0f, "reward net: keep_prob must be in (0,1]");                    \
  if (!reward_net_pop_ready(d, net, per_learner_net, K, net_stride))                                                     \
    return fail(MFG_EUNSUPPORTED, "IRL population: d=%d, k1=%d, f2=%d, k2=%d, n_fc3=%d, n_fc4=%d: not the matrix-core "  \
                "reward network (d = 21 / 15, 5 / 2 / 3, n_fc3 <= 16, 8-byte aligned fc3_w of every learner)",           \
                d, net->k1, net->f2, net->k2, net->n3, net->n4)

// the IRL population calls refuse a bound evolve block (mfg_ctx_set_pop_evolve) before anything is launched
#define REFUSE_POP_EVOLVE()                                                                                              \
  if (const mfg_ctx* c_evo = bound_ctx(); c_evo && c_evo->has_evo)                                                       \
  return fail(MFG_EUNSUPPORTED, "%s", "IRL population: the bound context carries a population evolve block; IRL learners " \
                                      "may carry different reward networks, which an exploit would have to copy too")

// a population with a geometry table (geom_host / geom_dev given; rn_pop_nets_struct, mfg_irl_population.h): its checks, then
// the launches are set up with the row base and the table's maxima
#define IRL_POP_NETS()                                                                                                   \
  mfg_reward_net_t net_max;                                                                                              \
  if (geom_host || geom_dev) {                                                                                           \
    REQUIRE(net && net->conv1_w, "null pointer");                                                                        \
    const int rc_g = rn_pop_nets_struct(net, geom_host, geom_dev, K, d, per_learner_net, net_stride, &net_max);          \
    if (rc_g != MFG_OK) return rc_g;                                                                                     \
    net = &net_max;                                                                                                      \
  }

// dropout key of reward-network call number `call` (1-based) under rn_seed (a population forms its learners' keys in the
// kernel, from rn_seed[k] and the counter call_base[k] + call_j)
static uint64_t rn_dropout_key(uint64_t rn_seed, uint64_t call) { return rn_seed ^ (call * 0x9E3779B97F4A7C15ull); }

// the reward network's population block (the call sets the strides of its flow: s_state, s_action, s_n, s_next, s_w)
// (rn_call0: the per-learner reward-call counters [K]; net_stride: elements between two learners' weights, 0: the numel
//  strides of the stacked tensors; geom_dev: the geometry table, NULL without one)
static RnPop rn_pop_args(int K, int per_learner_net, int64_t net_stride, const uint64_t* rn_seed, const uint64_t* rn_call0,
                         size_t workspace_bytes, const mfg_rn_geom_t* geom_dev) {
  RnPop rp{};
  rp.K = K;
  rp.per_learner_net = per_learner_net ? 1 : 0;
  rp.s_ws = (int64_t)workspace_bytes;
  rp.rn_seed = rn_seed;
  rp.call_base = rn_call0;
  rp.s_net = per_learner_net ? net_stride : 0;
  rp.geom = geom_dev;
  return rp;
}

// one learner's workspace (slice) in the two-launch step flow: control block, with two theta slots at bytes 16 / 24 (theta
// after odd / even steps) | column F of the rows, contiguous [max_rows] | the rows [max_rows][F+3]; max_rows <= 256: one row
// per block of the reward-network launch
struct IrlStepWs {
  int64_t max_rows;
  size_t bytes;
  double *theta_slot, *col_f, *rows;
};
static IrlStepWs irl_step_ws(void* workspace, int64_t B, int d) {
  IrlStepWs l{};
  l.max_rows = (B + 15) / 16 < 256 ? (B + 15) / 16 : 256;
  l.bytes = MFG_WS_CONTROL_BYTES + (size_t)l.max_rows * (mfg_num_features(d) + 3 + 1) * 8;
  l.theta_slot = reinterpret_cast<double*>((char*)workspace + 16);
  l.col_f = reinterpret_cast<double*>((char*)workspace + MFG_WS_CONTROL_BYTES);
  l.rows = l.col_f + l.max_rows;
  return l;
}

// One step-mode episode, two launches per env step where the matrix-core reward-network kernel serves (d = 21 / 15, n_fc3 <= 16;
// the caller asked reward_net_sums_td_ready / reward_net_pop_ready and checked the room for irl_step_ws):
//   step kernel (STEP variant): sampling + transition + score with theta formed from the PREVIOUS step's partial rows by
//     every wave; the grid's last blocks reduce those rows and publish w, theta, G, the return;
//   reward network: r, the TD error delta = r + discount V(pi') - V(pi) from the updated w, this step's partial rows.
// The row reduction -- a launch of its own between two dependent launches before -- leaves the critical path; ONE closes the
// episode.  mat_pi0 != NULL: the start states are DRAWN from the table [num_start,d] inside the first step kernel (the draw of
// mfg_draw_start at step = first_step) and pi_io is an output only; NULL (single learner): pi_io holds them.
// rn_call0: reward-network calls before this episode.  pop / rp != NULL: the population; the per-learner scalars (shift,
// alpha_scale, seed, the learning rates, rn_seed) then come from their device arrays and the ones passed here are not read;
// the strides that change from step to step (s_pi0, s_theta_b) and the reward-call number are set here.
static int train_episode_irl_step(const float* mat_pi0, int64_t num_start, float* pi_io, float* pi_scratch, int64_t B, int d, int T,
                                  double* theta, double shift, double alpha_scale, double* w, double gamma, uint64_t seed,
                                  uint32_t first_step, uint64_t traj_offset, int precision, double lr_critic, double lr_actor,
                                  const mfg_reward_net_t& net, uint64_t rn_seed, uint64_t rn_call0, uint64_t rn_sample_offset,
                                  float* P, float* reward, double* delta, double* g, double* G, double* reward_acc, void* workspace,
                                  size_t workspace_bytes, hipStream_t st, PopArgs* pop = nullptr, RnPop* rp = nullptr) {
  const int64_t FO = mfg_num_features(d) + 3;
  const IrlStepWs ws = irl_step_ws(workspace, B, d);
  // drawn start states: the buffers alternate so that the LAST step writes pi_io (no copy); given ones start in pi_io and,
  // after an odd number of steps, the final states are copied back
  const bool last_in_io = mat_pi0 && (T & 1);
  float* cur = last_in_io ? pi_scratch : pi_io;
  float* nxt = last_in_io ? pi_io : pi_scratch;
  const double* th_in = theta;          // theta [K] before the first update, then the slot the previous step kernel wrote
  int64_t s_th_in = sizeof(double);     // (bytes between two learners' th_in)
  double discount = 1.0;                // running gamma^t of ac_irl.py:691, :710
  int nrows = 0;
  for (int s = 0; s < T; ++s) {
    CoreArgs a{};
    a.pi0 = cur;
    if (s == 0 && mat_pi0) {  // the first step kernel draws its start states itself and leaves them in `cur` for the network
      a.pi0 = mat_pi0;
      a.num_start = num_start;
      a.start_draw = 1;
      a.pi_start_out = cur;
      a.step_nrows = -1;
    }
    a.theta = th_in;
    a.w = nullptr;  // no value part here
    a.shift = shift;
    a.alpha_scale = alpha_scale;
    a.gamma = discount;
    a.B = B;
    a.d = d;
    a.T = 1;
    a.reward_kind = MFG_REWARD_EXTERNAL;
    a.seed = seed;
    a.first_step = first_step + (uint32_t)s;
    a.traj_offset = traj_offset;
    a.pi_next_out = nxt;
    a.g = g;
    a.P_out = P;
    if (s > 0) {  // (the first step has nothing to reduce: the plain kernel, without its value part)
      a.step_G = G;
      a.pend_lr_c = lr_critic;
      a.pend_lr_a = lr_actor;
      a.w_out = w;
      a.pend_reward_acc = reward_acc;
      a.step_rows = ws.rows;
      a.step_nrows = nrows;
      a.theta_out = ws.theta_slot + (s & 1);
    }
    if (pop) {
      pop->s_pi0 = a.start_draw ? 0 : B * d;  // (0: the shared start-state table)
      pop->s_theta_b = s_th_in;
    }
    int rc = launch_core(a, true, true, precision, st, pop);
    if (rc != MFG_OK) return rc;
    if (s > 0) {
      th_in = ws.theta_slot + (s & 1);
      s_th_in = (int64_t)workspace_bytes;
    }
    const uint64_t call = rn_call0 + (uint64_t)s + 1ull;
    if (rp) rp->call_j = call;  // (a population passes rn_call0 = its own count: learner k's counter is rp->call_base[k])
    RnSums sm{};
    sm.g = g;
    sm.delta_out = delta;
    sm.part_rows = ws.rows;
    sm.max_rows = ws.max_rows;
    sm.td_w = w;
    sm.state_next = nxt;
    sm.td_gamma = discount;
    sm.col_f = ws.col_f;
    int rows = 0;
    rc = reward_net_forward_sums(cur, P, B, d, net, rn_dropout_key(rn_seed, call), rn_sample_offset, reward, &sm, &rows, st, 0, rp);
    if (rc != MFG_OK) return rc;
    if (rows != (int)ws.max_rows) return fail(MFG_ELAUNCH, "%s", "train_episode_irl: the reward-network launch left no partial rows");
    nrows = rows;
    discount *= gamma;
    float* t = cur;
    cur = nxt;
    nxt = t;
  }
  if (pop) pop->s_theta_b = s_th_in;
  launch_reduce_rows_apply(ws.rows, nrows, FO, G, lr_critic, lr_actor, (double)B, w, th_in, theta, reward_acc, ws.theta_slot, st, pop);
  if (cur != pi_io && hipMemcpyAsync(pi_io, cur, (size_t)B * d * sizeof(float) * (pop ? pop->K : 1), hipMemcpyDeviceToDevice,
                                     st) != hipSuccess)
    return fail(MFG_ELAUNCH, "%s", "train_episode_irl: final state copy failed");
  return check_launch("train_episode_irl");
}

// The same episode where the two-launch flow does not serve (single learner): three launches per env step, [step kernel with
// its value part | reward network | update]
static int train_episode_irl_3launch(const float* mat_pi0, int64_t num_start, float* pi_io, float* pi_scratch, int64_t B, int d,
                                     int T, double* theta, double shift, double alpha_scale, double* w, double gamma, uint64_t seed,
                                     uint32_t first_step, uint64_t traj_offset, int precision, double lr_critic, double lr_actor,
                                     const mfg_reward_net_t& net, uint64_t rn_seed, uint64_t rn_call0, uint64_t rn_sample_offset,
                                     float* P, float* reward, double* delta, double* g, double* G, double* reward_acc,
                                     void* workspace, size_t workspace_bytes, hipStream_t st) {
  float* cur = pi_io;
  float* nxt = pi_scratch;
  double discount = 1.0;
  if (mat_pi0) {
    launch_draw_start(mat_pi0, num_start, B, d, seed, first_step, traj_offset, nullptr, pi_io, st);
    const int rc = check_launch("draw_start");
    if (rc != MFG_OK) return rc;
  }
  for (int s = 0; s < T; ++s) {
    CoreArgs a{};
    a.pi0 = cur;
    a.theta = theta;
    a.w = w;
    a.shift = shift;
    a.alpha_scale = alpha_scale;
    a.gamma = discount;
    a.B = B;
    a.d = d;
    a.T = 1;
    a.reward_kind = MFG_REWARD_EXTERNAL;  // delta = discount V(pi') - V(pi); the reward joins it in the gradient kernel
    a.seed = seed;
    a.first_step = first_step + (uint32_t)s;
    a.traj_offset = traj_offset;
    a.pi_next_out = nxt;
    a.delta = delta;
    a.g = g;
    a.P_out = P;
    int rc = launch_core(a, true, true, precision, st);
    if (rc != MFG_OK) return rc;
    // reward network; at the packed sizes the same launch folds delta = delta0 + r and leaves the partial rows of the batch
    // sums (one per block of eight samples), so the update is a row reduction instead of a gradient kernel
    const int64_t FO = mfg_num_features(d) + 3;
    const int64_t room = workspace_bytes > MFG_WS_CONTROL_BYTES ? (int64_t)((workspace_bytes - MFG_WS_CONTROL_BYTES) / (size_t)(FO * 8)) : 0;
    const RnSums sm{delta, g, delta, reinterpret_cast<double*>((char*)workspace + MFG_WS_CONTROL_BYTES), room};
    int rows = 0;
    rc = reward_net_forward_sums(cur, P, B, d, net, rn_dropout_key(rn_seed, rn_call0 + (uint64_t)s + 1ull), rn_sample_offset, reward,
                                 &sm, &rows, st);
    if (rc != MFG_OK) return rc;
    const ApplyArgs ap{lr_critic, lr_actor, w, theta, reward_acc};
    bool applied = false;
    if (rows > 0) {
      ReduceApply rap{};
      rap.on = 1;
      rap.lr_c = lr_critic;
      rap.lr_a = lr_actor;
      rap.count = (double)B;
      rap.w = w;
      rap.theta = theta;
      rap.reward_acc = reward_acc;
      launch_reduce_partials(sm.part_rows, rows, FO, 0, G, rap, st);
      applied = true;
      rc = check_launch("irl_sums");
    } else {
      rc = launch_grad(cur, d, delta, g, reward, B, 1, d, G, 0, workspace, workspace_bytes, st, &ap, &applied, true);
    }
    if (rc != MFG_OK) return rc;
    if (!applied) launch_apply_update(G, d, lr_critic, lr_actor, w, theta, reward_acc, st);
    discount *= gamma;
    float* t = cur;
    cur = nxt;
    nxt = t;
  }
  if (cur != pi_io && hipMemcpyAsync(pi_io, cur, (size_t)B * d * sizeof(float), hipMemcpyDeviceToDevice, st) != hipSuccess)
    return fail(MFG_ELAUNCH, "%s", "train_episode_irl: final state copy failed");
  return check_launch("train_episode_irl");
}

// the single learner's episode: the two-launch flow where it serves and the workspace has room, else three launches per step
static int train_episode_irl_impl(const float* mat_pi0, int64_t num_start, float* pi_io, float* pi_scratch, int64_t B, int d, int T,
                                  double* theta, double shift, double alpha_scale, double* w, double gamma, uint64_t seed,
                                  uint32_t first_step, uint64_t traj_offset, int precision, double lr_critic, double lr_actor,
                                  const mfg_reward_net_t* net, uint64_t rn_seed, uint64_t rn_call0, uint64_t rn_sample_offset,
                                  float* P, float* reward, double* delta, double* g, double* G, double* reward_acc, void* workspace,
                                  size_t workspace_bytes, mfg_stream_t stream) {
  CHECK_IRL(CHECK_PRECISION(), pi_io && pi_scratch);
  REQUIRE(!mat_pi0 || (num_start > 0 && num_start <= 0x7FFFFFFF), "empty / oversized start-state table");
  const IrlStepWs ws = irl_step_ws(workspace, B, d);
  if (d <= WAVE && reward_net_sums_td_ready(B, d, *net, workspace_bytes >= ws.bytes ? ws.max_rows : 0))
    return train_episode_irl_step(mat_pi0, num_start, pi_io, pi_scratch, B, d, T, theta, shift, alpha_scale, w, gamma, seed,
                                  first_step, traj_offset, precision, lr_critic, lr_actor, *net, rn_seed, rn_call0, rn_sample_offset,
                                  P, reward, delta, g, G, reward_acc, workspace, workspace_bytes, S(stream));
  return train_episode_irl_3launch(mat_pi0, num_start, pi_io, pi_scratch, B, d, T, theta, shift, alpha_scale, w, gamma, seed,
                                   first_step, traj_offset, precision, lr_critic, lr_actor, *net, rn_seed, rn_call0,
                                   rn_sample_offset, P, reward, delta, g, G, reward_acc, workspace, workspace_bytes, S(stream));
}

// The IRL populations (include/mfg_hip.h): K learners in the launches of one, with or without a geometry table; rn_call0 [K].
// step mode: `episodes` x train_episode_irl_step over all K
int mfg_train_episodes_irl_pop(const float* mat_pi0, int64_t num_start, float* pi_out, float* pi_scratch, int64_t B, int K, int d,
                               int T, int64_t episodes, int64_t first_episode, int constant, double* theta, const double* shift,
                               const double* alpha_scale, double* w, double gamma, const uint64_t* seed, uint32_t first_step,
                               uint64_t traj_offset, int precision, const double* lr_critic, const double* lr_actor,
                               const mfg_reward_net_t* net, int per_learner_net, int64_t net_stride,
                               const mfg_rn_geom_t* geom_host, const mfg_rn_geom_t* geom_dev, const uint64_t* rn_seed,
                               const uint64_t* rn_call0, float* P, float* reward, double* delta, double* g, double* G,
                               double* reward_acc, void* workspace, size_t workspace_bytes, mfg_stream_t stream) {
  REQUIRE(rn_call0 && pi_out && pi_scratch, "null pointer");
  IRL_POP_NETS();
  CHECK_IRL_POP();
  REFUSE_POP_EVOLVE();
  CHECK_PRECISION();
  const size_t need = irl_step_ws(workspace, B, d).bytes;
  if (workspace_bytes < need)
    return fail(MFG_EWORKSPACE, "IRL population workspace: need %lld bytes per learner, have %lld", (long long)need,
                (long long)workspace_bytes);
  PopArgs p = pop_args(K, B, d, 1, episodes, seed, shift, alpha_scale, lr_critic, lr_actor, workspace_bytes);
  p.s_n = B;
  p.s_P = B * d * d;
  RnPop rp = rn_pop_args(K, per_learner_net, net_stride, rn_seed, rn_call0, workspace_bytes, geom_dev);
  rp.s_state = rp.s_next = B * d;
  rp.s_action = B * d * d;
  rp.s_n = B;
  rp.s_w = p.F;
  PopValidate pv;
  if (const int rc = pv.begin(K, d, theta, w, precision, S(stream)); rc != MFG_OK) return rc;
  PopControl pc;
  if (const int rc = pc.begin(p, theta, w, shift, precision == MFG_PRECISION_MIXED, S(stream)); rc != MFG_OK) return rc;
  rp.state = p.state;
  for (int64_t e = 0; e < episodes; ++e) {
    lr_schedule(first_episode + e, constant, &p.sc, &p.sa);
    const int rc = train_episode_irl_step(mat_pi0, num_start, pi_out, pi_scratch, B, d, T, theta, 0.0, 0.0, w, gamma, 0,
                                          first_step + (uint32_t)(e * T), traj_offset, precision, 0.0, 0.0, *net, 0,
                                          (uint64_t)(e * T), traj_offset, P, reward, delta, g, G,
                                          reward_acc ? reward_acc + e : nullptr, workspace, workspace_bytes, S(stream), &p, &rp);
    if (rc != MFG_OK) return rc;
    pc.retire();
    if (const int rv = pv.check(e, p); rv != MFG_OK) return rv;
  }
  return MFG_OK;
}

// rollout mode: `episodes` x train_rollout_impl with the reward network as its ExtReward
int mfg_train_rollouts_irl_pop(const float* mat_pi0, int64_t num_start, int64_t B, int K, int d, int T, int64_t episodes,
                               int64_t first_episode, int constant, double* theta, const double* shift, const double* alpha_scale,
                               double* w, double gamma, const uint64_t* seed, uint32_t first_step, uint64_t traj_offset, int flags,
                               const double* lr_critic, const double* lr_actor, const mfg_reward_net_t* net, int per_learner_net,
                               int64_t net_stride, const mfg_rn_geom_t* geom_host, const mfg_rn_geom_t* geom_dev,
                               const uint64_t* rn_seed, const uint64_t* rn_call0, float* pi_traj, float* pi_last, float* P,
                               float* reward, double* delta, double* g, double* G, double* reward_acc, void* workspace,
                               size_t workspace_bytes, mfg_stream_t stream) {
  REQUIRE(rn_call0 && pi_traj, "null pointer");
  IRL_POP_NETS();
  CHECK_IRL_POP();
  REFUSE_POP_EVOLVE();
  const size_t need = pop_workspace_need(d, B * T, false);
  if (workspace_bytes < need)
    return fail(MFG_EWORKSPACE, "IRL population workspace: need %lld bytes per learner, have %lld", (long long)need,
                (long long)workspace_bytes);
  PopArgs p = pop_args(K, B, d, T, episodes, seed, shift, alpha_scale, lr_critic, lr_actor, workspace_bytes);
  p.s_pi0 = 0;  // (the shared start-state table: the rows are drawn in the kernel)
  p.s_gpi = p.s_traj;
  p.s_n = B * T;
  p.s_P = B * T * d * d;
  RnPop rp = rn_pop_args(K, per_learner_net, net_stride, rn_seed, rn_call0, workspace_bytes, geom_dev);
  rp.s_state = B * (T + 1) * d;
  rp.s_action = B * T * d * d;
  rp.s_n = B * T;
  PopValidate pv;
  if (const int rc = pv.begin(K, d, theta, w, (flags & MFG_ROLLOUT_F64) ? MFG_PRECISION_F64 : MFG_PRECISION_MIXED, S(stream));
      rc != MFG_OK)
    return rc;
  PopControl pc;
  if (const int rc = pc.begin(p, theta, w, shift, !(flags & MFG_ROLLOUT_F64), S(stream)); rc != MFG_OK) return rc;
  rp.state = p.state;
  const ExtReward ext{net, P, 0, traj_offset * (uint64_t)T, &rp};
  for (int64_t e = 0; e < episodes; ++e) {
    lr_schedule(first_episode + e, constant, &p.sc, &p.sa);
    rp.call_j = (uint64_t)e + 1ull;
    const int rc = train_rollout_impl(mat_pi0, num_start, nullptr, B, d, T, theta, 0.0, 0.0, w, gamma, MFG_REWARD_EXTERNAL, 0,
                                      first_step + (uint32_t)(e * T), traj_offset, flags | MFG_TRAIN_APPLY, 0.0, 0.0, pi_traj,
                                      pi_last, reward, delta, g, G, reward_acc ? reward_acc + e : nullptr, workspace,
                                      workspace_bytes, S(stream), nullptr, &p, &ext);
    if (rc != MFG_OK) return rc;
    pc.retire();
    if (const int rv = pv.check(e, p); rv != MFG_OK) return rv;
  }
  return MFG_OK;
}

int mfg_train_rollout_irl(const float* mat_pi0, int64_t num_start, const int32_t* idx, int64_t B, int d, int T, double* theta,
                          double shift, double alpha_scale, double* w, double gamma, uint64_t seed, uint32_t first_step,
                          uint64_t traj_offset, int flags, double lr_critic, double lr_actor, const mfg_reward_net_t* net,
                          uint64_t rn_key, uint64_t rn_sample_offset, float* pi_traj, float* pi_last, float* P, float* reward,
                          double* delta, double* g, double* G, double* reward_acc, void* workspace, size_t workspace_bytes,
                          mfg_stream_t stream) {
  CHECK_IRL(REQUIRE(mat_pi0 && num_start > 0 && num_start <= 0x7FFFFFFF, "null / empty / oversized start-state table"), pi_traj);
  REQUIRE(B * (int64_t)T <= 0x7FFFFFFF, "B * T too large");
  const ExtReward ext{net, P, rn_key, rn_sample_offset, nullptr};
  return train_rollout_impl(mat_pi0, num_start, idx, B, d, T, theta, shift, alpha_scale, w, gamma, MFG_REWARD_EXTERNAL, seed,
                            first_step, traj_offset, flags, lr_critic, lr_actor, pi_traj, pi_last, reward, delta, g, G, reward_acc,
                            workspace, workspace_bytes, S(stream), nullptr, nullptr, &ext);
}

int mfg_train_episode_irl(float* pi_io, float* pi_scratch, int64_t B, int d, int T, double* theta, double shift,
                          double alpha_scale, double* w, double gamma, uint64_t seed, uint32_t first_step,
                          uint64_t traj_offset, int precision, double lr_critic, double lr_actor,
                          const mfg_reward_net_t* net, uint64_t rn_seed, uint64_t rn_call0, uint64_t rn_sample_offset,
                          float* P, float* reward, double* delta, double* g, double* G, double* reward_acc, void* workspace,
                          size_t workspace_bytes, mfg_stream_t stream) {
  return train_episode_irl_impl(nullptr, 0, pi_io, pi_scratch, B, d, T, theta, shift, alpha_scale, w, gamma, seed, first_step,
                                traj_offset, precision, lr_critic, lr_actor, net, rn_seed, rn_call0, rn_sample_offset, P, reward,
                                delta, g, G, reward_acc, workspace, workspace_bytes, stream);
}

int mfg_train_episode_irl_draw(const float* mat_pi0, int64_t num_start, float* pi_out, float* pi_scratch, int64_t B, int d, int T,
                               double* theta, double shift, double alpha_scale, double* w, double gamma, uint64_t seed,
                               uint32_t first_step, uint64_t traj_offset, int precision, double lr_critic, double lr_actor,
                               const mfg_reward_net_t* net, uint64_t rn_seed, uint64_t rn_call0, uint64_t rn_sample_offset,
                               float* P, float* reward, double* delta, double* g, double* G, double* reward_acc, void* workspace,
                               size_t workspace_bytes, mfg_stream_t stream) {
  if (!mat_pi0) return fail(MFG_EINVAL, "%s", "train_episode_irl_draw: null start-state table");
  return train_episode_irl_impl(mat_pi0, num_start, pi_out, pi_scratch, B, d, T, theta, shift, alpha_scale, w, gamma, seed,
                                first_step, traj_offset, precision, lr_critic, lr_actor, net, rn_seed, rn_call0, rn_sample_offset,
                                P, reward, delta, g, G, reward_acc, workspace, workspace_bytes, stream);
}

}  // extern "C"
