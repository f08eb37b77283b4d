/*
 * mfg_hip.h -- C ABI of the MI355X (gfx950) mean-field-game hot path.
 *
 * This is the drop-in boundary.  The reference has no FFI
 * layer: its hot path is the NumPy body of the methods of mfg_ac2.actor_critic /
 * ac_irl.AC_IRL.  Each entry point below replaces the batch-1 NumPy math of one of
 * those methods by one launch over B independent trajectories.  The Python classes
 * in discrete_mean_field_game_amd/ bind these symbols with ctypes and pass
 * tensor.data_ptr() of PyTorch-owned device memory.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no torch / C++ types.
 *   - every pointer is DEVICE memory unless the name ends in _host.
 *   - row-major; pi is [B,d] fp32, P is [B,d,d] fp32 (P[b][i][j] = prob. i -> j);
 *     theta and the critic weights w[F] live on the device as fp64 so that updates
 *     are stream ordered (no host round trip inside a rollout).
 *   - F = d(d+1)/2 + d + 1; w = [quadratic upper triangle row-major | linear | bias]
 *     (the order of mfg_ac2.py:325-344).
 *   - return 0 on success, a negative MFG_E* code otherwise; mfg_last_error() gives
 *     a thread-local message.  No allocation, no ownership transfer, no implicit
 *     synchronisation: all work is enqueued on `stream` (a hipStream_t).
 *   - all accumulations that feed rewards / TD errors / gradients are fp64.
 */
#ifndef MFG_HIP_H
#define MFG_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* mfg_stream_t; /* hipStream_t */

enum {
  MFG_OK = 0,
  MFG_EINVAL = -1,       /* bad argument (null pointer, d < 1, B < 0 ...) */
  MFG_ELAUNCH = -2,      /* HIP reported a launch/runtime error */
  MFG_EUNSUPPORTED = -3, /* shape outside the supported range (d > MFG_MAX_D) */
  MFG_EWORKSPACE = -4,   /* workspace too small */
  MFG_ERANGE = -5,       /* an earlier launch reported a numeric-range condition (mfg_status); sticky until cleared */
  MFG_ECOMM = -6         /* mfg_train_rollouts_dist: a launch / collective failed inside the episode loop and the RCCL communicator
                            has been ABORTED (ncclCommAbort, so that the peers fail instead of waiting): the handle is dead -- forget
                            it, do not destroy or use it again */
};

#define MFG_MAX_D 512

/* Global trajectory ids traj_offset + b live in [0, 2^48): the Philox counter keeps 48 bits of the id (low 32 in c2, high 16
 * in c3 below the draw block), so an id past 2^48 would draw another trajectory's actions.  Every entry point that takes a
 * traj_offset fails with MFG_EINVAL when traj_offset + B > MFG_TRAJ_ID_LIMIT. */
#define MFG_TRAJ_ID_LIMIT (1ull << 48)

/* reward_kind for mfg_step_given_P / mfg_rollout */
enum {
  MFG_REWARD_MFG_AC2 = 0,   /* sum_i pi_i sum_j P_ij^2 (pi_j - pi_i)   mfg_ac2.py:257-287 */
  MFG_REWARD_SYNTHETIC = 1, /* -1/2 sum_i pi_i ||P_i||^2               mfg_synthetic.py:249-265 */
  MFG_REWARD_EXTERNAL = 2   /* reward supplied by the caller (IRL reward net, ac_irl.py:683) */
};

/* precision of the per-element policy math (softplus / sigmoid / digamma / log):
 *   F64   every transcendental in fp64 (matches the fp64 oracle to ~1e-12 on identical inputs)
 *   MIXED fp32 hardware transcendentals, fp64 only for the sums (score g within ~1e-6 relative;
 *         rewards, transitions, values and TD errors are unaffected: they never use these functions) */
enum { MFG_PRECISION_F64 = 0, MFG_PRECISION_MIXED = 1 };

/* flags for mfg_rollout */
enum {
  MFG_ROLLOUT_WRITE_P = 1,     /* materialise P[B,T,d,d] (IRL / generate_trajectories, ac_irl.py:762) */
  MFG_ROLLOUT_TD = 2,          /* also compute reward, delta, g per step (train); else env only */
  MFG_ROLLOUT_DISCOUNT_POW = 4, /* bootstrap with running gamma^t (ac_irl.py:691,710) instead of gamma */
  MFG_ROLLOUT_F64 = 8           /* MFG_PRECISION_F64 instead of the default MFG_PRECISION_MIXED */
};

const char* mfg_last_error(void);
int mfg_abi_version(void);

/* Lane mapping of the d = 21 / 15 mixed-precision sampling launches (mfg_rollout, mfg_sample_dirichlet, the mfg_train_rollout*
 * and mfg_train_episode_irl* families; hot loop of mfg_ac2.py:478-526, ac_irl.py:664-712).  Two kernels produce the SAME bits:
 * the packed one (three / four trajectories per wavefront, a lane per matrix row) and -- round 6, ABI 17 -- one trajectory per
 * wavefront with three / four lanes per matrix row, whose serial chain per wave is 1.65x / 2.2x shorter; the library takes the
 * second where the packed kernel leaves the SIMDs under-occupied (d = 21: <= 16 trajectories per CU = 4 096 on an MI355X;
 * d = 15: <= 16 per CU, <= 12 with MFG_ROLLOUT_WRITE_P, <= 4 for single-step launches -- measured).
 * mode: 0 by batch size (default), 1 always packed, 2 one trajectory per wave wherever it supports the launch, 3 always packed and
 * in the packed kernel's GENERAL instantiation: a training rollout that asks for nothing optional (in-kernel mfg_ac2 reward, all
 * of pi_traj / reward / delta / g, no actions written out, constant bootstrap factor) otherwise runs an instantiation with those
 * options compiled out (k_core_small_lean: fewer registers, no scratch, the same bits).  Process-wide; returns the previous mode.
 * A measurement / test hook (A/B timing, bit-identity tests): results never depend on it. */
int mfg_set_core_mapping(int mode);

/* One-time per-device setup (fits the 12 KB h(z) = psi(softplus z) sigmoid z table used by the mixed-precision
 * score, one tiny launch + one device synchronise).  Optional: the first TD call does it lazily; call it
 * explicitly before capturing launches into a hipGraph. */
int mfg_init(void);

/* Device status word.  The mixed-precision SAMPLING kernels form e^{theta (pi_j - pi_i - shift)} as a product of two fp32
 * factors e^{theta (pi_j - 1/2)} e^{-theta (pi_i + shift - 1/2)}; their product, and the single fp32 exponential of the
 * mixed-precision kernels on given actions, is a normal fp32 number on every state while
 * |theta| (1 + |shift|) <= 86 (theta ~ 74 at the reference's shift 0.16; the reference trains at theta ~ 9).  theta lives
 * on the device, so the host cannot check it before a launch: a mixed-precision kernel that finds theta outside that range (or
 * not finite) sets MFG_STATUS_MIXED_RANGE in a host-visible status word and its outputs are unspecified (NaN where e^z
 * overflowed).  Every later call that
 * launches a mixed-precision SAMPLING kernel (sample / rollout / train entry points with MFG_PRECISION_MIXED) then fails
 * with MFG_ERANGE until mfg_clear_status() -- a diverged run stops with an error code instead of carrying NaNs.  The word is
 * one per CONTEXT (below; one per device and process for callers that never bind one): launches of MFG_PRECISION_F64 kernels and of kernels on given actions are
 * not refused (the latter report, but are never held up), so another model instance or thread on the device keeps working.  mfg_status() reads the word without
 * synchronising (synchronise the stream first to be sure a given launch has reported); it returns MFG_OK or MFG_ERANGE and
 * stores the bits in *bits_host (may be NULL). */
enum { MFG_STATUS_MIXED_RANGE = 1,
       MFG_STATUS_POP_NONFINITE = 2 /* per-learner words of a population control block only: theta or w not finite */ };
int mfg_status(unsigned* bits_host);
int mfg_clear_status(void);

/* Contexts ("no global mutable state except an opaque mfg_ctx*").  The mutable state a launch touches -- the
 * status word above, optionally an RCCL communicator -- belongs to a context; everything else the library keeps is immutable
 * (the h(z) table, per device) or passed in by the caller (workspaces).  Model: the CURRENT context of the calling thread,
 * like the current device of the HIP runtime -- mfg_ctx_bind(ctx) makes `ctx` the context of every entry point this thread
 * calls from then on (sampling launches report into ITS status word and are refused on ITS sticky bits; mfg_status /
 * mfg_clear_status act on it); mfg_ctx_bind(NULL) returns to the device's default context, which is what a thread that never
 * binds uses (the process-wide word of ABI <= 14: existing callers keep their behaviour).  Two model instances with a context
 * each cannot stop each other: a diverged run poisons only its own word.
 *   mfg_ctx_create      on the current device (initialises the device's table like mfg_init); one context per model instance
 *   mfg_ctx_destroy     also unbinds it from the calling thread and destroys an adopted communicator
 *   mfg_ctx_bind        thread-local, no device work; fails with MFG_EINVAL if ctx belongs to another device than the current
 *   mfg_ctx_status / mfg_ctx_clear_status   explicit-context forms of mfg_status / mfg_clear_status
 *   mfg_ctx_adopt_comm  hand a communicator from mfg_dist_init to the context (lifetime); mfg_ctx_comm returns it
 * Captured hipGraphs: the status-word address is baked into the captured kernel arguments (the capturing thread's context);
 * a replay reports into that word but is not refused on it -- check mfg_ctx_status after synchronising a replay. */
typedef struct mfg_ctx mfg_ctx_t;
int mfg_ctx_create(mfg_ctx_t** ctx_out);
int mfg_ctx_destroy(mfg_ctx_t* ctx);
int mfg_ctx_bind(mfg_ctx_t* ctx);
mfg_ctx_t* mfg_ctx_current(void);
int mfg_ctx_status(mfg_ctx_t* ctx, unsigned* bits_host);
int mfg_ctx_clear_status(mfg_ctx_t* ctx);
int mfg_ctx_adopt_comm(mfg_ctx_t* ctx, void* comm);
void* mfg_ctx_comm(mfg_ctx_t* ctx);

/* Population control block: per-learner activity states that live on the device, so that learners of a population call (the
 * mfg_train_*_pop entry points below) can be retired between two episodes -- early stop, divergence -- without a host round
 * trip and without stopping the others.  Device arrays, one entry per learner, owned by the caller:
 *   state [K]          0 active, 1 stopped (early stop), 2 failed; the blocks of a learner whose state is not 0 return at once
 *   status [K]         learner k's own status word: with a block, a mixed-precision launch books MFG_STATUS_MIXED_RANGE to the
 *                      learner whose theta left the range and not to the context, whose word stays 0
 *   theta_prev [K]     theta after the previous episode
 *   episodes_run [K]   += 1 after every episode the learner completed while active (the caller zeroes it)
 *   stop_criteria [K]  the learner stops once |theta - theta_prev| < stop_criteria[k] (AC_IRL.train, ac_irl.py:726); < 0: never
 * mfg_ctx_set_pop_control(ctx, block) binds a copy of the block to the context (NULL clears); every population training call
 * issued with that context bound then launches one small kernel (K waves) before its first episode and after every episode's
 * closing update.  For a learner still active it scans theta and the learner's w for non-finite values (MFG_STATUS_POP_NONFINITE),
 * in mixed precision tests !(|theta| (1 + |shift|) <= 86) (MFG_STATUS_MIXED_RANGE) and reads the learner's status word: any of
 * these -> the bits go to status[k] and state[k] = 2.  Otherwise, after an episode: episodes_run[k] += 1, state[k] = 1 when the
 * criterion is met, theta_prev[k] = theta (before the first episode: the checks and theta_prev only).  A call still enqueues all
 * its episodes and reads nothing back; the Philox step and the reward-call counters advance by the whole call for every learner.
 * Without a block the calls issue exactly the launches they always did.  Checked when the block is set and again before a
 * call launches anything: every pointer non-null, K the call's K (MFG_EINVAL). */
typedef struct mfg_pop_control {
  int32_t* state;
  unsigned* status;
  double* theta_prev;
  int32_t* episodes_run;
  const double* stop_criteria;
  int32_t K;
} mfg_pop_control_t;
int mfg_ctx_set_pop_control(mfg_ctx_t* ctx, const mfg_pop_control_t* block);

/* Host-side query: multiprocessor count and gcnArchName of the current device. */
int mfg_device_info(int* cu_count_host, char* arch_host, int arch_len);

/* Index of the quadratic feature pi_i*pi_j inside phi / w (host helper, integer
 * bookkeeping of itertools.combinations_with_replacement, mfg_ac2.py:333). */
int64_t mfg_feature_index(int i, int j, int d);
int64_t mfg_num_features(int d);

/* Bytes of scratch the gradient reductions need for N transitions of dimension d.  The first 64 bytes are a control
 * block (completion counter of the in-kernel finalisation): zero the workspace ONCE after allocating it
 * (hipMemset); every call leaves the control block zero again, so one workspace sized for the largest N serves
 * calls with any smaller N.  Everything behind the control block is scratch: no call reads a word there that it has not
 * written itself, so what an earlier call left behind never shows in a result.  The population forms take K such workspaces
 * back to back (slices of workspace_bytes each): every slice has a control block of its own, [k workspace_bytes,
 * k workspace_bytes + 64), zero before the call and left zero.  A workspace must not be shared by calls that can
 * run concurrently on different streams. */
size_t mfg_workspace_bytes(int64_t N, int d);

/* a9: pi0[b,:] = mat_pi0[idx[b],:]                       (mfg_ac2.py:466-469) */
int mfg_gather_start(const float* mat_pi0, int64_t num_start, const int32_t* idx, int64_t B, int d,
                     float* pi0, mfg_stream_t stream);

/* a9 on the device: the per-episode start-state draw  idx_row = randint(num_start_samples)  (mfg_ac2.py:466, ac_irl.py:655)
 * for B trajectories, from the counter-based generator of the action sampler instead of the host's np.random:
 *   Philox4x32-10, key = seed, counter = (0xFFFFFFFF, step, low 32 bits of the global trajectory id traj_offset + b,
 *   bits 32..47 of that id), x = first output word;  idx[b] = floor(x * num_start / 2^32)  (multiply-shift).
 * `step` = the Philox step of the episode's first env step, so an episode's draw and its actions share one counter space
 * (element id 0xFFFFFFFF is outside the action draws' i*d + j) and nothing but (seed, step, trajectory id) enters: the
 * draw does not depend on launch geometry or world size, and a resumed run redraws the same states.
 * Writes idx[B] (int32) and / or the gathered rows pi0[B,d] = mat_pi0[idx[b],:]; either may be NULL (mat_pi0 is only
 * needed for pi0).  The training entry points below draw the same rows inside their first kernel. */
int mfg_draw_start(const float* mat_pi0, int64_t num_start, int64_t B, int d, uint64_t seed, uint32_t step,
                   uint64_t traj_offset, int32_t* idx, float* pi0, mfg_stream_t stream);

/* a1: alpha[b,i,j] = softplus(theta (pi_j - pi_i - shift)) and its theta-derivative
 * (mfg_ac2.py:219-234; ac_irl.py:573-588).  Outputs fp64 [B,d,d]; either may be NULL. */
int mfg_alpha(const float* pi, int64_t B, int d, const double* theta, double shift, double* alpha,
              double* alpha_deriv, mfg_stream_t stream);

/* a2 (normalisation half): P = y / rowsum(y) with zeros -> 1e-20   (mfg_ac2.py:244-249).
 * Used when gamma variates are injected by the host (batch-1 reference RNG parity). */
int mfg_dirichlet_from_gamma(const float* y, int64_t B, int d, float* P, mfg_stream_t stream);

/* a1+a2: P[b] ~ prod_i Dirichlet(alpha[b,i,:] * alpha_scale)  (mfg_ac2.py:211-254).
 * Counter-based RNG: Philox4x32-10 keyed by `seed`, counter = (element i*d+j, step,
 * global trajectory id traj_offset + b, draw) so results do not depend on launch
 * geometry or world size. */
int mfg_sample_dirichlet(const float* pi, int64_t B, int d, const double* theta, double shift,
                         double alpha_scale, uint64_t seed, uint32_t step, uint64_t traj_offset, int precision,
                         float* P, mfg_stream_t stream);

/* Raw Philox4x32-10 blocks for counters (c0 = first_ctr + n, c1, c2, c3): out[n,4] u32.  Test hook
 * for bit-exact RNG parity. */
int mfg_philox_raw(uint64_t seed, uint32_t first_ctr, uint32_t c1, uint32_t c2, uint32_t c3, int64_t n,
                   uint32_t* out, mfg_stream_t stream);

/* a3+a4: pi_next = P^T pi, reward[b] (fp32) per reward_kind     (mfg_ac2.py:497-499).
 * reward may be NULL (transition only, ac_irl.py:679).  The HBM-bound kernel of the path: P is read once
 * (16-byte streaming loads when P is 16-byte aligned); with 16-byte aligned pi_next / reward, large batches
 * (d = 21, 15: >= ~10^5 transitions; d = 128, 256: >= 16 384) write their outputs as batched device-scope
 * bursts.  Results do not depend on which form runs.  pi_next must not alias pi. */
int mfg_step_given_P(const float* pi, const float* P, int64_t B, int d, int reward_kind, float* pi_next,
                     float* reward, mfg_stream_t stream);

/* a5: value[b] = phi(pi_b) . w (fp64 out)                     (mfg_ac2.py:290-322) */
int mfg_value(const float* pi, const double* w, int64_t B, int d, double* value, mfg_stream_t stream);
/* a5: phi[b,:] materialised (fp64 [B,F])                       (mfg_ac2.py:325-344) */
int mfg_features(const float* pi, int64_t B, int d, double* phi, mfg_stream_t stream);

/* a7: g[b] = sum_ij (-psi(alpha_ij) + psi(sum_j alpha_ij) + ln P_ij) alpha'_ij  (mfg_ac2.py:347-381).
 * pi_alpha is the state the concentrations are computed from (the reference reads the alpha left
 * behind by the previous sample_action; pass pi itself for the normal case).  Zeros of P count as
 * 1e-100 (mfg_ac2.py:369); P is not modified. */
int mfg_score(const float* pi_alpha, const float* P, int64_t B, int d, const double* theta, double shift,
              int precision, double* g, mfg_stream_t stream);

/* a5-a8 on given transitions: delta[b] = r + gamma_or_discount V(pi') - V(pi), g[b] as mfg_score,
 * and the batch sums G = [ sum_b delta_b phi(pi_b) (F) | sum_b delta_b g_b | sum_b r_b | B ] (fp64,
 * F+3 entries; accumulate != 0 adds onto the existing contents of G).  (mfg_ac2.py:501-522)
 * workspace: mfg_workspace_bytes(B, d) bytes; its control block is zero on entry and on return, the rest is scratch. */
int mfg_td_pg_accumulate(const float* pi, const float* pi_next, const float* P, const float* reward,
                         const double* w, const double* theta, double shift, double gamma_or_discount,
                         int64_t B, int d, int precision, double* delta, double* g, double* G, int accumulate,
                         void* workspace, size_t workspace_bytes, mfg_stream_t stream);

/* a6/a8: w += lr_critic * G_w / count ; theta += lr_actor * G_theta / count  (mfg_ac2.py:511-522).
 * count = G[F+2] (number of transitions summed, after any all-reduce).  If reward_acc is not NULL the mean
 * reward of the update, G[F+1]/count, is added to *reward_acc (total_reward += reward, mfg_ac2.py:526) so the
 * episode return never needs a host round trip. */
int mfg_apply_update(const double* G, int d, double lr_critic, double lr_actor, double* w, double* theta,
                     double* reward_acc, mfg_stream_t stream);

/* Fused T-step rollout with fixed (theta, w): a1-a5, a7 per step, state kept on chip.
 *   pi_traj[B,T+1,d] fp32 (pi_traj[:,0] = pi0; may be NULL for env-only rollouts), pi_last[B,d] = final state
 *   (contiguous, may be NULL), reward[B,T] fp32, delta[B,T], g[B,T] fp64,
 *   P_out[B,T,d,d] fp32 when MFG_ROLLOUT_WRITE_P; G as in mfg_td_pg_accumulate over all B*T
 *   transitions when MFG_ROLLOUT_TD.  first_step offsets the RNG step counter.
 *   reward_kind = MFG_REWARD_EXTERNAL (the IRL step: the reward network needs the sampled action first,
 *   ac_irl.py:679-691): `reward` is not touched, delta = gamma V(pi') - V(pi) WITHOUT the reward, G must be NULL;
 *   finish with mfg_grad_accumulate(add_reward = 1) once the rewards exist.
 *   workspace as for mfg_td_pg_accumulate(B*T) when G is given; may be NULL otherwise. */
int mfg_rollout(const float* pi0, int64_t B, int d, int T, const double* theta, double shift,
                double alpha_scale, const double* w, double gamma, int reward_kind, uint64_t seed,
                uint32_t first_step, uint64_t traj_offset, int flags, float* pi_traj, float* pi_last,
                float* reward, double* delta, double* g, float* P_out, double* G, int accumulate,
                void* workspace, size_t workspace_bytes, mfg_stream_t stream);

/* a9, one training update per episode (update_every = 'rollout'): start-state gather (mfg_ac2.py:466-469: row idx[b] of
 * the table mat_pi0[num_start,d], read inside the rollout kernel -- no separate gather launch), the fused T-step TD
 * rollout, the batch sums over all B*T transitions.  flags: MFG_ROLLOUT_F64 / MFG_ROLLOUT_DISCOUNT_POW as for
 * mfg_rollout, plus MFG_TRAIN_APPLY: also apply w += lr_critic G_w/N, theta += lr_actor G_theta/N and add the mean
 * reward to *reward_acc (if not NULL) inside the launch that finishes the sums -- a single-GPU update is then 2-3
 * launches.  Without MFG_TRAIN_APPLY G is complete on return: multi-GPU jobs all-reduce it and call mfg_apply_update.
 * Outputs as for mfg_rollout (pi_traj, reward, delta, g are required; pi_last may be NULL).
 * idx == NULL: the start rows are DRAWN inside the rollout kernel (mfg_draw_start with step = first_step) -- batched runs
 * need no host RNG, no index upload and, with several ranks, no broadcast in front of an episode.
 * workspace as for mfg_td_pg_accumulate(B*T). */
#define MFG_TRAIN_APPLY 16
int mfg_train_rollout(const float* mat_pi0, int64_t num_start, const int32_t* idx, int64_t B, int d, int T, double* theta,
                      double shift, double alpha_scale, double* w, double gamma, int reward_kind, uint64_t seed,
                      uint32_t first_step, uint64_t traj_offset, int flags, double lr_critic, double lr_actor,
                      float* pi_traj, float* pi_last, float* reward, double* delta, double* g, double* G,
                      double* reward_acc, void* workspace, size_t workspace_bytes, mfg_stream_t stream);

/* a9, the episode loop itself (mfg_ac2.py:460-526 with one update per episode): `episodes` training updates issued back to
 * back from native code -- per episode k: start states drawn in the rollout kernel (Philox step first_step + k T), fused
 * T-step TD rollout, batch sums, update with the reference's learning-rate schedule evaluated natively:
 *   e = first_episode + k;  constant != 0: lr_critic, lr_actor;  else lr_critic / (e+1), lr_actor / ((e+1) ln ln (e+20))
 * (mfg_ac2.py:511-522; pass the 1-indexed episode number for ac_irl.py:697-708), mean reward of the update added to
 * reward_acc[k] (may be NULL).  flags as for mfg_train_rollout (MFG_TRAIN_APPLY implied).  Single GPU: between two
 * episodes of a multi-GPU job sits an all-reduce, which stays with the caller (mfg_train_rollout per episode).
 * The output buffers hold the LAST episode's values on return.  workspace as for mfg_td_pg_accumulate(B*T). */
int mfg_train_rollouts(const float* mat_pi0, int64_t num_start, int64_t B, int d, int T, int64_t episodes, int64_t first_episode,
                       int constant, double* theta, double shift, double alpha_scale, double* w, double gamma, int reward_kind,
                       uint64_t seed, uint32_t first_step, uint64_t traj_offset, int flags, double lr_critic, double lr_actor,
                       float* pi_traj, float* pi_last, float* reward, double* delta, double* g, double* G, double* reward_acc,
                       void* workspace, size_t workspace_bytes, mfg_stream_t stream);

/* a9 on several GPUs: the update cycle of a rank without an update launch.  A multi-GPU update is
 *   rollout | batch sums | all-reduce(G) | w, theta += lr G / count              (mfg_ac2.py:511-522 for the global batch)
 * and its last step needs nothing but G: this entry point takes the all-reduced sums of the PREVIOUS update as G_pending
 * (NULL: none) and applies them while the rollout kernel stages its weights (d <= 64; a separate out-of-place launch
 * above): the parameters the rollout runs with -- and (theta_out, w_out), written by one block -- are
 *   theta + lr_actor_pending G_pending[F] / count,  w + lr_critic_pending G_pending[:F] / count,  count = G_pending[F+2],
 * bit for bit what mfg_apply_update would have produced in place; *reward_acc_pending += G_pending[F+1] / count.  The
 * outputs must be OTHER buffers than theta / w (blocks that start later still read the old values): callers ping-pong
 * two parameter sets.  Then as mfg_train_rollout without MFG_TRAIN_APPLY: G holds this rank's sums of the new update on
 * return (G may alias G_pending: it is written by a later launch).  A rank's cycle is rollout -> sums -> all-reduce, and
 * mfg_apply_update only once, after the last episode.  workspace as for mfg_td_pg_accumulate(B*T). */
int mfg_train_rollout_deferred(const float* mat_pi0, int64_t num_start, const int32_t* idx, int64_t B, int d, int T,
                               const double* theta, const double* w, const double* G_pending, double lr_critic_pending,
                               double lr_actor_pending, double* reward_acc_pending, double* theta_out, double* w_out, double shift,
                               double alpha_scale, double gamma, int reward_kind, uint64_t seed, uint32_t first_step,
                               uint64_t traj_offset, int flags, float* pi_traj, float* pi_last, float* reward, double* delta,
                               double* g, double* G, void* workspace, size_t workspace_bytes, mfg_stream_t stream);

/* a9 on several GPUs, natively: the episode loop of mfg_train_rollouts with ONE RCCL all-reduce of G per update issued by
 * this library on the caller's stream -- per episode [rollout kernel (applies the previous update, draws the start
 * states) | batch sums | ncclAllReduce(G)], then mfg_apply_update once after the last episode; no interpreter and no
 * framework call between the updates of a multi-GPU job.  RCCL is resolved at run time from the librccl.so the process
 * already holds (PyTorch's); MFG_EUNSUPPORTED where there is none.
 *   mfg_dist_unique_id : ncclGetUniqueId on ONE rank; ship the 128 bytes to the others (e.g. torch.distributed.broadcast)
 *   mfg_dist_init      : ncclCommInitRank on EVERY rank (collective; the current device is the rank's GPU)
 *   mfg_dist_all_reduce: in-place SUM of n doubles (the exchange of a per-step update; test hook)
 *   mfg_dist_abort     : ncclCommAbort -- frees the communicator WITHOUT the collective hand-shake of mfg_dist_destroy (a rank
 *                        whose peers failed or timed out during set-up; ABI 17)
 *   mfg_train_rollouts_dist: arguments as mfg_train_rollouts (B = this rank's shard, traj_offset = its first global
 *     trajectory id, G / count summed over the ranks) plus the second parameter set (theta_alt, w_alt) the updates
 *     ping-pong through; on return the parameters are in (theta, w) and identical on every rank.  MFG_ECOMM: the call
 *     aborted the communicator (see the error codes). */
typedef struct mfg_rccl_id { char bytes[128]; } mfg_rccl_id_t; /* ncclUniqueId */
int mfg_dist_available(void); /* 1 if librccl's entry points resolve in this process, else 0 (no error recorded) */
int mfg_dist_unique_id(mfg_rccl_id_t* id_host);
int mfg_dist_init(const mfg_rccl_id_t* id_host, int nranks, int rank, void** comm_out);
int mfg_dist_destroy(void* comm);
int mfg_dist_abort(void* comm);
int mfg_dist_all_reduce(void* comm, double* G, int64_t n, mfg_stream_t stream);
int mfg_train_rollouts_dist(void* comm, const float* mat_pi0, int64_t num_start, int64_t B, int d, int T, int64_t episodes,
                            int64_t first_episode, int constant, double* theta, double* w, double* theta_alt, double* w_alt,
                            double shift, double alpha_scale, double gamma, int reward_kind, uint64_t seed, uint32_t first_step,
                            uint64_t traj_offset, int flags, double lr_critic, double lr_actor, float* pi_traj, float* pi_last,
                            float* reward, double* delta, double* g, double* G, double* reward_acc, void* workspace,
                            size_t workspace_bytes, mfg_stream_t stream);

/* f1 (IRL): reward[b] = r_net(state_b, action_b), the reward network of networks.py:46-81 evaluated for B
 * transitions in one launch (ac_irl.py:683 evaluates it with batch 1 per env step).  fp32.  Weight layouts are
 * PyTorch's: conv1_w [k1*k1], conv2_w [f2][k2*k2], fc3_w [n3][d*d*f2] with the input index (pixel*f2 + channel)
 * (TF's NHWC flatten, networks.py:67), fc4_w [n4][n3+d] (inputs = [fc3 activations, state], networks.py:72),
 * out_w [n4].  keep_prob < 1 applies inverted dropout after fc3 and fc4 like tf.contrib.layers.dropout in
 * training mode (the reference leaves it on when the net serves as the RL reward); masks come from Philox keyed
 * by (seed, sample_offset + b).  Supported: d <= 32, f2 <= 2, n3, n4 <= 32, odd k1, k2 <= 7. */
int mfg_reward_net_forward(const float* state, const float* action, int64_t B, int d, int k1, int f2, int k2, int n3,
                           int n4, const float* conv1_w, const float* conv1_b, const float* conv2_w,
                           const float* conv2_b, const float* fc3_w, const float* fc3_b, const float* fc4_w,
                           const float* fc4_b, const float* out_w, const float* out_b, float keep_prob, uint64_t seed,
                           uint64_t sample_offset, float* reward, mfg_stream_t stream);

/* f1 (IRL), reward learning on the device: ONE call = one AC_IRL.update_reward (ac_irl.py:804-846) -- batch assembly,
 * forward of networks.py:46-81 over the sampled demonstration and generated transitions, the max-ent loss of
 * ac_irl.py:390-413
 *     L = -(1/demo_divisor) sum r_demo + log( (1/n_gen) sum_traj exp( sum_t r_gen ) ) [+ l1_l2(fc3_w) + l1_l2(fc4_w)],
 * its gradient and one tf.train.AdamOptimizer step (ac_irl.py:417-418;  lr_t = lr sqrt(1-beta2^t)/(1-beta1^t),
 * m = beta1 m + (1-beta1) g, v = beta2 v + (1-beta2) g^2, p -= lr_t m / (sqrt v + eps)), in two launches and no host
 * synchronisation.
 *   params / adam_m / adam_v [NP] fp32: ONE flat buffer per quantity, tensors in the order
 *     conv1_w [k1*k1] | conv1_b [1] | conv2_w [f2][k2*k2] | conv2_b [f2] | fc3_w [n3][f2*d*d] | fc3_b [n3] |
 *     fc4_w [n4][n3+d] | fc4_b [n4] | out_w [n4] | out_b [1]      (layouts of mfg_reward_net_forward;
 *     mfg_reward_net_param_offsets gives the 10 start offsets and NP as offsets_host[0..10]).
 *   The trajectories live in device-resident stores: *_state [rows, steps, d], *_action [rows, steps, d, d] fp32; the
 *   batch is the store rows demo_rows_host[n_demo] and gen_rows_host[n_gen] (HOST arrays, copied into the kernel
 *   arguments: no index upload; each <= MFG_RN_TRAIN_MAX_TRAJ).  Transition n of the batch (demonstrations first, row
 *   major over (trajectory, step)) draws its dropout masks from Philox key `seed`, counter (unit, 3 | 4, n, block 0) when
 *   keep_prob < 1, like mfg_reward_net_forward with sample_offset 0.
 *   flags & MFG_RN_TRAIN_GRAD_ONLY: stop at the gradient (grad [NP], required) -- the multi-GPU form: all-reduce grad,
 *   then mfg_reward_net_adam.  grad may also be given without the flag (gradient written AND update applied).
 *   stats (may be NULL) [4] <- loss, first term, second term, regulariser, evaluated at the weights BEFORE the update
 *   (what sess.run([r_train_op, loss, ...]) returns, ac_irl.py:846).
 *   workspace: mfg_reward_net_train_workspace_bytes(..., (n_demo + n_gen) * steps); contents are scratch.
 * Supported shapes as mfg_reward_net_forward; batch: (n_demo + n_gen) * steps <= 2048 transitions and
 * (n_demo + n_gen) * steps * (1 + n3) * 4 B <= 60 KB (MFG_EUNSUPPORTED beyond; the reference's batch is 150 transitions). */
#define MFG_RN_TRAIN_MAX_TRAJ 64
enum { MFG_RN_TRAIN_GRAD_ONLY = 1 };
int64_t mfg_reward_net_num_params(int d, int k1, int f2, int k2, int n3, int n4);
int mfg_reward_net_param_offsets(int d, int k1, int f2, int k2, int n3, int n4, int64_t* offsets_host);
size_t mfg_reward_net_train_workspace_bytes(int d, int k1, int f2, int k2, int n3, int n4, int64_t n_transitions);
int mfg_reward_net_train_step(float* params, float* adam_m, float* adam_v, int d, int k1, int f2, int k2, int n3, int n4,
                              const float* demo_state, const float* demo_action, const int32_t* demo_rows_host, int n_demo,
                              const float* gen_state, const float* gen_action, const int32_t* gen_rows_host, int n_gen, int steps,
                              int demo_divisor, float keep_prob, int l1l2, uint64_t seed, double lr, double beta1, double beta2,
                              double eps, int64_t adam_step, int flags, float* grad, float* stats, void* workspace,
                              size_t workspace_bytes, mfg_stream_t stream);
int mfg_reward_net_adam(float* params, float* adam_m, float* adam_v, const float* grad, int64_t n, double lr, double beta1,
                        double beta2, double eps, int64_t adam_step, mfg_stream_t stream);

/* mfg_reward_net_train_step with the importance weights of the max-ent IRL loss as the reference wrote it (ac_irl.py:292-321
 * z_j, :404-406 the weighted second term  log( 1/M sum_j z_j exp(sum_t r_j,t) ), commented out there because its linear-space
 * calc_z overflows).  gen_log_z: device fp64 [gen_capacity], ln z of the generated store's rows (mfg_traj_log_z_pop), indexed by
 * the same physical gen_rows.  The soft-max phase of the combine kernel forms trajectory j's weight as
 *   D_j = (double)S_j + gen_log_z[row_j];  mx = max_j D_j (fp64);  e_j = expf((float)(D_j - mx));  c_j = e_j / sum e;
 *   stats[2] = (float)(mx + log(sum e / n_gen)), formed in fp64 and rounded once
 * (fp64 until the maximum is gone: |ln z| ~ 1e4 with a spread of tens, so an fp32 ln z is off by 5e-4 before it reaches expf).
 * Everything else -- arguments, checks, per-sample coefficients, the fp64 batch sum, regulariser, Adam, MFG_RN_TRAIN_GRAD_ONLY
 * -- is mfg_reward_net_train_step's, which is this call with gen_log_z = NULL (then, or with n_gen = 0, the same launches
 * and the same bits); workspace as for mfg_reward_net_train_step.  A +inf entry (a generated P with an exact zero under p_floor = 0) poisons the update with NaN as it would
 * in the reference; nothing hides it. */
int mfg_reward_net_train_step_z(float* params, float* adam_m, float* adam_v, int d, int k1, int f2, int k2, int n3, int n4,
                                const float* demo_state, const float* demo_action, const int32_t* demo_rows_host, int n_demo,
                                const float* gen_state, const float* gen_action, const int32_t* gen_rows_host, int n_gen, int steps,
                                int demo_divisor, float keep_prob, int l1l2, uint64_t seed, double lr, double beta1, double beta2,
                                double eps, int64_t adam_step, int flags, float* grad, float* stats, void* workspace,
                                size_t workspace_bytes, const double* gen_log_z, mfg_stream_t stream);

/* f3: backward value recursion of the mfg_synthetic variant: V^n = r^n + P^n V^{n+1}, r^n_i = -1/2 ||P^n_i||^2,
 * V^T = 0 (mfg_synthetic.py:768-774) for P[B,T,d,d] -> V[B,T+1,d] (fp64), plus per (b,n) the consistency
 * metrics of evaluate_synthetic (diff_l1 = sum_ij |P_ij - value_ij|, :776-790) and, if diff_jsd != NULL, of
 * evaluate_synthetic_JSD (sum_i JSD(P_i, implied row i), entries <= 0 -> 1e-100, :858-880). */
int mfg_backward_value(const float* P, int64_t B, int T, int d, double* V, double* diff_l1, double* diff_jsd,
                       mfg_stream_t stream);

/* a6/a8 batch sums on their own: G (+)= [sum delta phi(pi) | sum delta g | sum reward | N] over the B*T samples
 * n = (b, s), pi_n = pi + b*stride_b + s*d (stride_b = (T+1)*d for a pi_traj, d for a plain [B,d] batch).
 * add_reward != 0: first delta_n <- delta_n + reward_n, written back -- the IRL step, where the rollout
 * (reward_kind = MFG_REWARD_EXTERNAL) leaves delta = gamma V(pi') - V(pi) and the reward network (ac_irl.py:683)
 * runs in between (:691).  Workspace as for mfg_td_pg_accumulate(B*T).
 * Any stride_b >= T*d and any alignment of pi are served (float4 staging at d >= 64 needs a 16-byte aligned pi and
 * stride_b % 4 == 0; otherwise the scalar staging path runs, same sums).  d <= 28: a skipped part stride_b - T*d of 2^23
 * floats or more, or T >= 2^22, takes the kernel's 64-bit address form (slower, same sums); T <= 2^31 - 65, a longer
 * trajectory is refused with MFG_EUNSUPPORTED (mfg_grad_apply and the batch sums of mfg_rollout likewise). */
int mfg_grad_accumulate(const float* pi, int64_t stride_b, double* delta, const double* g, const float* reward, int64_t B,
                        int T, int d, int add_reward, double* G, int accumulate, void* workspace, size_t workspace_bytes,
                        mfg_stream_t stream);

/* mfg_grad_accumulate (accumulate = 0) followed by mfg_apply_update, with the update applied inside the kernel that
 * finishes the sums (single GPU; mfg_ac2.py:511-522 / ac_irl.py:697-708 for the batch): the IRL step
 * rollout(EXTERNAL) -> reward net -> this call is three launches.  Workspace as for mfg_grad_accumulate. */
int mfg_grad_apply(const float* pi, int64_t stride_b, double* delta, const double* g, const float* reward, int64_t B, int T,
                   int d, int add_reward, double* G, double lr_critic, double lr_actor, double* w, double* theta,
                   double* reward_acc, void* workspace, size_t workspace_bytes, mfg_stream_t stream);

/* a9, native inner loop of train() with the reference's per-step updates (mfg_ac2.py:478-525) on ONE GPU: for
 * s < T: sample P ~ policy(pi), pi' = P^T pi, r, delta = r + gamma V(pi') - V(pi), g (a1-a7, one fused launch);
 * batch sums over the B trajectories (a6/a8); w += lr_critic G_w/B, theta += lr_actor G_theta/B,
 * *reward_acc += mean reward (if not NULL); pi <- pi'.  3T+... launches issued back to back from native code: no
 * host round trip, no interpreter between dependent small kernels.  pi_io [B,d]: start states in, final states out;
 * pi_scratch [B,d]; reward/delta/g [B] hold the last step's values on return; G [F+3]; workspace as for
 * mfg_td_pg_accumulate(B).  Philox steps first_step .. first_step+T-1.  Multi-GPU jobs keep the per-step
 * mfg_rollout(T=1) + all-reduce + mfg_apply_update sequence instead. */
int mfg_train_episode(float* pi_io, float* pi_scratch, int64_t B, int d, int T, double* theta, double shift,
                      double alpha_scale, double* w, double gamma, int reward_kind, uint64_t seed, uint32_t first_step,
                      uint64_t traj_offset, int precision, double lr_critic, double lr_actor, float* reward, double* delta,
                      double* g, double* G, double* reward_acc, void* workspace, size_t workspace_bytes,
                      mfg_stream_t stream);

/* a9, the episode loop with the reference's per-step updates (mfg_ac2.py:460-526): `episodes` x [start states drawn on the
 * device into pi_io (mfg_draw_start, step = first_step + k T) | mfg_train_episode], learning rates per episode as in
 * mfg_train_rollouts, reward_acc[k] += mean reward of every step's update of episode k (may be NULL).  Single GPU.
 * pi_scratch and workspace as for mfg_train_episode. */
int mfg_train_episodes(const float* mat_pi0, int64_t num_start, float* pi_io, float* pi_scratch, int64_t B, int d, int T,
                       int64_t episodes, int64_t first_episode, int constant, double* theta, double shift, double alpha_scale,
                       double* w, double gamma, int reward_kind, uint64_t seed, uint32_t first_step, uint64_t traj_offset,
                       int precision, double lr_critic, double lr_actor, float* reward, double* delta, double* g, double* G,
                       double* reward_acc, void* workspace, size_t workspace_bytes, mfg_stream_t stream);

/* Populations: K independent learners trained in lock-step, every launch of an episode serving all K (single GPU,
 * d <= 64, in-kernel reward).  Learner k of a population call gives, bit for bit in every output, what the single-learner
 * call (mfg_train_episodes / mfg_train_rollouts) gives with B = Bk, the same traj_offset and workspace_bytes, and learner
 * k's seed, theta, w, shift, alpha_scale and learning rates -- the reference's independent trainings (mfg_ac2.py:448-539,
 * one per grid point / seed / learning rate of mfg_ac2.gridsearch, mfg_ac2.py:673-689) in the launches of one.
 *   B = Bk trajectories per learner; per-learner scalars are device arrays [K]: seed (uint64), shift, alpha_scale,
 *   lr_critic, lr_actor (learner k's rates in episode e: lr_critic[k] x, lr_actor[k] x the schedule of mfg_train_rollouts).
 *   Learner-major arrays: theta [K], w [K,F], G [K,F+3], reward_acc [K,episodes] (may be NULL); step mode pi_io /
 *   pi_scratch [K,Bk,d], reward / delta / g [K,Bk]; rollout mode pi_traj [K,Bk,T+1,d], pi_last [K,Bk,d] (may be NULL),
 *   reward / delta / g [K,Bk,T].  mat_pi0 [num_start,d] is shared.
 *   workspace_bytes: ONE learner's slice, a multiple of 256 (the buffer holds K slices back to back).  Every slice is a
 *   workspace of mfg_workspace_bytes: its control block, bytes [k workspace_bytes, k workspace_bytes + 64) of the buffer, is
 *   zero on entry and on return (a retired learner's too), the rest of the slice is scratch.
 * Checked before anything is launched: 1 <= K <= MFG_POP_MAX_K, no null pointer, d <= 64 (MFG_EUNSUPPORTED beyond: one wave
 * per trajectory fills the machine there), an in-kernel reward_kind, the Philox step counter does not wrap (MFG_EINVAL);
 * the slice holds the update's partial rows (MFG_EWORKSPACE).  Rollout mode, d <= 28: the population form of the batch sums
 * has the 32-bit address form only (mfg_grad_accumulate), so an episode of T >= 2^22 steps is refused with MFG_EUNSUPPORTED --
 * by the update, i.e. after the episode's rollout has been enqueued (mfg_train_rollouts_pop, mfg_train_rollouts_irl_pop).
 * The sticky mixed-range status word (mfg_status) is per
 * device / context: one learner whose policy left the fp32 range blocks the population's next mixed-precision launch --
 * unless the bound context carries a population control block (mfg_ctx_set_pop_control), which books the condition to that
 * learner alone, retires it at the next episode boundary and lets the others run on. */
#define MFG_POP_MAX_K 65535
/* step mode (update_every = 'step', mfg_ac2.py:478-526): mfg_train_episodes for K learners; workspace: K slices, each with
 * its control block zero (above); pi_scratch is scratch */
int mfg_train_episodes_pop(const float* mat_pi0, int64_t num_start, float* pi_io, float* pi_scratch, int64_t B, int K, int d, int T,
                           int64_t episodes, int64_t first_episode, int constant, double* theta, const double* shift,
                           const double* alpha_scale, double* w, double gamma, int reward_kind, const uint64_t* seed,
                           uint32_t first_step, uint64_t traj_offset, int precision, const double* lr_critic,
                           const double* lr_actor, float* reward, double* delta, double* g, double* G, double* reward_acc,
                           void* workspace, size_t workspace_bytes, mfg_stream_t stream);
/* Step mode for small learners, resident (the reference's per-step updates, mfg_ac2.py:478-526): the parameter list and the
 * outputs of mfg_train_episodes_pop, with learner k held by ONE workgroup for the whole launch -- start draw, T x [env step |
 * row reduction + update], episode after episode, a block barrier between the phases; learners never communicate, so the
 * kernel has no fence wider than the workgroup and no spin, and is correct for any K.
 *   Bit identity: theta, w, G, pi_io, reward, delta, g and reward_acc of every learner equal, bit for bit, what
 *   mfg_train_episodes_pop leaves for the same arguments (given a workspace slice from mfg_workspace_bytes, with which that
 *   call forms its batch sums inside the step kernel); pi_scratch and the workspace are scratch.
 *   Launches: ceil(episodes / MFG_POP_RESIDENT_EPISODES) -- the learning-rate schedule of a launch's episodes is computed on
 *   the host and passed by value -- against episodes x (1 + 2 T) launches (+ a copy when T is odd) of mfg_train_episodes_pop.
 *   Shapes (mfg_pop_resident_supported, host only, no GPU: 1 / 0): d = 21 or 15, an in-kernel reward_kind and
 *   1 <= ceil(B / TB) <= MFG_POP_RESIDENT_MAX_TILES tiles of TB = 12 (d = 21) / 16 (d = 15) trajectories, i.e. B <= 768 /
 *   1 024: a functional cap (one row per slice of the row reduction, a bounded launch), not a performance claim.
 * Checked before anything is launched: everything mfg_train_episodes_pop checks; MFG_EUNSUPPORTED for another shape, and
 * when the bound context carries a population control block (retiring learners stays with the per-step launches);
 * MFG_EWORKSPACE when the slice does not hold the tiles' partial rows. */
#define MFG_POP_RESIDENT_EPISODES 64
#define MFG_POP_RESIDENT_MAX_TILES 64
int mfg_pop_resident_supported(int d, int64_t B, int reward_kind);
int mfg_train_episodes_pop_resident(const float* mat_pi0, int64_t num_start, float* pi_io, float* pi_scratch, int64_t B, int K,
                                    int d, int T, int64_t episodes, int64_t first_episode, int constant, double* theta,
                                    const double* shift, const double* alpha_scale, double* w, double gamma, int reward_kind,
                                    const uint64_t* seed, uint32_t first_step, uint64_t traj_offset, int precision,
                                    const double* lr_critic, const double* lr_actor, float* reward, double* delta, double* g,
                                    double* G, double* reward_acc, void* workspace, size_t workspace_bytes, mfg_stream_t stream);
/* rollout mode (one update per episode, mfg_ac2.py:460-526): mfg_train_rollouts for K learners (flags: MFG_ROLLOUT_F64 /
 * MFG_ROLLOUT_DISCOUNT_POW); workspace: K slices, each with its control block zero (above) */
int mfg_train_rollouts_pop(const float* mat_pi0, int64_t num_start, int64_t B, int K, int d, int T, int64_t episodes,
                           int64_t first_episode, int constant, double* theta, const double* shift, const double* alpha_scale,
                           double* w, double gamma, int reward_kind, const uint64_t* seed, uint32_t first_step,
                           uint64_t traj_offset, int flags, const double* lr_critic, const double* lr_actor, float* pi_traj,
                           float* pi_last, float* reward, double* delta, double* g, double* G, double* reward_acc,
                           void* workspace, size_t workspace_bytes, mfg_stream_t stream);

/* Population evaluation (evaluate / gridsearch, mfg_ac2.py:595-689; ac_irl.py:1495-1590 is the same with d = 15): the test
 * rollouts and the eight metrics of K policies in at most two launches, with no host synchronisation.
 *   emp32 / emp64 [N,L,d]: the N test files' first L rows (fp32 for the rollouts and the JSD, fp64 for the L1 metric).
 *   theta, shift, alpha_scale [K] fp64 and seed [K] uint64: learner k's policy; first_step: shared by all K.
 *   repeats R >= 1: learner k's trajectory j (0 <= j < N R) starts at emp32[j mod N, 0] and is keyed by Philox
 *   (seed[k], first_step + t, trajectory id j) -- bit for bit the states of mfg_rollout over those start rows (no TD).
 *   metrics [K,8] fp64, the CSV's column order: mean / std (ddof = 0) over the N R trajectories of l1_final, l1_mean,
 *   JSD_final, JSD_mean; L1 per step in fp64 against emp64, JSD per step as mfg_jsd(emp32 row, generated row); "final" is
 *   row L-1, "mean" the mean over the L rows.  Reduced in a fixed order, no floating-point atomics: learner k's row depends
 *   on its own inputs only, run to run and whatever K is.
 *   pi_traj [K, N R, L, d] fp32 or NULL (then the trajectories stay in the workspace).
 *   workspace: mfg_evaluate_pop_workspace_bytes(N, L, d, K, repeats, pi_traj != NULL) bytes; contents are scratch.
 * Checked before anything is launched: 1 <= K <= MFG_POP_MAX_K, d <= 64 (MFG_EUNSUPPORTED beyond, as for the populations),
 * L >= 2, N >= 1, repeats >= 1, no null pointer, the Philox step counter does not wrap (MFG_EINVAL), the workspace
 * (MFG_EWORKSPACE).  Mixed precision reports into and is refused on the bound context's status word like every sampling
 * launch. */
size_t mfg_evaluate_pop_workspace_bytes(int64_t N, int L, int d, int K, int repeats, int traj_given);
int mfg_evaluate_pop(const float* emp32, const double* emp64, int64_t N, int L, int d, int K, const double* theta,
                     const double* shift, const double* alpha_scale, const uint64_t* seed, uint32_t first_step, int repeats,
                     int precision, double* metrics, float* pi_traj, void* workspace, size_t workspace_bytes,
                     mfg_stream_t stream);

/* Ensemble forecast: R rollouts per start state of K policies, reduced on the device -- the expected histogram per hour, its
 * spread, order statistics per topic and the error against held-out rows per hour.  The reference draws this by hand from ONE
 * sample path (generate_trajectory, mfg_ac2.py:566-592, plotted by visualize_test, mfg_ac2.py:763, ac_irl.py:1663); its VAR
 * baseline returns a forecast with intervals (var.py:294-327).  At most THREE launches (the rollouts, the reduction over the
 * members, and with emp the curves), no host synchronisation.
 *   start32 [N,d]: the start states.  theta, shift, alpha_scale [K] fp64 and seed [K] uint64: learner k's policy; first_step:
 *   shared by all K.  H >= 2: rows per member, row 0 the start row.
 *   Members: learner k's member j (0 <= j < N R, R = repeats) belongs to start state n = j mod N, starts at start32[n] and is
 *   keyed by Philox (seed[k], first_step + t, trajectory id j): bit for bit the trajectories of mfg_evaluate_pop for an emp32
 *   whose row 0 is start32, i.e. of mfg_rollout over the R-fold tiled start rows (generate_trajectory's states).
 *   mean, std [K,N,H,d] fp64: over the R members of (k, n), per hour l and topic i; std with ddof = 0.  Both accumulate in fp64
 *   from the fp32 trajectory values, std in two passes (the mean first, then sum (x - mean)^2), in a fixed order that depends on
 *   (R, d) only.  No floating-point atomics: learner k's outputs depend on its own inputs only, whatever K is.
 *   quant [K,N,H,Q,d] fp32 (NULL allowed iff Q == 0): quant[k,n,l,q,i] is the order statistic of rank ranks[q] (0-based,
 *   ascending) among the R member values of the cell -- an element of the ensemble, not an interpolation, hence bit exact.
 *   Ties are legal (row 0 is all ties); ranks (a HOST array [Q]) may repeat and need not be sorted.
 *   curves [K,H,4] fp64 (NULL iff emp32 and emp64 are NULL): curves[k,l,:] = (l1_mean, l1_std, jsd_mean, jsd_std), mean and
 *   std (ddof = 0) over all N R members of the step's L1 (fp64, against emp64 [N,H,d]) and JSD (mfg_jsd(emp32 row, generated
 *   row)): the per-step terms of mfg_evaluate_pop's metrics (mfg_ac2.py:631-666), per step instead of per trajectory.
 *   pi_traj [K, N R, H, d] fp32 or NULL (then the trajectories stay in the workspace).
 *   workspace: mfg_forecast_pop_workspace_bytes(N, H, d, K, repeats, pi_traj != NULL) bytes; contents are scratch.
 * Checked before anything is launched: everything mfg_evaluate_pop checks, with H for L; 0 <= Q <= MFG_FORECAST_MAX_RANKS, every
 * rank in [0, repeats), emp32 and emp64 both given or both NULL, curves NULL exactly when they are (MFG_EINVAL); repeats <=
 * MFG_FORECAST_MAX_REPEATS (MFG_EUNSUPPORTED); the workspace (MFG_EWORKSPACE).  Mixed precision reports into and is refused
 * on the bound context's status word exactly as mfg_evaluate_pop. */
#define MFG_FORECAST_MAX_RANKS 8
#define MFG_FORECAST_MAX_REPEATS 1024
size_t mfg_forecast_pop_workspace_bytes(int64_t N, int H, int d, int K, int repeats, int traj_given);
int mfg_forecast_pop(const float* start32, int64_t N, int H, int d, int K, const double* theta, const double* shift,
                     const double* alpha_scale, const uint64_t* seed, uint32_t first_step, int repeats, int precision,
                     const int32_t* ranks, int Q, const float* emp32, const double* emp64, double* mean, double* std, float* quant,
                     double* curves, float* pi_traj, void* workspace, size_t workspace_bytes, mfg_stream_t stream);

/* Proper scores of an ensemble forecast: CRPS per topic, the energy score per histogram and the rank of the observation among
 * the members (Gneiting & Raftery, Strictly Proper Scoring Rules, Prediction, and Estimation, JASA 2007; kernel forms, beta = 1).
 * This goes beyond the reference, whose only quality numbers are the L1 / JSD tables of ONE sample path (evaluate,
 * mfg_ac2.py:595-670; the VAR baseline, var.py:330-416), and beyond mfg_forecast_pop, whose curves score single members too:
 * here the forecast DISTRIBUTION is scored.  The entry scores GIVEN members (no rollouts) in at most TWO launches, no host
 * synchronisation, no allocation, on `stream`.
 *   traj [K, N R, H, d] fp32: the members as mfg_forecast_pop writes pi_traj (R = repeats): member r of start row n is row
 *   r N + n.  emp32, emp64 [N,H,d]: the held-out rows y.  For cell (k, n, l) with members x_r and observation y:
 *   crps [K,N,H,d] fp64: 1/R sum_r |x_rc - y_c| - 1/(2 R^2) sum_{r,s} |x_rc - x_sc|, y from emp64, members widened to fp64.
 *     Order: lane r mod 64 of the column's wave adds |x_r - y| over r, r + 64, ... in member order, the 64 lane values go
 *     through an xor butterfly (offsets 32, 16, ..., 1); the double sum is 2 sum_i (2 i - R + 1) x_(i) over the ascending
 *     column (0-based), lane i mod 64 adding entries i, i + 64, ..., then the butterfly; crps = first / R - second / R^2.
 *   less, equal [K,N,H,d] int32: #{r : x_rc < y32_c} and #{r : x_rc == y32_c}, fp32 comparisons against emp32: exact.
 *   energy [K,N,H] fp64 or NULL (then the O(R^2 d) pass is skipped): 1/R sum_r ||x_r - y||_2 - 1/(2 R^2) sum_{r,s} ||x_r - x_s||_2,
 *     differences, squares and sqrt in fp64, the d squares of a norm added in column order (fused multiply-add).  Order: the
 *     members go in tiles of MFG_FORECAST_SCORE_TILE; every unordered pair r < s is taken once, by the thread (wave w, lane j)
 *     with r mod TILE = w (mod 4) and s mod TILE = j; a thread adds its norms to one fp64 partial in the order (tile of r,
 *     tile of s, r) ascending; the 64 lane partials go through the butterfly, the four wave totals are added in wave order and
 *     doubled by the formula: energy = first / R - (sum_{r<s}) / R^2.  The first sum: lane r mod 64 of wave 0 adds
 *     ||x_r - y|| over r, r + 64, ..., then the butterfly.
 *   summary [K,H,2] fp64: per policy and hour the mean of crps over (n, c) and of energy over n (NaN without energy): a cell's
 *     d CRPS values are added in column order, lane n mod 64 adds the cells n, n + 64, ..., then the butterfly -- an order that
 *     does not depend on K.
 *   A cell that holds a non-finite member or observation gets NaN scores and -1 counts (and its hour's summary is NaN); every
 *   other cell is as without it.  Policy k's outputs depend on policy k alone: the same bits whatever K is and run to run
 *   (no floating-point atomics).  With R = 1: crps = |x - y|, energy = ||x - y||.  When every member equals y and emp64 is
 *   fp32-representable, crps and energy are exactly 0, less 0 and equal R (hour 0 of a forecast).
 *   workspace: mfg_forecast_score_workspace_bytes(N, H, d, K, repeats) bytes, 8-byte aligned; contents are scratch.
 * Checked before anything is launched: no null pointer but energy, 1 <= K <= MFG_POP_MAX_K, N, d, repeats >= 1, H >= 2,
 * N H < 2^31 (MFG_EINVAL); d <= 64, repeats <= MFG_FORECAST_MAX_REPEATS (MFG_EUNSUPPORTED); the workspace (MFG_EWORKSPACE). */
#define MFG_FORECAST_SCORE_TILE 64
size_t mfg_forecast_score_workspace_bytes(int64_t N, int H, int d, int K, int repeats);
int mfg_forecast_score(const float* traj, int64_t N, int H, int d, int K, int repeats, const float* emp32, const double* emp64,
                       double* crps, int32_t* less, int32_t* equal, double* energy, double* summary, void* workspace,
                       size_t workspace_bytes, mfg_stream_t stream);

/* Population validation block: held-out checks INSIDE a population training call, so that a held-out learning curve, the best
 * iterate and "stop when the held-out metric stops improving" need no host round trip between episodes (the reference
 * evaluates only the iterate a training ends on, mfg_ac2.py:595-670).  Like the control block above it is bound to a context
 * by a setter that takes no stream, and the four population training calls (mfg_train_episodes_pop, mfg_train_rollouts_pop,
 * mfg_train_episodes_irl_pop, mfg_train_rollouts_irl_pop) act on it.  By value:
 *   N, L, repeats      as for mfg_evaluate_pop (N held-out files of L rows, R = repeats rollouts per file)
 *   period >= 1        a check runs after the closing update of the call's episode k (0-based) whenever (k + 1) % period == 0 --
 *                      with a control block also bound, after that episode's retire step
 *   column             in [0, 10): the curve column the best iterate is selected by (smaller is better); 8, 9 need with_score
 *   with_score         0 / 1: also score the members just rolled out (mfg_forecast_score with the energy score)
 *   patience >= 0      > 0: a learner whose `column` has not improved in `patience` consecutive checks is stopped (state 1, as the
 *                      early stop); needs a control block bound when a call is made
 *   first_step         the Philox step of EVERY check's rollouts (steps first_step .. first_step + L - 2): common random numbers
 *                      along the curve, so two checks differ by theta alone
 *   max_checks >= 1    rows of `curve` per learner
 *   K                  the population size
 *   workspace_bytes    >= mfg_pop_validate_workspace_bytes(N, L, d, K, repeats, with_score) for the d of the call
 * Device arrays, owned and initialised by the caller:
 *   emp32, emp64 [N,L,d]      the held-out rows (fp32 for the rollouts, the JSD and the ranks; fp64 for L1, CRPS, energy)
 *   curve [K, max_checks, 10] fp64: row c of learner k is its c-th check.  Columns 0-7: the eight metrics of mfg_evaluate_pop in
 *                             the CSV's column order, bit for bit what that call returns for the learner's theta at the check (the
 *                             same kernels, the call's shift / alpha_scale / seed arrays and precision).  Column 8 (9): the mean over
 *                             the hours l = 1 .. L-1 of summary[k,l,0] (summary[k,l,1]) of mfg_forecast_score on the check's
 *                             members -- CRPS (energy score) --, added in hour order in fp64 by one lane and divided by L - 1;
 *                             NaN without with_score
 *   checks [K] int32          += 1 per check the learner took part in (the caller zeroes it); a row is written only while
 *                             checks[k] < max_checks, the best tracking below goes on past that
 *   best_value [K] fp64       the smallest finite value of `column` so far (the caller sets +inf)
 *   best_check [K] int32      the check it was seen at (the caller sets -1); the EARLIEST minimum wins (strict <)
 *   since_best [K] int32      checks since then (the caller zeroes it)
 *   best_theta [K], best_w [K,F] fp64: theta[k] and w[k,:] as they were at that check
 *   workspace                 scratch (the members, the metrics and the scores of one check), 8-byte aligned
 * A check is three groups of launches on the call's stream, no host read, no allocation: the two launches of mfg_evaluate_pop,
 * with with_score the two of mfg_forecast_score, and k_pop_validate_select (one wave per learner).  A learner that is not active
 * at the check (state[k] != 0 under a control block) is skipped entirely: its blocks of every launch return at once and none of
 * its arrays is touched.  Mixed precision: a check reports into and is refused on the status word exactly as mfg_evaluate_pop;
 * under a control block it books to the learner, as the training launches do.  Without a block the calls issue exactly the
 * launches they always did.
 * Checked when the block is set: MFG_EINVAL for a null context or pointer, period < 1, max_checks < 1, patience < 0, column
 * outside [0, 10) or >= 8 without with_score, with_score not 0 / 1, K outside [1, MFG_POP_MAX_K], N < 1, L < 2, repeats < 1, N L
 * or N repeats >= 2^31, first_step + L - 1 wrapping; MFG_EUNSUPPORTED for repeats > MFG_FORECAST_MAX_REPEATS with with_score.
 * Checked again before a call launches anything: MFG_EINVAL when K differs from the call's K or patience > 0 without a control
 * block; MFG_EWORKSPACE when workspace_bytes is below mfg_pop_validate_workspace_bytes for the call's d.
 * mfg_train_episodes_pop_resident refuses a bound validation block with MFG_EUNSUPPORTED, as it refuses a control block.
 * mfg_pop_validate_workspace_bytes is 0 for a degenerate shape, never below mfg_evaluate_pop_workspace_bytes(N, L, d, K,
 * repeats, 0) otherwise, and larger with with_score. */
typedef struct mfg_pop_validate {
  const float* emp32;
  const double* emp64;
  double* curve;
  int32_t* checks;
  double* best_value;
  int32_t* best_check;
  int32_t* since_best;
  double* best_theta;
  double* best_w;
  void* workspace;
  size_t workspace_bytes;
  int64_t N;
  int32_t L, repeats;
  int32_t period, column;
  int32_t with_score, patience;
  int32_t max_checks, K;
  uint32_t first_step;
} mfg_pop_validate_t;
#define MFG_POP_VALIDATE_COLUMNS 10
int mfg_ctx_set_pop_validate(mfg_ctx_t* ctx, const mfg_pop_validate_t* block);
size_t mfg_pop_validate_workspace_bytes(int64_t N, int L, int d, int K, int repeats, int with_score);

/* Population evolve block: population-based training (Jaderberg et al. 2017, truncation selection) on the device.  After a
 * held-out check of the validation block above, the worst learners take over the parameters of one of the best (exploit) and
 * go on with perturbed learning rates (explore), with no host round trip: the K values never leave the device.  Like the two
 * blocks above it is bound to a context by a setter that takes no stream; the two forward population calls
 * (mfg_train_episodes_pop, mfg_train_rollouts_pop) act on it, on the stream they are given.  It needs a validation block bound
 * at the call.  By value:
 *   every >= 1         a step runs behind k_pop_validate_select of the call's validation check c (0-based) whenever
 *                      (c + 1) % every == 0; its index is s = (c + 1) / every - 1
 *   n_top, n_bottom    >= 1, n_top + n_bottom <= K: the donors are the n_top best, the receivers the n_bottom worst learners
 *   perturb            bit 0: the critic rate is perturbed, bit 1: the actor rate; a rate whose bit is clear is copied
 *   factor_down, factor_up   finite, > 0 (e.g. 0.8, 1.25)
 *   lr_critic_min <= lr_critic_max, lr_actor_min <= lr_actor_max, every bound > 0: the clamp of a perturbed rate
 *   seed               key of the step's Philox draws
 *   max_steps >= 1     steps the logs hold per learner; a call needs (episodes / period) / every <= max_steps
 *   K                  the population size
 * Device arrays, owned by the caller:
 *   lr_critic, lr_actor [K] fp64   the SAME arrays the training call is given: a step writes them between two episodes, and the
 *                                  launches of the following episodes read the new rates
 *   order [K] int32                scratch: order[r] = the active learner of rank r at the last step.  A step writes the slots
 *                                  r < A and reads only those back, as learner indices (the donors): what the caller leaves in
 *                                  the array is never read
 *   active [1] int32               scratch: the number A of active learners at the last step
 *   rank, parent [K, max_steps] int32   logs (the caller sets -1)
 *   lr_log [K, max_steps, 2] fp64  log: (critic, actor) rate after the step (the caller sets NaN)
 * A step.  Learner k's value is column `column` of the validation block's row of that check, formed from the check's metrics /
 * summary in the validation workspace by the device function k_pop_validate_select forms it with.  The active learners are all
 * learners without a control block, and those with state[k] == 0 (after the check's patience stop) under one.  They are ordered
 * ascending by the key (value not finite, value, k), in which a non-finite value counts as +inf: a strict total order; ties go
 * to the smaller index, non-finite values come last in index order.  rank[k, s] is learner k's position in that order,
 * order[rank] = k, active[0] = A.  A learner that is not active is skipped entirely: none of its arrays is touched, its log
 * entries stay -1 / NaN.
 * Learners are replaced only when A >= n_top + n_bottom and the learner of rank n_top - 1 has a finite value (every donor's
 * value is then finite); otherwise the step only logs.  When they are, every active learner k with rank >= A - n_bottom draws
 * the Philox4x32-10 block of counter (0xFFFFFFFE, s, k, 0) under the key (seed low, seed high) -- element id 0xFFFFFFFE lies
 * outside the action draws and the start draw's 0xFFFFFFFF -- for the words x0 .. x3, and
 *   donor = order[floor(x0 n_top / 2^32)]      (the integer form of mfg_draw_start)
 *   exploit: theta[k], w[k,:] and the validation block's best_value, best_check, since_best, best_theta, best_w[k,:] become the
 *            donor's (the best iterate of the lineage); with a control block theta_prev[k] = theta[donor], so that the next
 *            retire step compares the new theta with the donor's and not with the replaced learner's
 *   explore: lr_critic[k] = min(max(lr_critic[donor] f, lr_critic_min), lr_critic_max) in fp64 with f = factor_up when
 *            x1 >> 31 is 1, else factor_down; lr_actor[k] by the same rule with x2 >> 31 and the actor bounds; a rate whose
 *            perturb bit is clear becomes the donor's unchanged
 *   parent[k, s] = donor.  The learner keeps its own seed, shift and alpha_scale.
 * Every other active learner gets parent[k, s] = k.  lr_log[k, s, :] holds every active learner's rates after the step.
 * Donor and receiver ranks are disjoint, a receiver writes only its own rows and reads only a donor's: no race, no fence.
 * A step is two launches on the call's stream (k_pop_evolve_rank, k_pop_evolve_apply), no atomics, no host read, no allocation.
 * Without a block the calls issue exactly the launches they always did.
 * Checked when the block is set: MFG_EINVAL for a null context or pointer, every / n_top / n_bottom < 1, n_top + n_bottom > K, K
 * outside [1, MFG_POP_MAX_K], max_steps < 1, a factor that is not finite or <= 0, a bound pair with min > max or min <= 0 (or
 * not finite), perturb outside [0, 3].  Checked again before a call launches anything: MFG_EINVAL when K differs from the call's
 * K, when no validation block is bound, when lr_critic / lr_actor are not the call's pointers, or when max_steps <
 * (episodes / period) / every.  mfg_train_episodes_pop_resident, mfg_train_episodes_irl_pop and mfg_train_rollouts_irl_pop
 * refuse a bound block with MFG_EUNSUPPORTED: the resident kernel reads its rates once per launch, and IRL learners may carry
 * different reward networks, which an exploit would have to copy too. */
typedef struct mfg_pop_evolve {
  double* lr_critic;
  double* lr_actor;
  int32_t* order;
  int32_t* active;
  int32_t* rank;
  int32_t* parent;
  double* lr_log;
  uint64_t seed;
  double factor_down, factor_up;
  double lr_critic_min, lr_critic_max, lr_actor_min, lr_actor_max;
  int32_t every, n_top, n_bottom, perturb;
  int32_t max_steps, K;
} mfg_pop_evolve_t;
int mfg_ctx_set_pop_evolve(mfg_ctx_t* ctx, const mfg_pop_evolve_t* block);

/* Finite populations: a member is ONE population of A agents (1 <= A <= MFG_AGENTS_MAX) instead of the mean-field limit
 * pi' = P^T pi that every other entry rolls.  Its state is counts [d] int32 (d <= 64) summing to A; each agent of topic i draws
 * its next topic from row P[i,:] of the member's action, so the histogram carries sampling noise of order 1 / sqrt(A) on top of
 * the policy's -- the N-player game whose limit the mean-field forecast is.  The reference has no such path.  Everything is
 * integer but the thresholds, which are defined operation by operation: the results are the same bits on every run and layout.
 *   Histogram row: pi_i = (float)((double)counts_i / (double)A).
 *   One step of the member with global id j under seed s at Philox step `step`, given its action P [d,d] fp32:
 *   1. thresholds: S_ic = the sequential sum of (double)P[i,0..c] in column order (adds only), t_ic = floor(S_ic / S_i,d-1 2^32)
 *      as a 64-bit integer, clamped to [0, 2^32]; t_i,d-1 = 2^32 exactly.
 *   2. agent a (0 <= a < counts_i) of topic i reads word a mod 4 (x, y, z, w) of philox4x32_10 with counter
 *      c0 = 0x80000000 | (i << 22) | (a >> 2), c1 = step, c2 = (uint32)j, c3 = (j >> 32) & 0xFFFF and key (s low, s high):
 *      draw block 0, a c0 range above the action element ids (< 2^18) and never the start draw's 0xFFFFFFFF.
 *   3. the agent moves to the first column c with word < t_ic (64-bit comparison: t = 2^32 accepts 0xFFFFFFFF, t = 0 nothing);
 *      moves[i,c] counts these moves and counts'_c = sum_i moves[i,c], which sum to A again.
 *   4. a row with counts_i > 0 whose S_i,d-1 is not finite or <= 0, or a count outside [0, A], fails the member: its counts' and
 *      moves are -1 and its histogram row is NaN; every other member is as without it.
 *
 * mfg_agents_step_pop: the given-P building block (the counterpart of mfg_step_given_P) in ONE launch, no workspace, no
 * allocation, no synchronisation, on `stream`.
 *   counts [K,B,d] int32, P [K,B,d,d] fp32; member b of group k has id traj_offset + b and seed seed[k] (a device array [K]).
 *   counts_next [K,B,d] int32 (may be `counts`); pi_next [K,B,d] fp32 or NULL; moves [K,B,d,d] int32 or NULL.
 *   Group k's outputs depend on group k alone.
 * Checked before launch: no null pointer but pi_next / moves, 1 <= K <= MFG_POP_MAX_K, 0 <= B < 2^31, d >= 1, 1 <= agents <=
 * MFG_AGENTS_MAX, traj_offset + B <= MFG_TRAJ_ID_LIMIT (MFG_EINVAL); d <= 64 (MFG_EUNSUPPORTED).
 *
 * mfg_forecast_agents_pop: mfg_forecast_pop with finite-population members.  Its arguments are mfg_forecast_pop's with
 * counts0 [N,d] int32 (the start counts, each row summing to `agents`) for start32, `agents`, and two more outputs that may be
 * NULL: counts_traj [K, N R, H, d] int32 and actions [K, N R, H-1, d, d] fp32.  Member j of learner k (start row j mod N) at
 * step t forms pi from its counts, draws P from that row exactly as mfg_forecast_pop's members do -- Philox keys (seed[k],
 * first_step + t, j): actions[k,j,t] is mfg_sample_dirichlet's row j on pi_traj[k,:,t] -- and resamples its agents as above
 * with step = first_step + t.  pi_traj rows are the histogram rows of counts_traj; a member that fails at step t has NaN rows
 * and -1 counts from row t + 1 on (its later actions are drawn from its last valid row).  mean, std, quant and curves are
 * mfg_forecast_pop's, by the same kernels on pi_traj.  Launches: one for row 0, then the sampling kernel over all K N R members
 * and the agents kernel per step -- 2 (H - 1) whatever K is -- and the one or two reductions.
 *   workspace: mfg_forecast_agents_pop_workspace_bytes(N, H, d, K, repeats, pi_traj != NULL, counts_traj != NULL) bytes, 8-byte
 *   aligned; contents are scratch.
 * Checked before anything is launched: everything mfg_forecast_pop checks, 1 <= agents <= MFG_AGENTS_MAX (MFG_EINVAL).  Mixed
 * precision reports into and is refused on the bound context's status word exactly as mfg_forecast_pop: the word is read once,
 * before the first launch; a policy that leaves the range INSIDE the call does not stop it -- its actions are unspecified, so
 * each of its members fails or stays a histogram of its agents, every other policy's outputs are complete, the call returns
 * MFG_OK and the next mixed-precision call is refused. */
#define MFG_AGENTS_MAX (1 << 24)
int mfg_agents_step_pop(const int32_t* counts, const float* P, int64_t B, int d, int K, int agents, const uint64_t* seed,
                        uint32_t step, uint64_t traj_offset, int32_t* counts_next, float* pi_next, int32_t* moves,
                        mfg_stream_t stream);
size_t mfg_forecast_agents_pop_workspace_bytes(int64_t N, int H, int d, int K, int repeats, int traj_given, int counts_given);
int mfg_forecast_agents_pop(const int32_t* counts0, int64_t N, int H, int d, int K, int agents, const double* theta,
                            const double* shift, const double* alpha_scale, const uint64_t* seed, uint32_t first_step, int repeats,
                            int precision, const int32_t* ranks, int Q, const float* emp32, const double* emp64, double* mean,
                            double* std, float* quant, double* curves, float* pi_traj, int32_t* counts_traj, float* actions,
                            void* workspace, size_t workspace_bytes, mfg_stream_t stream);

/* Distribution summary of R rows of N fp32 values in ONE launch, one workgroup per row: what plot_reward_distribution and
 * its two siblings (ac_irl.py:1046-1263) take from plt.hist (np.histogram, :1116-1119) and gaussian_kde (:1087-1100) for each
 * of their reward sets.  Row r is values[r stride .. r stride + N), stride >= N; everything below is on x = (double)values.
 *   moments [R,6] fp64: number of values the histogram kept (N without a range), min, max, mean (a fixed-order sum),
 *   variance (ddof = 1, two passes: sum (x - mean)^2 / (N - 1)), KDE bandwidth variance c = variance N^(-2/5) (gaussian_kde's
 *   Scott factor squared).  Mean and variance are over all N values; the range only affects the histogram.
 *   counts [R,bins] int64, edges [R,bins+1] fp64: those of np.histogram(x, bins) on the fp64 array, with use_range those of
 *   np.histogram(x, bins, range=(lo, hi)): first = min, last = max (lo, hi with a range); first - 0.5, last + 0.5 if they are
 *   equal; step = (last - first) / bins; edge_i = fl(fl(i step) + first) for i < bins (two roundings), edge_bins = last.  A
 *   value is counted in bin i when edge_i <= x < edge_(i+1), the last bin closed on the right; values outside a given range
 *   are dropped.  The index is NumPy's guess ((x - first) / (last - first)) bins, truncated, corrected against the exact edges.
 *   density [R,G] fp64 (NULL allowed iff G == 0): scipy.stats.gaussian_kde(x)(grid) on grid = linspace(x_lo, x_hi, G), i.e.
 *   density_g = sum_n exp(-(g - x_n)^2 / (2c)) / (N sqrt(2 pi c)), fp64, the terms added in ascending n.
 *   status [R] int32 bit flags: MFG_DIST_NONFINITE: the row holds a non-finite value -- its moments, edges and density are NaN
 *   and its counts zero, every other row is as without it; MFG_DIST_NO_KDE: N < 2 or variance == 0 (gaussian_kde raises
 *   there) -- the density is NaN, the rest of the row stands.
 * Row r's outputs depend on row r alone and are the same bits whatever R is; no floating-point atomics.
 * workspace: mfg_row_distribution_workspace_bytes(R, N, bins, G) bytes (at present 0: NULL is then allowed).
 * Checked before anything is launched: no null pointer, R >= 1, 1 <= N < 2^31, stride >= N, 1 <= bins <= MFG_DIST_MAX_BINS,
 * 0 <= G <= MFG_DIST_MAX_GRID, finite lo < hi with use_range, finite x_lo, x_hi with G > 0 (MFG_EINVAL); the workspace
 * (MFG_EWORKSPACE).  No allocation, no synchronisation; runs on `stream`. */
#define MFG_DIST_MAX_BINS 1024
#define MFG_DIST_MAX_GRID 4096
#define MFG_DIST_NONFINITE 1
#define MFG_DIST_NO_KDE 2
size_t mfg_row_distribution_workspace_bytes(int R, int64_t N, int bins, int G);
int mfg_row_distribution(const float* values, int R, int64_t N, int64_t stride, int bins, int use_range, double lo, double hi,
                         int G, double x_lo, double x_hi, double* moments, int64_t* counts, double* edges, double* density,
                         int32_t* status, void* workspace, size_t workspace_bytes, mfg_stream_t stream);

/* Mean action matrix of K learners in TWO launches: np.mean(np.asarray(actions), axis=0) of plot_action_heatmap
 * (ac_irl.py:1276-1289), for every learner at once.
 *   action: learner k's N matrices [N,d,d] fp32 start at action + k s_action; s_action = 0: one input shared by all K.
 *   mean [K,d,d] fp64.
 *   launch 1, grid (chunks, K): thread e mod 256 owns matrix element e (consecutive threads, consecutive floats) and adds its
 *   chunk of n in ascending n in fp64 into partials [K,chunks,d d] in the workspace; launch 2 adds a learner's partials (16
 *   runs of chunks, each in chunk order, the run totals in run order) and divides by N.  The number of chunks depends on N
 *   alone, so learner k's mean is the same bits whatever K is.  The input is read once (K N d d 4 bytes).
 *   workspace: mfg_action_mean_pop_workspace_bytes(K, N, d) bytes; contents are scratch.
 * Checked before anything is launched: no null pointer, 1 <= K <= MFG_POP_MAX_K, N >= 1, d >= 1, s_action = 0 or >= N d d
 * (MFG_EINVAL); d <= 64 (MFG_EUNSUPPORTED); the workspace (MFG_EWORKSPACE). */
size_t mfg_action_mean_pop_workspace_bytes(int K, int64_t N, int d);
int mfg_action_mean_pop(const float* action, int64_t s_action, int K, int64_t N, int d, double* mean, void* workspace,
                        size_t workspace_bytes, mfg_stream_t stream);

/* Backward-equation check of K groups of trajectories, reduced on the device: the scoring of the reference's synthetic sweep
 * (evaluate_synthetic / evaluate_synthetic_JSD, mfg_synthetic.py:741-899, called once per learner by its __main__, :902-925).
 * mfg_consistency_given, TWO launches on given actions:
 *   P [K,M,T,d,d] fp32: K groups of M trajectories of T row-stochastic action matrices.
 *   launch 1: per trajectory the reverse-time scan V^n = r^n + P^n V^{n+1}, r^n_i = -1/2 ||P^n_i||^2, V^T = 0 (:768-774), and
 *   per hour n  l1 = sum_ij |P_ij - value_ij| (:776-790)  and  jsd = sum_i JSD(P_i, implied row i) (:858-880), where implied
 *   row i is V^n_j - V^n_i off the diagonal and 1 - (sum_j V^n_j - d V^n_i) on it; in the JSD every entry <= 0 of either
 *   argument counts as 1e-100 and P, Q and M are renormalised (mfg_backward_value's formulas).  fp64 throughout, in an order
 *   that depends on (d, T) only.
 *   launch 2: metrics [K,4] fp64 = (l1_mean, l1_std, jsd_mean, jsd_std): mean and std (ddof = 0, np.mean / np.std at :800-801,
 *   :887-888) over the group's M T values, two passes in a fixed order.  No floating-point atomics: group k's outputs depend
 *   on group k's inputs only.
 *   steps [K,M,T,2] fp64 (l1, jsd per hour) or NULL (then they stay in the workspace); V [K,M,T+1,d] fp64 or NULL (then V is
 *   not written to memory at all).
 *   workspace: mfg_consistency_given_workspace_bytes(K, M, T, steps != NULL) bytes (0 with steps: NULL is then allowed);
 *   contents are scratch.
 * mfg_consistency_pop, THREE launches, no host synchronisation: the actions are those of K policies' rollouts.
 *   start32 [N,d], theta / shift / alpha_scale [K] fp64, seed [K] uint64, first_step, repeats R, precision: as for
 *   mfg_forecast_pop -- learner k's member j (0 <= j < N R) starts at start32[j mod N] and is keyed by Philox (seed[k],
 *   first_step + t, j): the actions and states of mfg_rollout over the R-fold tiled start rows (generate_trajectory,
 *   mfg_ac2.py:566-592).  H >= 2 hours per member, T = H - 1 action matrices; M = N R.
 *   metrics, steps, V: as above.  actions [K, N R, T, d, d] fp32 or NULL, pi_traj [K, N R, H, d] fp32 or NULL (then in the
 *   workspace).  workspace: mfg_consistency_pop_workspace_bytes(N, H, d, K, repeats, steps != NULL, actions != NULL,
 *   pi_traj != NULL) bytes; contents are scratch.
 * Checked before anything is launched: no null pointer, 1 <= K <= MFG_POP_MAX_K, H >= 2 (T >= 1), N, M, repeats >= 1, the
 * Philox step counter does not wrap (MFG_EINVAL); d <= 64 (MFG_EUNSUPPORTED); the workspace (MFG_EWORKSPACE).  Mixed precision
 * reports into and is refused on the bound context's status word exactly as mfg_evaluate_pop. */
size_t mfg_consistency_given_workspace_bytes(int K, int64_t M, int T, int steps_given);
int mfg_consistency_given(const float* P, int K, int64_t M, int T, int d, double* metrics, double* steps, double* V,
                          void* workspace, size_t workspace_bytes, mfg_stream_t stream);
size_t mfg_consistency_pop_workspace_bytes(int64_t N, int H, int d, int K, int repeats, int steps_given, int actions_given,
                                           int traj_given);
int mfg_consistency_pop(const float* start32, int64_t N, int H, int d, int K, const double* theta, const double* shift,
                        const double* alpha_scale, const uint64_t* seed, uint32_t first_step, int repeats, int precision,
                        double* metrics, double* steps, double* V, float* actions, float* pi_traj, void* workspace,
                        size_t workspace_bytes, mfg_stream_t stream);

/* Weights of the reward network of networks.py:46-81 as device pointers (layouts as for mfg_reward_net_forward). */
typedef struct mfg_reward_net {
  int k1, f2, k2, n3, n4;
  const float *conv1_w, *conv1_b, *conv2_w, *conv2_b, *fc3_w, *fc3_b, *fc4_w, *fc4_b, *out_w, *out_b;
  float keep_prob; /* < 1: inverted dropout after fc3 and fc4 (the reference leaves it on, ac_irl.py:683) */
} mfg_reward_net_t;

/* a9 (IRL flavour), native inner loop of AC_IRL.train with the reference's per-step updates (ac_irl.py:664-712) on ONE
 * GPU.  For s < T, all launches issued back to back from native code (no interpreter between the dependent kernels):
 *   sample P ~ policy(pi), pi' = P^T pi, g, delta0 = discount V(pi') - V(pi)     (one fused launch, P materialised, :674-679)
 *   r = r_net(pi, P)                                                              (mfg_reward_net_forward, :683)
 *   delta = r + delta0; batch sums; w += lr_critic G_w/B, theta += lr_actor G_theta/B; *reward_acc += mean r   (:691-708)
 *   discount *= gamma; pi <- pi'                                                   (:710-711)
 * Where the matrix-core reward-network kernel serves (d = 21 / 15, the reference's layer geometry, n_fc3 <= 16) an env step is
 * TWO launches: [sampling + transition + score, theta formed by every wavefront from the previous step's partial sums; the
 * grid's last blocks reduce those sums and publish w, theta, G, the return] | [reward network + TD error from the updated w
 * + this step's partial sums]; one row reduction closes the episode.  Otherwise three (step | network | row reduction).
 * The dropout masks of step s use the Philox key  rn_seed ^ ((rn_call0 + s + 1) * 0x9E3779B97F4A7C15)  (mod 2^64) and the
 * sample counter rn_sample_offset + b -- the keys the host class would have passed to T separate
 * mfg_reward_net_forward calls numbered rn_call0 + 1 ... .  pi_io [B,d]: start states in, final states out; pi_scratch
 * [B,d]; P [B,d,d], reward / delta / g [B] hold the last step's values on return; G [F+3]; workspace as for
 * mfg_td_pg_accumulate(B) (the two-launch flow keeps theta between two env steps in the control block; the row reduction that
 * closes the episode leaves it zero again).  Philox steps first_step .. first_step+T-1 for the actions. */
int mfg_train_episode_irl(float* pi_io, float* pi_scratch, int64_t B, int d, int T, double* theta, double shift,
                          double alpha_scale, double* w, double gamma, uint64_t seed, uint32_t first_step,
                          uint64_t traj_offset, int precision, double lr_critic, double lr_actor,
                          const mfg_reward_net_t* net_host, uint64_t rn_seed, uint64_t rn_call0, uint64_t rn_sample_offset,
                          float* P, float* reward, double* delta, double* g, double* G, double* reward_acc, void* workspace,
                          size_t workspace_bytes, mfg_stream_t stream);

/* The same episode with the start states DRAWN from the table mat_pi0 [num_start,d] (the draw of mfg_draw_start at
 * step = first_step, trajectory ids traj_offset + b; ac_irl.py:655) -- inside the first step kernel where the two-launch flow
 * serves, by a launch of its own otherwise.  pi_out [B,d]: final states (output only); the rest as above: pi_scratch and
 * workspace as for mfg_train_episode_irl. */
int mfg_train_episode_irl_draw(const float* mat_pi0, int64_t num_start, float* pi_out, float* pi_scratch, int64_t B, int d, int T,
                               double* theta, double shift, double alpha_scale, double* w, double gamma, uint64_t seed,
                               uint32_t first_step, uint64_t traj_offset, int precision, double lr_critic, double lr_actor,
                               const mfg_reward_net_t* net_host, uint64_t rn_seed, uint64_t rn_call0, uint64_t rn_sample_offset,
                               float* P, float* reward, double* delta, double* g, double* G, double* reward_acc, void* workspace,
                               size_t workspace_bytes, mfg_stream_t stream);

/* a9 (IRL flavour), one update per episode (the batched form of ac_irl.py:664-712 with theta, w fixed over the episode) on
 * ONE GPU, issued natively: [fused T-step rollout: start states drawn in the kernel (idx == NULL) or gathered, actions
 * materialised, delta0 = discount V(pi') - V(pi), scores] | [reward network over all B*T transitions, states read in place
 * from pi_traj] | [batch sums with delta = delta0 + r folded in (+ row reduction)] (+ update with MFG_TRAIN_APPLY):
 * 3-4 launches, no framework call in between.  flags: MFG_ROLLOUT_DISCOUNT_POW | MFG_ROLLOUT_F64 | MFG_TRAIN_APPLY.
 * Dropout masks: Philox key rn_key, sample counter rn_sample_offset + b T + t (ONE mfg_reward_net_forward call over the
 * [B*T] transitions).  pi_traj [B,T+1,d], P [B,T,d,d], reward [B*T] (the network's output), delta / g [B*T] (delta final),
 * G [F+3]; workspace as for mfg_td_pg_accumulate(B*T).  *reward_acc += mean reward over the B*T transitions. */
int mfg_train_rollout_irl(const float* mat_pi0, int64_t num_start, const int32_t* idx, int64_t B, int d, int T, double* theta,
                          double shift, double alpha_scale, double* w, double gamma, uint64_t seed, uint32_t first_step,
                          uint64_t traj_offset, int flags, double lr_critic, double lr_actor, const mfg_reward_net_t* net_host,
                          uint64_t rn_key, uint64_t rn_sample_offset, float* pi_traj, float* pi_last, float* P, float* reward,
                          double* delta, double* g, double* G, double* reward_acc, void* workspace, size_t workspace_bytes,
                          mfg_stream_t stream);

/* Per-learner reward-network geometry, the optional TABLE of the four IRL population calls below: populations whose learners
 * differ in the SHAPE and the REGULARISER of their reward networks, the reference's sweep gridsearch.py:8-31 (reg x n_fc3 x
 * n_fc4, one AC_IRL per point) as ONE population.  Entry k is learner k's n_fc3, n_fc4, keep_prob (1: no dropout) and l1_l2
 * flag (read by the training steps only); d, k1 = 5, f2 = 2, k2 = 3 stay shared.  Limits per entry, those of the matrix-core
 * kernel: 1 <= n3 <= 16, 1 <= n4 <= 32, keep_prob in (0, 1]. */
typedef struct mfg_rn_geom { int32_t n3, n4; float keep_prob; int32_t l1l2; } mfg_rn_geom_t;   /* 16 bytes */

/* The table arguments geom_host / geom_dev of mfg_train_episodes_irl_pop, mfg_train_rollouts_irl_pop,
 * mfg_reward_net_forward_pop and mfg_reward_net_train_steps_pop.  Both NULL: no table, every learner has the geometry and
 * keep_prob (and l1l2) the call passes.  Both given: geom_host [K] is read by the checks, geom_dev [K] (device, the same
 * entries) by the kernels.  Then per_learner_net = 1 and net_stride / param_stride > 0 are required: learner k's parameters
 * are ONE flat row at conv1_w + k net_stride (params + k param_stride) in the order and at the offsets of
 * mfg_reward_net_param_offsets(d, 5, 2, 3, n3_k, n4_k); rows are as long as the longest learner's and nothing beyond a
 * learner's own NP_k floats is read or written.  Of the struct, k1 / f2 / k2 and conv1_w (the base of row 0) are read; n3,
 * n4, keep_prob and the other nine pointers are ignored (mfg_reward_net_train_steps_pop: its n3, n4, keep_prob and l1l2).
 * Learner k of a call with a table gives, bit for bit, what the single entry point (mfg_train_episode_irl_draw,
 * mfg_train_rollout_irl, mfg_reward_net_forward, mfg_reward_net_train_step) gives with learner k's geometry; a table whose
 * entries are all equal gives the bits of the call without a table.  Dynamic LDS and workspace slices are sized for
 * the largest n3 and the largest n4 of the table; the combine kernel's grid is ceil(max NP_k / 64) wide and blocks beyond a
 * learner's own NP_k do nothing.  No allocation; the training entry points do not synchronise.
 * Checked before anything is launched, on top of the checks of the call without a table: MFG_EINVAL for exactly one copy
 * NULL, per_learner_net = 0, a stride below the largest NP_k, an entry's keep_prob outside (0, 1]; MFG_EUNSUPPORTED
 * for an entry outside n3 <= 16 / n4 <= 32, d other than 15 / 21, an fc3_w of any learner not 8-byte aligned, a training batch
 * beyond the single step's limits at the largest n3; MFG_EWORKSPACE as without a table, at the largest geometry. */

/* IRL populations: K independent forward learners of AC_IRL.train (ac_irl.py:634-732; without a population control block
 * stop_criteria = -1 as in outerloop, with one -- mfg_ctx_set_pop_control -- learner k stops after the episode at which
 * |theta - theta_prev| < stop_criteria[k], as ac_irl.py:726 does, and holds what the single learner holds at that point)
 * trained in lock-step on ONE GPU, every launch of an episode serving all K.  Learner k of a population call gives, bit for bit
 * (theta, w, G, reward_acc, final states and the last step's P / reward / delta / g), what the single-learner path gives with
 * B = Bk, the same traj_offset and learner k's seed, theta, w, shift, alpha_scale, learning rates and reward network:
 *   step mode     `episodes` calls of mfg_train_episode_irl_draw (first_step + e T, lr x lr_schedule(first_episode + e),
 *                 reward_acc + e, rn_seed[k], rn_call0[k] + e T, rn_sample_offset = traj_offset);
 *   rollout mode  `episodes` calls of mfg_train_rollout_irl with idx = NULL and MFG_TRAIN_APPLY (first_step + e T, the same
 *                 rates, rn_key = rn_seed[k] ^ ((rn_call0[k] + e + 1) 0x9E3779B97F4A7C15), rn_sample_offset = traj_offset T).
 * Learning rates in episode e: lr_critic[k] x, lr_actor[k] x the schedule of mfg_train_rollouts at episode number
 * first_episode + e (AC_IRL.train numbers its episodes from 1: pass first_episode + 1 to reproduce it).
 * Dropout keys: rn_seed is a device array [K] (AC_IRL passes its seed + 0x5EED); rn_call0 a device array [K] (uint64,
 * required), learner k's count of reward calls made before (AC_IRLPopulation after reward_iteration, where each learner's
 * early stop has consumed its own number of reward calls; learners in lock-step pass K equal counts).  Step mode, episode e,
 * env step s:  rn_seed[k] ^ ((rn_call0[k] + e T + s + 1) x 0x9E3779B97F4A7C15);  rollout mode, episode e:
 * rn_seed[k] ^ ((rn_call0[k] + e + 1) x 0x9E3779B97F4A7C15)  (mod 2^64).
 * Reward networks: `net` (host struct).  per_learner_net = 0: every learner reads the same tensors; 1: every pointer is the
 * base of a stacked tensor, learner k's tensor t at base_t + k numel_t (numel_t from the geometry: k1^2, 1, f2 k2^2, f2,
 * n3 f2 d^2, n3, n4 (n3 + d), n4, n4, 1) when net_stride = 0, at base_t + k net_stride when net_stride > 0 (one padded flat
 * parameter row per learner, the layout of mfg_reward_net_train_steps_pop).  Geometry and keep_prob are shared, or per
 * learner with a table (geom_host / geom_dev, above; both NULL: none).
 * Per-learner scalars and learner-major arrays as for mfg_train_episodes_pop / mfg_train_rollouts_pop, plus P: step mode
 * pi_out / pi_scratch [K,Bk,d], P [K,Bk,d,d], reward / delta / g [K,Bk]; rollout mode pi_traj [K,Bk,T+1,d], pi_last [K,Bk,d]
 * (may be NULL), P [K,Bk,T,d,d], reward / delta / g [K,Bk,T].  reward_acc [K,episodes] (may be NULL; step mode: += every
 * step's mean reward, rollout mode: += the mean over the Bk T transitions).  Start states are drawn on the device from mat_pi0.
 * Checked before anything is launched: MFG_EINVAL for K outside [1, MFG_POP_MAX_K], a null pointer, keep_prob outside (0,1],
 * a Philox step counter that would wrap; MFG_EUNSUPPORTED where the matrix-core reward-network kernel does not serve
 * (d = 21 / 15, k1 = 5, f2 = 2, k2 = 3, n_fc3 <= 16, n_fc4 <= 32, every learner's fc3_w 8-byte aligned); MFG_EWORKSPACE when
 * one learner's slice (workspace_bytes, a multiple of 256) cannot hold the control block and the partial rows of the update:
 * 64 + min(ceil(Bk / 16), 256) (F + 4) 8 bytes in step mode, those of the gradient kernels over Bk T samples in rollout mode. */
/* step mode (AC_IRL.train, ac_irl.py:634-732; with a table: for the K points of gridsearch.py:8-31); workspace: K slices, each
 * with its control block zero on entry and on return, the rest scratch, as for mfg_train_episodes_pop; pi_scratch is scratch */
int mfg_train_episodes_irl_pop(const float* mat_pi0, int64_t num_start, float* pi_out, float* pi_scratch, int64_t B, int K, int d,
                               int T, int64_t episodes, int64_t first_episode, int constant, double* theta, const double* shift,
                               const double* alpha_scale, double* w, double gamma, const uint64_t* seed, uint32_t first_step,
                               uint64_t traj_offset, int precision, const double* lr_critic, const double* lr_actor,
                               const mfg_reward_net_t* net_host, int per_learner_net, int64_t net_stride,
                               const mfg_rn_geom_t* geom_host, const mfg_rn_geom_t* geom_dev, const uint64_t* rn_seed,
                               const uint64_t* rn_call0, float* P, float* reward, double* delta, double* g, double* G,
                               double* reward_acc, void* workspace, size_t workspace_bytes, mfg_stream_t stream);
/* rollout mode (one update per episode); flags: MFG_ROLLOUT_DISCOUNT_POW | MFG_ROLLOUT_F64; workspace: K slices, each with its
 * control block zero on entry and on return, the rest scratch, as for mfg_train_rollouts_pop */
int mfg_train_rollouts_irl_pop(const float* mat_pi0, int64_t num_start, int64_t B, int K, int d, int T, int64_t episodes,
                               int64_t first_episode, int constant, double* theta, const double* shift, const double* alpha_scale,
                               double* w, double gamma, const uint64_t* seed, uint32_t first_step, uint64_t traj_offset, int flags,
                               const double* lr_critic, const double* lr_actor, const mfg_reward_net_t* net_host,
                               int per_learner_net, int64_t net_stride, const mfg_rn_geom_t* geom_host,
                               const mfg_rn_geom_t* geom_dev, const uint64_t* rn_seed, const uint64_t* rn_call0, float* pi_traj,
                               float* pi_last, float* P, float* reward, double* delta, double* g, double* G, double* reward_acc,
                               void* workspace, size_t workspace_bytes, mfg_stream_t stream);

/* The reward network of n listed learners of a population in ONE launch of the matrix-core kernel (grid rows = the list; the
 * reward averages of reward_iteration and test_reward_network, ac_irl.py:848-897, :1008-1046): for slot s, learner
 * k = learners_host[s] (distinct, in [0, K)):
 *   reward[k N .. k N + N) = mfg_reward_net_forward(state + k s_state, action + k s_action, N, learner k's weights,
 *                                                   seed = keys_host[s], sample_offset)
 * bit for bit.  s_state / s_action: elements between two learners' inputs, 0 = one input shared by all (>= N d / N d^2
 * otherwise).  Weights: as for mfg_train_episodes_irl_pop (per_learner_net, net_stride), with the same optional table
 * (geom_host / geom_dev, above; both NULL: none).  reward [K,N]; rows of learners not listed are left alone.  The keys and the
 * list are uploaded into `scratch` (device, >= 16 n bytes) and the stream is drained once before the launch.  MFG_EINVAL:
 * null pointers, counts, a learner out of range or listed twice; MFG_EUNSUPPORTED outside the matrix-core geometry;
 * MFG_EWORKSPACE: scratch too small -- all before anything is launched. */
int mfg_reward_net_forward_pop(const float* state, const float* action, int64_t s_state, int64_t s_action, int64_t N, int d,
                               const mfg_reward_net_t* net_host, int per_learner_net, int64_t net_stride,
                               const mfg_rn_geom_t* geom_host, const mfg_rn_geom_t* geom_dev, int K,
                               const int32_t* learners_host, const uint64_t* keys_host, int n, uint64_t sample_offset,
                               float* reward, void* scratch, size_t scratch_bytes, mfg_stream_t stream);

/* Input gradients of the reward network ("reward sensitivities": what the learned reward rewards, locally, on given
 * transitions).  A block bound to the context (mfg_ctx_set_rn_input_grad; NULL unbinds; no device work, no stream) rides on
 * mfg_reward_net_forward_pop: with the context bound, that call enqueues, behind its reward launch and on its stream, the
 * gradient launch and the two launches of the means, for the learners of ITS list with their weights, geometry-table rows and
 * keys.  Every other call ignores the block; without one mfg_reward_net_forward_pop issues the launches it always did, and
 * with one its `reward` is bit for bit what it is without.
 *   Per sample n of learner k, for r = tanh(.) as mfg_reward_net_forward documents it (networks.py:46-81):
 *     grad_state [K,N,d] fp32    d r / d state, the state as it enters FC4 (the concatenation of networks.py:72)
 *     grad_action [K,N,d,d] fp32 d r / d action, the [d,d] image that enters the first convolution
 *   A ReLU passes the derivative where its pre-activation is > 0 and blocks it at 0.  With keep_prob < 1 the masks are the
 *   forward's own -- key keys_host[s], counter (unit, 3 | 4, sample_offset + n, 0) -- and a kept unit carries 1 / keep_prob
 *   in the backward pass as well.  fp32 like the forward; the sample's forward is recomputed by the gradient kernel (one
 *   256-thread block per (sample, list slot), every activation in LDS), so `reward` does not depend on it.
 *   Means over n, fp64:
 *     mean_state [K,2,d], mean_action [K,2,d,d]:  [k,0] = mean of the gradient, [k,1] = mean of gradient x input, each product
 *     formed in fp64 from the two fp32 values (exact).
 *   No floating-point atomics: chunk c of mfg_action_mean_pop's chunking of N is added in ascending n by one thread per
 *   element, a learner's chunk totals are added in chunk order by one thread per element and divided by N -- an order that
 *   depends on N alone, not on K, the list, or which outputs are requested; the means are the same bits with and without
 *   the per-sample arrays.
 *   Any of the four outputs may be NULL (not all); rows of learners not in the list are left alone in all four.  A per-sample
 *   array that is NULL lives in `workspace` (mfg_rn_input_grad_workspace_bytes(K, N, d) bytes, 8-byte aligned, contents
 *   scratch: the per-sample arrays [K,N,d + d d] fp32 and the chunk totals [K,chunks,2,d + d d] fp64).
 * Checked when the block is set: MFG_EINVAL for a null or destroyed context, all four outputs NULL, K outside
 * [1, MFG_POP_MAX_K], N < 1, a workspace that is not 8-byte aligned.  Checked again before the call launches anything (nothing
 * is written on refusal): MFG_EINVAL when K, N or d differ from the call's; MFG_EUNSUPPORTED for N >= 2^31; MFG_EWORKSPACE
 * when workspace is NULL or workspace_bytes is too small.  The geometry is the call's (d = 15 / 21, k1 = 5, f2 = 2, k2 = 3,
 * n_fc3 <= 16, n_fc4 <= 32, the optional table included). */
typedef struct mfg_rn_input_grad {
  float* grad_state;    /* [K, N, d]     d r / d state,  per sample; may be NULL */
  float* grad_action;   /* [K, N, d, d]  d r / d action, per sample; may be NULL */
  double* mean_state;   /* [K, 2, d]     may be NULL */
  double* mean_action;  /* [K, 2, d, d]  may be NULL */
  void* workspace;
  size_t workspace_bytes;
  int64_t N;
  int32_t K, d, reserved;
} mfg_rn_input_grad_t;
size_t mfg_rn_input_grad_workspace_bytes(int K, int64_t N, int d);
int mfg_ctx_set_rn_input_grad(mfg_ctx_t* ctx, const mfg_rn_input_grad_t* block);

/* One entry of the plan of mfg_reward_net_train_steps_pop: one update_reward of one learner. */
typedef struct mfg_rn_train_plan {
  int32_t learner;    /* in [0, K), once per update */
  float lr_t;         /* written by the call: (float)(lr sqrt(1 - beta2^t) / (1 - beta1^t)), t = adam_step, as the single step */
  uint64_t key;       /* Philox key of the dropout masks, as the seed of mfg_reward_net_train_step */
  double lr;          /* Adam learning rate */
  int64_t adam_step;  /* >= 1, the adam_step of mfg_reward_net_train_step */
  int32_t demo_rows[MFG_RN_TRAIN_MAX_TRAJ];  /* rows of the shared demonstration store (n_demo used) */
  int32_t gen_rows[MFG_RN_TRAIN_MAX_TRAJ];   /* rows of learner k's generated store (n_gen used) */
} mfg_rn_train_plan_t;

/* n_updates consecutive update_reward steps (ac_irl.py:804-846) of n_active learners of a population: update u, slot s runs,
 * for learner k = plan[u n_active + s].learner, exactly mfg_reward_net_train_step(params + k param_stride, adam_m + k param_stride,
 * adam_v + k param_stride, geometry, demo store, the entry's demo_rows, learner k's generated store (gen_state +
 * k gen_capacity steps d, gen_action + k gen_capacity steps d^2), the entry's gen_rows, steps, demo_divisor, keep_prob, l1l2,
 * the entry's key, lr and adam_step, flags 0, stats + 4 k) -- the same bits.  Two launches per update: the sample kernel on
 * grid (N + 1, n_active) and the combine kernel on grid (ceil(NP / 64), n_active), N = (n_demo + n_gen) steps.  Learners
 * without an entry in an update are not touched (no blocks).
 * params / adam_m / adam_v [K, param_stride] fp32 (param_stride >= mfg_reward_net_num_params); stats [K, 4] fp32.
 * Optional table (geom_host / geom_dev, above; both NULL: none): learner k's n3, n4, keep_prob and l1l2 come from entry k, and
 * the arguments n3, n4, keep_prob and l1l2 are not read.
 * plan_host [n_updates n_active] (its lr_t fields written first) is uploaded ONCE into plan_dev (device, >= n_updates n_active
 * sizeof(mfg_rn_train_plan_t) bytes) and the stream is drained once before the first launch.  workspace: n_active slices, each
 * mfg_reward_net_train_workspace_bytes(geometry, N) rounded up to 256 bytes; contents are scratch (plan_dev likewise).
 * Checked before anything is launched: MFG_EINVAL for null pointers, bad counts, param_stride < NP, a learner id out of
 * range or twice in one update, a store row negative or >= its capacity, adam_step < 1; MFG_EUNSUPPORTED outside
 * d = 15 / 21, k1 = 5, f2 = 2, k2 = 3, n_fc3 <= 16, n_fc4 <= 32, or for a batch beyond the single step's limits (n_demo, n_gen
 * <= MFG_RN_TRAIN_MAX_TRAJ, N <= 2048, N (1 + n_fc3) 4 B <= 60 KB); MFG_EWORKSPACE for a too small workspace or plan_dev. */
int mfg_reward_net_train_steps_pop(float* params, float* adam_m, float* adam_v, int64_t param_stride, int K, int d, int k1, int f2,
                                   int k2, int n3, int n4, const mfg_rn_geom_t* geom_host, const mfg_rn_geom_t* geom_dev,
                                   const float* demo_state, const float* demo_action, int64_t demo_capacity,
                                   const float* gen_state, const float* gen_action, int64_t gen_capacity,
                                   mfg_rn_train_plan_t* plan_host, void* plan_dev, size_t plan_dev_bytes, int n_updates,
                                   int n_active, int n_demo, int n_gen, int steps, int demo_divisor, float keep_prob, int l1l2,
                                   double beta1, double beta2, double eps, float* stats, void* workspace, size_t workspace_bytes,
                                   mfg_stream_t stream);

/* mfg_reward_net_train_steps_pop with importance weights (ac_irl.py:404-406, see mfg_reward_net_train_step_z): gen_log_z is a
 * device fp64 array [K, gen_capacity], learner k's ln z at gen_log_z + k gen_capacity, indexed by the plan entries' gen_rows
 * (already checked against gen_capacity).  Update u, slot s is exactly mfg_reward_net_train_step_z for that learner -- the same
 * bits, with or without a geometry table.  gen_log_z = NULL: mfg_reward_net_train_steps_pop; workspace as for
 * mfg_reward_net_train_steps_pop. */
int mfg_reward_net_train_steps_pop_z(float* params, float* adam_m, float* adam_v, int64_t param_stride, int K, int d, int k1, int f2,
                                     int k2, int n3, int n4, const mfg_rn_geom_t* geom_host, const mfg_rn_geom_t* geom_dev,
                                     const float* demo_state, const float* demo_action, int64_t demo_capacity,
                                     const float* gen_state, const float* gen_action, int64_t gen_capacity,
                                     mfg_rn_train_plan_t* plan_host, void* plan_dev, size_t plan_dev_bytes, int n_updates,
                                     int n_active, int n_demo, int n_gen, int steps, int demo_divisor, float keep_prob, int l1l2,
                                     double beta1, double beta2, double eps, float* stats, void* workspace, size_t workspace_bytes,
                                     const double* gen_log_z, mfg_stream_t stream);

/* f1 (optional importance weights, ac_irl.py:270-289 calc_pdf_action, :324-379 calc_z): log-density of the
 * product-Dirichlet policy for N (state, action) pairs under K policies theta_k (device array):
 *   out[n*K + k] = sum_i log Dirichlet(P_n[i,:] ; a_i),  a_ij = max(alpha_floor, alpha_scale * softplus(theta_k x_ij)).
 * The reference evaluates the density itself and divides by a normaliser c before multiplying 15*d factors
 * (:365-373); the log-space value is exact where that under/overflows.  alpha_floor = 1+1e-6 and alpha_scale = 1
 * reproduce calc_z; alpha_floor = 0 reproduces calc_pdf_action.  Entries of P below p_floor are raised to it
 * (p_floor = 0: ln 0 = -inf, density 0, like tf.distributions.Dirichlet.prob).  fp64 out. */
int mfg_policy_logpdf(const float* pi, const float* P, int64_t N, int d, const double* thetas, int K, double shift,
                      double alpha_scale, double alpha_floor, double p_floor, double* out, mfg_stream_t stream);

/* f1, the importance log-weights of a trajectory store in ONE launch (ac_irl.py:292-321 calc_z's z_j = [1/k sum_k q_k(tau_j)]^-1
 * over the last num_policies policies, :324-379 its graph, which multiplies 15 d densities in linear space over c = 2e11 and
 * overflows): for learner k and every physical store row listed in rows_host,
 *   log_z[k capacity + row] = ln n_pol - logsumexp_p( sum_t ln q_{thetas[k n_pol + p]}(a_t; s_t) - log_start ),
 * ln q the formula of mfg_policy_logpdf (alpha_floor / p_floor clamps, shift[k], fp64 throughout), log_start = ln of the number
 * of start states (Pr(s_1)).  Stores: state [capacity, steps, d], action [capacity, steps, d, d] fp32, shared by all learners
 * (per_learner_store = 0), or [K, capacity, ...] with learner k's store at k capacity rows (per_learner_store = 1).  thetas
 * [K, n_pol] and shift [K] are device fp64; K = 1 is the single-learner form; any n_pol >= 1.  Rows not listed are left
 * alone.  Grid (n_rows, K), one wavefront per policy; the per-policy sums are folded into the logsumexp in policy order by
 * one thread, so learner k's values are the same bits whatever K and the row list are.  A row whose every density is 0 (an
 * exact zero in P with p_floor = 0) gets +inf, as tf.distributions.Dirichlet.prob would give.
 * rows_host is uploaded into `scratch` (device, >= 4 n_rows bytes) and the stream is drained once before the launch; nothing
 * is read back.  Checked before anything is launched: MFG_EINVAL for null pointers, bad counts (capacity, steps, d, n_pol < 1,
 * K outside [1, MFG_POP_MAX_K], d > MFG_MAX_D), a row outside [0, capacity) or listed twice; MFG_EWORKSPACE for a scratch
 * too small for the row list. */
int mfg_traj_log_z_pop(const float* state, const float* action, int64_t capacity, const int32_t* rows_host, int n_rows,
                       int steps, int d, const double* thetas, int n_pol, const double* shift, int K, int per_learner_store,
                       double alpha_scale, double alpha_floor, double p_floor, double log_start, double* log_z, void* scratch,
                       size_t scratch_bytes, mfg_stream_t stream);

/* a11: out[b] = JSD(p_b, q_b), zeros -> 1e-100, inputs renormalised like scipy.stats.entropy
 * (mfg_ac2.py:546-563).  fp64 out. */
int mfg_jsd(const float* p, const float* q, int64_t B, int d, double* out, mfg_stream_t stream);

/* The VAR baseline as a population (the reference's var.py: train, forecast, validation, evaluate_train, evaluate_test and the
 * 100 fits of cross_validation, :102-162, :195-416): K independent vector autoregressions, each with its own lag, ridge and
 * days, fitted, forecast and scored in the three launches of one call.  fp64 throughout.
 *   days [D, Hd, d] fp64: a table of day matrices.  Model k (models[k]) has a lag p >= 1, a ridge lambda > 0, an ordered list of
 *   n_train training days train_idx[k train_stride + 0 ..] and of n_test >= 0 test days test_idx[k test_stride + 0 ..] (indices
 *   into the table), and an origin, 0 or 1.
 *   Series and regressors: Y is the training days concatenated in list order (lags run across day boundaries, var.py:129-141);
 *   T = n_train Hd, n = T - p, m = 1 + p d; for t = p .. T-1, z_t = [1, y_{t-1}, ..., y_{t-p}]: regressor 0 is the constant,
 *   regressor 1 + (l-1) d + j is topic j at lag l.
 *   coef [K, M, d]: B = (Z'Z + lambda I)^-1 Z'Y in rows < m, zeros in rows >= m.  This is RIDGE regression, not the reference's
 *   minimum-norm least squares (statsmodels): rows that sum to 1 make Z'Z singular for every shape, and lambda > 0 is what
 *   factors by Cholesky; B tends to the minimum-norm solution as lambda -> 0.  No information criterion selects the order
 *   (the residual covariance is exactly singular): the model of lag p has order p.
 *   sse [K, d]: sum over t of the squared residual per topic.  insample [K, 2]: the mean over t of ||y_t - B'z_t||_1 and of
 *   JSD(y_t, B'z_t) (evaluate_train part 2, var.py:229-241).  JSD as var.py:175-192: entries <= 0 become 1e-100, then
 *   1/2 (KL(P||M) + KL(Q||M)), M = (P + Q)/2, every argument renormalised as scipy.stats.entropy does.
 *   future [K, S_max, d] or NULL: the forecast of S = n_test Hd rows, zeros in rows >= S.  Origin 0 (var.py:258-327): one path
 *   fed by the last p training rows and then by its own outputs.  Origin 1 (rolling): for test day j the history is the
 *   training series, then test days 0 .. j-1, then hour 0 of day j; hours 1 .. Hd-1 are forecast from it and hour 0 of the
 *   output is the observed row, bit for bit.  Row s is compared with row s of the concatenated test days:
 *   per_day [K, test_stride, 4] or NULL: (l1_final, l1_mean, JSD_final, JSD_mean) per test day -- hour Hd-1 and the mean over the
 *   Hd hours (evaluate_test, var.py:342-383); zeros in rows >= n_test.  metrics [K, 8]: mean and standard deviation (ddof 0) over
 *   the test days of each of the four, in that order; NaN without a test day.
 *   status [K] int32: bit 0 (MFG_VAR_NONFINITE) a non-finite value in the rows the model reads, or a day index outside [0, D);
 *   bit 1 (MFG_VAR_PIVOT) a non-positive or non-finite Cholesky pivot (reported only without bit 0).  A model whose status is
 *   not 0 returns NaN in all its float outputs; no other model is affected.
 *   Order: G = Z'Z + lambda I and Z'Y are formed element by element, t ascending, fused multiply-add; a right-looking Cholesky
 *   in 16-wide panels (the d right-hand sides ride along as d more rows; the trailing update subtracts a panel's 16 products in
 *   column order), the back substitution panel by panel from the last; a dot product B'z is 16 strided partial sums (terms
 *   i, i + 16, ... ascending) added in partial order; every mean is added in row, hour or day order by one thread.  So each
 *   summation order is a function of the model's own shapes, there are no floating-point atomics, and a model's outputs are
 *   the same bits whether it runs alone or among others, in any position.
 *   models_host / models: the same K records on the host (read by the checks and for the launch geometry) and on the device
 *   (read by the kernels).  ws_offset is the model's byte offset into the workspace: mfg_var_fit_workspace_bytes fills it in
 *   the host records (each model gets 64 bytes + (m + d) m doubles, rounded up to 256 bytes) and returns the total, 0 for K < 1,
 *   a null table or a record outside the limits.  The workspace is 8-byte aligned; its contents are scratch.
 *   Everything is enqueued on fit->stream; the call neither allocates nor synchronises.
 * Checked before anything is launched (MFG_EINVAL): a null struct or pointer (future and per_day may be null, the index tables
 * when their stride is 0), 1 <= K <= MFG_POP_MAX_K, D >= 1, 1 <= Hd <= 64, 1 <= d <= 64; per model 1 <= n_train <= 64 and
 * <= train_stride, 0 <= n_test <= 64 and <= test_stride, lag >= 1, m <= MFG_VAR_MAX_REGRESSORS and <= M, n >= 1, origin 0
 * or 1 and with origin 1 lag <= T + 1, lambda finite and > 0, n_test Hd <= S_max when future is given, ws_offset as
 * mfg_var_fit_workspace_bytes lays it out; MFG_EWORKSPACE when workspace_bytes is below that call's total. */
#define MFG_VAR_MAX_REGRESSORS 512
#define MFG_VAR_NONFINITE 1
#define MFG_VAR_PIVOT 2
typedef struct mfg_var_model {
  int32_t lag, origin;
  int32_t n_train, n_test;
  double ridge;
  int64_t ws_offset;
} mfg_var_model_t; /* 32 bytes */
typedef struct mfg_var_fit {
  const double* days;
  const mfg_var_model_t* models_host;
  const mfg_var_model_t* models;
  const int32_t* train_idx;
  const int32_t* test_idx;
  double* coef;
  double* sse;
  double* insample;
  double* future;
  double* per_day;
  double* metrics;
  int32_t* status;
  void* workspace;
  size_t workspace_bytes;
  mfg_stream_t stream;
  int32_t D, Hd;
  int32_t d, K;
  int32_t train_stride, test_stride;
  int32_t M, S_max;
} mfg_var_fit_t;
size_t mfg_var_fit_workspace_bytes(int K, mfg_var_model_t* models_host, int d);
int mfg_var_fit_pop(const mfg_var_fit_t* fit);

/* The RNN baseline as a population: the third arm of the paper's comparison.  The reference only prepares the network's
 * training file (process.py:4-22), reads its predictions back for a figure (read_rnn, mfg_ac2.py:757-761) and hard-codes its
 * scores (plots.py:29-30); the network itself is not in the reference, so the model below is this project's definition.
 * K independent models, each with its own hidden size, learning rate, weight decay, clip, epochs and day lists, trained,
 * selected on held-out days, forecast and scored in the two launches of one call.  fp64 throughout.
 *   days [D, Hd, d] fp64: a table of day matrices, as for mfg_var_fit_pop.  Model k (models[k]) lists n_train training days
 *   train_idx[k train_stride + 0 ..], n_val >= 0 validation days (val_idx, val_stride) and n_test >= 0 test days (test_idx,
 *   test_stride).  A day is one sequence: nothing crosses a day boundary.
 *   The model: one LSTM layer of hidden size H and a softmax head.  Weights are packed as
 *     Wx [4H, d] | Wh [4H, H] | b [4H] | Wo [d, H] | bo [d],    W(H, d) = 4H (d + H + 1) + d (H + 1) values,
 *   gate order i, f, g, o (torch.nn.LSTMCell's; one gate bias).  a = Wx x + Wh h + b; c' = s(a_f) c + s(a_i) tanh(a_g);
 *   h' = s(a_o) tanh(c'); yhat = softmax(Wo h' + bo); s the logistic function; h = c = 0 at hour 0 of every day.
 *   Loss (teacher forced): L = 1/(n_train (Hd-1)) sum_n sum_{t=0..Hd-2} -sum_j y[n,t+1,j] log yhat[n,t,j] + wd/2 ||w||^2,
 *   the network fed the observed rows y[n,t].  The whole training set is one batch: an epoch is one gradient of L (the
 *   weight-decay term included) and one update.  If clip > 0 and ||g||_2 > clip, g is scaled by clip / ||g||_2.  optimizer
 *   MFG_RNN_ADAM: m = b1 m + (1-b1) g, v = b2 v + (1-b2) g^2, w -= lr / (1 - b1^e) m / (sqrt(v) / sqrt(1 - b2^e) + 1e-8),
 *   b1 = 0.9, b2 = 0.999, e the epoch from 1 (torch.optim.Adam's form; b^e by repeated multiplication); MFG_RNN_SGD: w -= lr g.
 *   w0 [K, W_max]: the initial weights (first W(H, d) values of a row).  There is no device random number in this call.
 *   loss [K, E_max]: L at the weights BEFORE the update of each epoch; NaN beyond the model's epochs.
 *   Forecast (the definition of origin 1 of mfg_var_fit_pop): a day starts from its observed hour 0 with zero state and the
 *   model's own output is fed back for Hd - 1 hours.  Per day (l1_final, l1_mean, JSD_final, JSD_mean) against the observed
 *   day, hour Hd-1 and the mean over the Hd hours (hour 0 contributes 0), L1 and JSD as for mfg_var_fit_pop.
 *   Selection: after every eval_every-th epoch and after the last one the validation days are forecast and the mean over
 *   them of JSD_mean goes to val [K, C_max] (NaN beyond the model's own checks); the weights with the lowest value are kept,
 *   ties go to the earlier check, its epoch to best_epoch [K].  weights [K, W_max] (zeros beyond W(H, d)) are that iterate's;
 *   without validation days they are the last iterate's, best_epoch = epochs and val is all NaN.
 *   future [K, test_stride, Hd, d]: the forecast of the test days from `weights`, hour 0 the observed row, zeros in days
 *   >= n_test.  per_day [K, test_stride, 4], zeros in rows >= n_test.  metrics [K, 8]: mean and standard deviation (ddof 0)
 *   over the test days of each of the four, the columns of mfg_var_fit_pop; NaN without a test day.
 *   status [K] int32: bit 0 (MFG_RNN_NONFINITE) a non-finite value in a row the model reads (training, validation or test
 *   day) or in its w0, or a day index outside [0, D) -- the index is clamped before it addresses anything; bit 1
 *   (MFG_RNN_DIVERGED) a non-finite loss or gradient norm in some epoch, reported when bit 0 is clear.  Such a model returns
 *   NaN in every float output and best_epoch 0; no other model is affected.
 *   Order: every dot product is added in ascending index order with fused multiply-add (a gate: the bias, the d inputs, the H
 *   hidden values; the backward product with Wh': four partial sums, one per gate block, added in gate order); a gradient
 *   entry is added over hours ascending, days ascending within an hour; sums over the weights (||w||^2, ||g||^2) and over the
 *   (hour, day) losses are 1024 strided partial sums, folded by an xor butterfly within each group of 64 and then added in
 *   group order.  So each summation order is a function of the model's own (d, H, n_train, n_val, n_test, Hd), there are no
 *   floating-point atomics, and a model's outputs are the same bits alone, among others, in any position.
 *   models_host / models: the same K records on the host (for the checks) and on the device (for the kernels).  ws_offset is
 *   the model's byte offset into the workspace; mfg_rnn_fit_workspace_bytes fills it in the host records and returns the
 *   total, 0 for K < 1, a null table or a record outside the limits.  The workspace is 8-byte aligned, its contents scratch.
 *   Everything is enqueued on fit->stream; the call neither allocates nor synchronises nor reads back.
 * Checked before anything is launched (MFG_EINVAL): a null struct or pointer (an index table may be null when its stride is
 * 0; future and per_day when test_stride is 0; val when C_max is 0), 1 <= K <= MFG_POP_MAX_K, D >= 1, 2 <= Hd <= 64,
 * 2 <= d <= 64, optimizer MFG_RNN_ADAM or MFG_RNN_SGD, eval_every >= 1; per model H a multiple of 4 in [4, 64],
 * 1 <= n_train <= 64 and <= train_stride, 0 <= n_val <= 64 and <= val_stride, 0 <= n_test <= 64 and <= test_stride,
 * 1 <= epochs <= 65535 and <= E_max, its checks <= C_max, W(H, d) <= W_max, lr finite and > 0, wd and clip finite and >= 0,
 * ws_offset as mfg_rnn_fit_workspace_bytes lays it out; MFG_EWORKSPACE when workspace_bytes is below that call's total. */
#define MFG_RNN_ADAM 0
#define MFG_RNN_SGD 1
#define MFG_RNN_NONFINITE 1
#define MFG_RNN_DIVERGED 2
#define MFG_RNN_MAX_EPOCHS 65535
typedef struct mfg_rnn_model {
  int32_t hidden, epochs;
  int32_t n_train, n_val;
  int32_t n_test, reserved;
  double lr;
  double wd;
  double clip;
  int64_t ws_offset;
} mfg_rnn_model_t; /* 56 bytes */
typedef struct mfg_rnn_fit {
  const double* days;
  const mfg_rnn_model_t* models_host;
  const mfg_rnn_model_t* models;
  const int32_t* train_idx;
  const int32_t* val_idx;
  const int32_t* test_idx;
  const double* w0;
  double* weights;
  double* loss;
  double* val;
  int32_t* best_epoch;
  double* future;
  double* per_day;
  double* metrics;
  int32_t* status;
  void* workspace;
  size_t workspace_bytes;
  mfg_stream_t stream;
  int32_t D, Hd;
  int32_t d, K;
  int32_t train_stride, val_stride;
  int32_t test_stride, W_max;
  int32_t E_max, C_max;
  int32_t optimizer, eval_every;
} mfg_rnn_fit_t;
size_t mfg_rnn_fit_workspace_bytes(int K, mfg_rnn_model_t* models_host, int d, int Hd);
int mfg_rnn_fit_pop(const mfg_rnn_fit_t* fit);

/* Demonstrations from agent logs: the states pi [d] and actions P [d,d] that AC_IRL, the forward learners and the baselines
 * start from, counted on the device from a log that says which of C categories each of U agents was in at each hour.  The
 * reference reads them from files of a recorder that is not part of it and patches them up in three routines (reorder,
 * mfg_ac2.py:58-81; normalize, :116-137; convert_action, ac_irl.py:116-157); the definitions below are this project's own and
 * restate those routines where they are cited.  Integer work: every output is the same bits on every run and layout.
 *   topic [N, H, U] int32 (day, hour, agent; agent fastest).  A value in [0, C) is a raw category, a negative value an agent
 *   that is absent that hour, a value >= C counts as absent and sets bit 0 of the day's status.
 *   1. raw[n,h,c]: the agents of day n in category c at hour h.
 *   2. rank[n,c].  MFG_DEMOS_ORDER_FIRST_HOUR (reorder): per day by decreasing raw[n,0,c], ties by ascending c.
 *      MFG_DEMOS_ORDER_TOTAL: one ranking for all days by decreasing sum_{n,h} raw, the same tie rule.  MFG_DEMOS_ORDER_GIVEN:
 *      order_given [order_given_rows, C] int32 (rows = N, or 1 for all days) holds the ranks; -1 drops a category, a value outside
 *      [-1, C) drops it and sets status bit 0 (of every day that row serves); duplicate ranks are not checked.  An agent in a
 *      category that is dropped or of rank >= width is absent for that hour.
 *   3. counts[n,h,i], i < width: the agents at rank i.  present[n,h] = sum_i counts.
 *   4. moves[n,h,i,j], h < H-1: the agents at rank i at hour h and rank j at hour h+1, both < width.  row_total[n,h,i] = sum_j.
 *   5. state[n,h,i] = (float)((double)counts / (double)present), i < d (with width > d the row sums to less than 1, as normalize
 *      followed by the [0:d] slice of init_pi0).  present = 0: the row is NaN and status bit 1 is set.
 *   6. action[n,h,i,j] = (float)((double)moves / (double)row_total), i, j < d.  row_total = 0 and counts = 0: every entry
 *      (float)(1 / (double)d) with MFG_DEMOS_EMPTY_UNIFORM (convert_action), 1 on the diagonal with MFG_DEMOS_EMPTY_IDENTITY
 *      (what the recorder wrote); row_total = 0 and counts > 0 (every agent of the row left the recorded set): identity under
 *      either setting (convert_action tests state == 0 and leaves such a row alone).
 *   7. left[n,h,i] = counts[n,h,i] - row_total[n,h,i] and entered[n,h,j] = counts[n,h+1,j] - sum_i moves[n,h,i,j], both over
 *      width and >= 0; a closed population has 0 in both.
 *   Shapes: state [N,H,d], action [N,H-1,d,d] fp32; counts [N,H,width], moves [N,H-1,width,width], present [N,H], left and
 *   entered [N,H-1,width], order [N,C] (rank -> raw category, -1 where no category has the rank), status [N] int32.  order and
 *   status are required, every other output may be NULL and changes no other output.
 *   Second mode, topic = NULL: counts and moves are INPUTS (the int32 arrays of mfg_agents_step_pop, width = d) and only steps
 *   5 to 7 run; order is not written, order_mode / C / U are ignored.  An hour with a negative count or move (the failed-member
 *   mark of mfg_agents_step_pop) sets status bit 2: its state and action are NaN, its present, left and entered -1, and so is
 *   entered of the hour before an hour with a negative count.
 *   status: bit 0 MFG_DEMOS_BAD_VALUE, bit 1 MFG_DEMOS_EMPTY_HOUR, bit 2 MFG_DEMOS_FAILED; one word per day, a day's bits and
 *   outputs do not depend on any other day (but through MFG_DEMOS_ORDER_TOTAL's ranking).
 *   Launches, all on demos->stream: the workspace and status are zeroed (memset nodes), the category histogram the ranking
 *   needs (none for a given order), the ranking (a workgroup per day), the counting pass (a workgroup walks the hours of its
 *   chunks of MFG_DEMOS_CHUNK agents of one day; tiles in LDS, one global integer atomic per non-zero cell and hour of a
 *   workgroup), the finishing pass (a workgroup per day and hour).  Nothing is allocated or synchronised; the call can be captured.
 *   workspace: mfg_demos_workspace_bytes(N, H, C, width) bytes (0 for arguments outside the limits; the second mode needs none
 *   and takes NULL), 8-byte aligned; contents are scratch and are zeroed inside the call.
 *   groups: the workgroups of the counting pass per day, each taking every groups-th chunk; 0 (the default) spreads two
 *   workgroups per compute unit over the days.  No output depends on it.
 *   lds_update: MFG_DEMOS_LDS_PLAIN (0, the default: one LDS atomic per lane) or MFG_DEMOS_LDS_COMBINE (lanes of a wave that hit
 *   the same cell are combined before the LDS atomic, two rounds, then one atomic per lane that is left).  The same bits; the
 *   plain form measured faster on both logs of tools/demos_probe.py (profiles/demos_from_logs.txt), the other is kept for
 *   logs that are more contended than those.
 * Checked before anything is launched (MFG_EINVAL): a null descriptor, order or status; N < 1, H < 2; with a log U < 1 or
 * U > 2^31 - 1, C < 1 or C > MFG_DEMOS_MAX_C, width > C, an unknown order_mode, MFG_DEMOS_ORDER_GIVEN without a table or with
 * order_given_rows not 1 or N, a null or misaligned workspace; without a log null counts or moves; d < 1 or d > width; an
 * unknown empty_row or lds_update, groups < 0; workspace_bytes below the query's value (the message names the bytes needed); N H times
 * the chunks of a day above 2^31 - 1.  MFG_EUNSUPPORTED: width > 64. */
#define MFG_DEMOS_MAX_C 4096
#define MFG_DEMOS_CHUNK 8192
#define MFG_DEMOS_ORDER_FIRST_HOUR 0
#define MFG_DEMOS_ORDER_TOTAL 1
#define MFG_DEMOS_ORDER_GIVEN 2
#define MFG_DEMOS_EMPTY_UNIFORM 0
#define MFG_DEMOS_EMPTY_IDENTITY 1
#define MFG_DEMOS_LDS_PLAIN 0
#define MFG_DEMOS_LDS_COMBINE 1
#define MFG_DEMOS_BAD_VALUE 1
#define MFG_DEMOS_EMPTY_HOUR 2
#define MFG_DEMOS_FAILED 4
typedef struct mfg_demos {
  const int32_t* topic;
  const int32_t* order_given;
  float* state;
  float* action;
  int32_t* counts;
  int32_t* moves;
  int32_t* order;
  int32_t* present;
  int32_t* left;
  int32_t* entered;
  int32_t* status;
  void* workspace;
  size_t workspace_bytes;
  mfg_stream_t stream;
  int64_t U;
  int32_t N, H;
  int32_t C, d;
  int32_t width, order_mode;
  int32_t empty_row, order_given_rows;
  int32_t lds_update, groups;
} mfg_demos_t;
size_t mfg_demos_workspace_bytes(int N, int H, int C, int width);
int mfg_demos_from_logs(const mfg_demos_t* demos);

/* Bootstrap replicates of the demonstrations: the agents of a log resampled on the device.  A state of mfg_demos_from_logs is a
 * proportion over the U recorded agents and an action row a proportion over the agents of one topic at one hour; this call
 * says how far those move when the recorded agents are drawn again.  It is the Poisson bootstrap over the sampling unit, the
 * agent with its whole trajectory: in replicate r every agent counts w times, w ~ Poisson(1) independent per agent and
 * replicate and the same at every hour.  Nothing is gathered: the log is streamed, with R weighted tallies instead of one.
 * (The exact multinomial bootstrap fixes sum w = U; here the weighted `present` varies by about 1 / sqrt(U) between replicates.)
 *   topic [N, H, U] int32 as mfg_demos_from_logs.  rank [rank_rows, C] int32, rank_rows 1 or N: the ranks, with the meaning of
 *   MFG_DEMOS_ORDER_GIVEN (-1 drops a category, a value outside [-1, C) drops it and sets status bit 0).  The ranking is always
 *   given and shared by the replicates -- the ranking of the recorded sample (mfg_demos_from_logs' `order`, inverted) --, so
 *   that topic i is the same category in every replicate and a cell's R values can be compared; a ranking per replicate would
 *   mix the noise of the labels into every cell and is not offered.
 *   Weights, word by word.  Replicate r, day n, agent u:
 *     (x0, x1, x2, x3) = Philox4x32-10(counter = (u, day_key low 32 bits, r >> 2, MFG_DEMOS_BOOT_TAG | (day_key >> 32) << 16),
 *                                      key = (seed low 32 bits, seed high 32 bits))
 *     day_key = day_offset + n with MFG_DEMOS_UNIT_AGENT_DAY (an agent index is another person each day; day_offset lets the
 *     days be sent in chunks without changing a bit), day_key = 0 with MFG_DEMOS_UNIT_AGENT (agent u is one person who carries
 *     one weight through all days; day_offset is ignored).  day_key must lie in [0, 2^48).
 *     w = #{k < 12 : x[r & 3] >= T[k]},  T[k] = floor(2^32 sum_{j <= k} e^-1 / j!) = MFG_DEMOS_BOOT_TABLE, so 0 <= w <= 12: the
 *     tail beyond 12, of mass < 2^-32, is folded into 12.  MFG_DEMOS_BOOT_TAG in the low 16 bits of the fourth counter word
 *     separates these draws from every other use of the generator (the samplers put bits 32..47 of a trajectory id there).
 *   Outputs, replicate r: steps 3 to 7 of mfg_demos_from_logs with every agent of day n counted w times -- counts
 *   [R,N,H,width], moves [R,N,H-1,width,width], present [R,N,H], left and entered [R,N,H-1,width] int32, state [R,N,H,d], action
 *   [R,N,H-1,d,d] fp32, status [R,N].  Steps 5 to 7 are the second mode of mfg_demos_from_logs over the R N "days" r N + n, by
 *   the same kernel.  status bits as there: bit 0 for a value >= C in the day's log or a bad rank, in every replicate of the day
 *   whatever the weights; bit 1 for a replicate whose weighted present is 0 at some hour (NaN rows, as an empty hour).
 *   status is required; every other output may be NULL and changes no other output.  Integer work: no output depends on
 *   groups, on how replicates are blocked or on the chunking of agents or days.
 *   Launches, all on boot->stream: memsets (the flags, counts and moves -- the caller's arrays when given, else the
 *   workspace's --, status), the counting pass (a workgroup walks its chunks of MFG_DEMOS_CHUNK agents of one day for four
 *   replicates -- one Philox block -- or one where four sets of tiles do not fit in LDS; one LDS atomic of w per agent, hour
 *   and replicate with w > 0; one global integer atomic per non-zero cell), the finishing pass, and one pass that adds bit 0.
 *   Nothing is allocated or synchronised; the call can be captured.
 *   workspace: mfg_demos_bootstrap_workspace_bytes(R, N, H, C, width) bytes (0 for arguments outside the limits), 8-byte
 *   aligned; contents are scratch and are zeroed inside the call.
 *   groups: the workgroups of the counting pass per day and replicate block; 0 spreads two per compute unit.
 * Checked before anything is launched (MFG_EINVAL): a null descriptor, topic, status or rank table; rank_rows not 1 or N;
 * N < 1, H < 2; R outside [1, MFG_DEMOS_BOOT_MAX_R]; R N H > 2^31 - 1; U < 1 or 12 U > 2^31 - 1 (a weighted cell must fit
 * int32); C < 1 or C > MFG_DEMOS_MAX_C; width > C; d < 1 or d > width; an unknown unit or empty_row; groups < 0; day_key outside
 * [0, 2^48); a null or misaligned workspace or workspace_bytes below the query's value.  MFG_EUNSUPPORTED: width > 64. */
#define MFG_DEMOS_BOOT_MAX_R 1024
#define MFG_DEMOS_BOOT_TAG 0xB007u
#define MFG_DEMOS_UNIT_AGENT_DAY 0
#define MFG_DEMOS_UNIT_AGENT 1
#define MFG_DEMOS_BOOT_TABLE                                                                                      \
  { 1580030168u, 3160060337u, 3950075421u, 4213413783u, 4279248373u, 4292415291u, 4294609777u, 4294923276u, 4294962463u, \
    4294966817u, 4294967252u, 4294967292u }
typedef struct mfg_demos_boot {
  const int32_t* topic;
  const int32_t* rank;
  float* state;
  float* action;
  int32_t* counts;
  int32_t* moves;
  int32_t* present;
  int32_t* left;
  int32_t* entered;
  int32_t* status;
  void* workspace;
  size_t workspace_bytes;
  mfg_stream_t stream;
  int64_t U;
  uint64_t seed;
  int64_t day_offset;
  int32_t N, H;
  int32_t C, d;
  int32_t width, R;
  int32_t rank_rows, unit;
  int32_t empty_row, groups;
} mfg_demos_boot_t;
size_t mfg_demos_bootstrap_workspace_bytes(int R, int N, int H, int C, int width);
int mfg_demos_bootstrap(const mfg_demos_boot_t* boot);

/* Bands over replicates: x [R, cells] fp32 (member r of cell c at x[r cells + c]; e.g. the state or action of
 * mfg_demos_bootstrap flattened), per cell over its R values
 *   mean [cells], std [cells] fp64: s = x[0] + x[1] + ... in the order r = 0 .. R - 1 in fp64, mean = s / R; then
 *   q = sum_r (x[r] - mean)^2 in the same order, every operation rounded on its own, std = sqrt(q / R) (ddof 0);
 *   quant [Q, cells] fp32: the order statistic of 0-based rank ranks[q] among the R values -- an element, not an interpolation
 *   (the convention of mfg_forecast_pop); ranks may repeat and need not be sorted.
 * A cell with a NaN in any replicate is NaN in all three.  mean, std and quant may each be NULL (quant only with Q = 0).  One
 * launch on bands->stream (a workgroup per 16 cells, their R values in LDS); nothing is allocated or synchronised.
 * MFG_EINVAL: a null descriptor or x, R outside [1, MFG_DEMOS_BOOT_MAX_R], cells < 0, Q outside [0, MFG_FORECAST_MAX_RANKS],
 * Q > 0 without quant, a rank outside [0, R). */
typedef struct mfg_replicate_bands {
  const float* x;
  double* mean;
  double* std;
  float* quant;
  mfg_stream_t stream;
  int64_t cells;
  int32_t R, Q;
  int32_t ranks[MFG_FORECAST_MAX_RANKS];
} mfg_replicate_bands_t;
int mfg_replicate_bands(const mfg_replicate_bands_t* bands);

/* The Dirichlet-multinomial (Polya) likelihood of the counted moves under each of a population of policies: how probable the
 * integer moves of mfg_demos_from_logs / mfg_demos_bootstrap / mfg_agents_step_pop are under (theta, shift, alpha_scale), in
 * closed form -- no sampling, no floor; a zero count is an ordinary outcome, and a row of 3 agents weighs less than a row of
 * 300 000.  Under the policy row i of the action is Dirichlet(a_i.) and the n_i agents of topic i each draw from that row.
 *   Data.  `sets` data sets, data set s at state + s state_stride and moves + s moves_stride (in elements; not read when
 *   sets = 1): state [N, H, d] fp32, the policy's input as the forward learners see it; moves [N, H-1, width, width] int32, of
 *   which only the corner i, j < d is read (d <= width).  set_index [policies] int32 says which data set policy k is held
 *   against; NULL: all 0.  (sets = 1: a grid search; sets = R with set_index[k] = k: one policy per bootstrap replicate.)
 *   Policy k: theta[k], shift[k], alpha_scale[k], three device fp64 arrays.
 *   Value.  Policy k, day n, transition h, row i, m_j = moves[n,h,i,j] and pi = state[n,h,.], j < d:
 *     n_i = sum_{j<d} m_j               (the agents that stay inside the d topics: the likelihood is conditional on that)
 *     x_j = (double)pi_j - (double)pi_i - shift,   a_j = alpha_scale * log1p(exp(theta * x_j))   (as mfg_policy_logpdf, no floor)
 *     A   = a_0 + ... + a_{d-1}, summed in column order
 *     T(a, m) = ln Gamma(a + m) - ln Gamma(a) = sum_{t<m} ln(a + t);  T(a, 0) = 0 exactly for every a >= 0, T(0, m > 0) = -inf
 *     ll_row = lgamma(n_i + 1) - sum_j lgamma(m_j + 1) + sum_j T(a_j, m_j) - T(A, n_i);  a row with n_i = 0 contributes exactly 0
 *     ll [policies, N, H-1]:  ll[k,n,h] = sum_i ll_row, in the order i = 0 .. d - 1 in fp64, every addition rounded on its own
 *     ll_day [policies, N]:   ll[k,n,0] + ... + ll[k,n,H-2], in that order in fp64, every addition rounded on its own
 *   Gradient.  D(a, m) = psi(a + m) - psi(a) = sum_{t<m} 1 / (a + t), D(a, 0) = 0:
 *     d ll_row / d p = sum_j D(a_j, m_j) da_j/dp - D(A, n_i) sum_j da_j/dp,   with s_j = e^(theta x_j) / (1 + e^(theta x_j)):
 *     da_j/dtheta = alpha_scale s_j x_j,   da_j/dshift = -alpha_scale s_j theta,   da_j/dln(alpha_scale) = a_j
 *     grad [policies, N, H-1, 3] and grad_day [policies, N, 3] in the order (theta, shift, ln alpha_scale), summed as the
 *     value is.  Both NULL: no gradient is formed.
 *   T and D are evaluated without the difference of two ln Gamma or two digamma values (at a ~ 1e5 and a handful of agents that
 *   difference loses ten digits): the first terms as the finite sums themselves -- all of them for m <= 8, else those that bring
 *   a to 16 --, the remaining terms from the two ends' asymptotic series combined through log1p(m / a).
 *   Failures are marked, not raised.  status [policies, N] int32, the OR over the day's transitions of
 *     bit 0 (1): a negative move in the corner (the failed-member mark of mfg_agents_step_pop) or a non-finite entry of
 *                state[n,h,0..d-1]: the value and gradient of that transition and of the day are NaN;
 *     bit 1 (2): some a_j = 0 with m_j > 0: the value is -inf, the gradient NaN;
 *     bit 2 (4): theta, shift or alpha_scale not finite, or alpha_scale <= 0: everything of that policy is NaN;
 *     bit 3 (8): set_index[k] outside [0, sets): marked on the device, nothing is read, everything of that policy is NaN.
 *   (theta x_j above 709 overflows the softplus as in mfg_policy_logpdf: NaN, no bit.)  Every NaN written is the canonical one.
 *   Independence: the outputs of policy k are the same bits alone, among any other policies, in any order and however the
 *   policies are split over calls.
 *   Launches, all on loglik->stream: one pass over the rows of the data (the multinomial coefficients, which no policy
 *   changes), the cell pass (a lane per policy and row, 64 / d policies to a wavefront), the pass over the days.
 *   Nothing is allocated or synchronised; the call can be captured.
 *   workspace: mfg_moves_loglik_workspace_bytes(policies, sets, N, H, d) bytes (0 for arguments outside the limits), 8-byte
 *   aligned; contents are scratch, and every word the call reads it has written first.
 * Checked before anything is launched.  MFG_EINVAL: a null descriptor, state, moves, parameter array, ll, ll_day or status;
 * exactly one of grad / grad_day; policies outside [1, MFG_POP_MAX_K]; N < 1; H < 2; d outside [1, 64]; d > width; sets < 1;
 * N (H - 1) > 2^31 - 1 or more rows than one launch covers; with sets > 1 a stride below one data set; a null or misaligned
 * workspace.  MFG_EWORKSPACE: workspace_bytes below the query's value. */
typedef struct mfg_moves_loglik {
  const float* state;
  const int32_t* moves;
  const int32_t* set_index;
  const double* theta;
  const double* shift;
  const double* alpha_scale;
  double* ll;
  double* ll_day;
  double* grad;
  double* grad_day;
  int32_t* status;
  void* workspace;
  size_t workspace_bytes;
  mfg_stream_t stream;
  int64_t state_stride;
  int64_t moves_stride;
  int32_t N, H;
  int32_t d, width;
  int32_t sets, policies;
} mfg_moves_loglik_t;
size_t mfg_moves_loglik_workspace_bytes(int policies, int sets, int N, int H, int d);
int mfg_moves_loglik_pop(const mfg_moves_loglik_t* loglik);

#ifdef __cplusplus
}
#endif
#endif /* MFG_HIP_H */
