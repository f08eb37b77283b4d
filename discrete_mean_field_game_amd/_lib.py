"""ctypes binding of the C ABI in include/mfg_hip.h (libmfg_hip.so, built in-tree by csrc/Makefile).

There is deliberately NO fallback: if the HIP library is missing or a call fails, an exception is
raised.  The product path never routes through the CPU oracle.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, 'csrc')
LIB_PATH = os.environ.get('MFG_HIP_LIB') or os.path.join(CSRC, 'libmfg_hip.so')   # MFG_HIP_LIB: alternative build

MFG_MAX_D = 512
REWARD_MFG_AC2, REWARD_SYNTHETIC, REWARD_EXTERNAL = 0, 1, 2
ROLLOUT_WRITE_P, ROLLOUT_TD, ROLLOUT_DISCOUNT_POW, ROLLOUT_F64, TRAIN_APPLY = 1, 2, 4, 8, 16
PRECISION_F64, PRECISION_MIXED = 0, 1
POP_MAX_K = 65535                # MFG_POP_MAX_K: learners of one population call
POP_RESIDENT_MAX_TILES = 64      # MFG_POP_RESIDENT_MAX_TILES: tiles of one learner the resident step-mode kernel walks
STATUS_MIXED_RANGE = 1
STATUS_POP_NONFINITE = 2        # MFG_STATUS_POP_NONFINITE: per-learner words of a population control block only
ECOMM = -6                      # MFG_ECOMM: the call aborted its RCCL communicator, the handle is dead
RN_TRAIN_MAX_TRAJ = 64          # MFG_RN_TRAIN_MAX_TRAJ
FORECAST_MAX_RANKS = 8          # MFG_FORECAST_MAX_RANKS: order statistics of one mfg_forecast_pop call
FORECAST_MAX_REPEATS = 1024     # MFG_FORECAST_MAX_REPEATS: members per start state of one mfg_forecast_pop call
FORECAST_SCORE_TILE = 64        # MFG_FORECAST_SCORE_TILE: members per tile of mfg_forecast_score's energy pass
AGENTS_MAX = 1 << 24            # MFG_AGENTS_MAX: agents of one finite-population member
DIST_MAX_BINS = 1024            # MFG_DIST_MAX_BINS: histogram bins of one mfg_row_distribution call
DIST_MAX_GRID = 4096            # MFG_DIST_MAX_GRID: KDE grid points of one mfg_row_distribution call
DIST_NONFINITE, DIST_NO_KDE = 1, 2      # MFG_DIST_NONFINITE / MFG_DIST_NO_KDE: bits of a row's status
PRECISIONS = {'f64': PRECISION_F64, 'mixed': PRECISION_MIXED, 0: 0, 1: 1}


class MfgError(RuntimeError):
    code = 0                    # the negative MFG_E* code of the failed call (0 for errors raised on the Python side)


def build(force: bool = False) -> str:
    """Compile csrc/ for gfx950 with hipcc (cross-compiles without a GPU)."""
    args = ['make', '-C', CSRC]
    if force:
        args.append('-B')
    subprocess.run(args, check=True, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    return LIB_PATH


_p = C.c_void_p
_i64, _i32, _u64, _u32, _f64, _sz = C.c_int64, C.c_int, C.c_uint64, C.c_uint32, C.c_double, C.c_size_t

# symbol -> (restype, argtypes); mirrors include/mfg_hip.h one to one
SIGNATURES = {
    'mfg_last_error': (C.c_char_p, []),
    'mfg_abi_version': (_i32, []),
    'mfg_set_core_mapping': (_i32, [_i32]),   # 0 auto, 1 packed, 2 one trajectory per wave, 3 packed without k_core_small_lean
    'mfg_init': (_i32, []),
    'mfg_status': (_i32, [C.POINTER(C.c_uint)]),
    'mfg_clear_status': (_i32, []),
    'mfg_ctx_create': (_i32, [C.POINTER(C.c_void_p)]),
    'mfg_ctx_destroy': (_i32, [_p]),
    'mfg_ctx_bind': (_i32, [_p]),
    'mfg_ctx_current': (_p, []),
    'mfg_ctx_status': (_i32, [_p, C.POINTER(C.c_uint)]),
    'mfg_ctx_clear_status': (_i32, [_p]),
    'mfg_ctx_adopt_comm': (_i32, [_p, _p]),
    'mfg_ctx_comm': (_p, [_p]),
    'mfg_device_info': (_i32, [C.POINTER(C.c_int), C.c_char_p, _i32]),
    'mfg_feature_index': (_i64, [_i32, _i32, _i32]),
    'mfg_num_features': (_i64, [_i32]),
    'mfg_workspace_bytes': (_sz, [_i64, _i32]),
    'mfg_gather_start': (_i32, [_p, _i64, _p, _i64, _i32, _p, _p]),
    'mfg_draw_start': (_i32, [_p, _i64, _i64, _i32, _u64, _u32, _u64, _p, _p, _p]),
    'mfg_alpha': (_i32, [_p, _i64, _i32, _p, _f64, _p, _p, _p]),
    'mfg_dirichlet_from_gamma': (_i32, [_p, _i64, _i32, _p, _p]),
    'mfg_sample_dirichlet': (_i32, [_p, _i64, _i32, _p, _f64, _f64, _u64, _u32, _u64, _i32, _p, _p]),
    'mfg_philox_raw': (_i32, [_u64, _u32, _u32, _u32, _u32, _i64, _p, _p]),
    'mfg_step_given_P': (_i32, [_p, _p, _i64, _i32, _i32, _p, _p, _p]),
    'mfg_value': (_i32, [_p, _p, _i64, _i32, _p, _p]),
    'mfg_features': (_i32, [_p, _i64, _i32, _p, _p]),
    'mfg_score': (_i32, [_p, _p, _i64, _i32, _p, _f64, _i32, _p, _p]),
    'mfg_td_pg_accumulate': (_i32, [_p, _p, _p, _p, _p, _p, _f64, _f64, _i64, _i32, _i32, _p, _p, _p, _i32, _p, _sz,
                                   _p]),
    'mfg_apply_update': (_i32, [_p, _i32, _f64, _f64, _p, _p, _p, _p]),
    'mfg_rollout': (_i32, [_p, _i64, _i32, _i32, _p, _f64, _f64, _p, _f64, _i32, _u64, _u32, _u64, _i32,
                           _p, _p, _p, _p, _p, _p, _p, _i32, _p, _sz, _p]),
    'mfg_jsd': (_i32, [_p, _p, _i64, _i32, _p, _p]),
    'mfg_grad_accumulate': (_i32, [_p, _i64, _p, _p, _p, _i64, _i32, _i32, _i32, _p, _i32, _p, _sz, _p]),
    'mfg_grad_apply': (_i32, [_p, _i64, _p, _p, _p, _i64, _i32, _i32, _i32, _p, _f64, _f64, _p, _p, _p, _p, _sz, _p]),
    'mfg_train_episode': (_i32, [_p, _p, _i64, _i32, _i32, _p, _f64, _f64, _p, _f64, _i32, _u64, _u32, _u64, _i32, _f64, _f64,
                                 _p, _p, _p, _p, _p, _p, _sz, _p]),
    'mfg_train_rollout': (_i32, [_p, _i64, _p, _i64, _i32, _i32, _p, _f64, _f64, _p, _f64, _i32, _u64, _u32, _u64, _i32, _f64,
                                 _f64, _p, _p, _p, _p, _p, _p, _p, _p, _sz, _p]),
    'mfg_train_rollouts': (_i32, [_p, _i64, _i64, _i32, _i32, _i64, _i64, _i32, _p, _f64, _f64, _p, _f64, _i32, _u64, _u32, _u64,
                                  _i32, _f64, _f64, _p, _p, _p, _p, _p, _p, _p, _p, _sz, _p]),
    'mfg_train_rollout_deferred': (_i32, [_p, _i64, _p, _i64, _i32, _i32, _p, _p, _p, _f64, _f64, _p, _p, _p, _f64, _f64, _f64,
                                          _i32, _u64, _u32, _u64, _i32, _p, _p, _p, _p, _p, _p, _p, _sz, _p]),
    'mfg_train_episodes': (_i32, [_p, _i64, _p, _p, _i64, _i32, _i32, _i64, _i64, _i32, _p, _f64, _f64, _p, _f64, _i32, _u64, _u32,
                                  _u64, _i32, _f64, _f64, _p, _p, _p, _p, _p, _p, _sz, _p]),
    'mfg_train_episodes_pop': (_i32, [_p, _i64, _p, _p, _i64, _i32, _i32, _i32, _i64, _i64, _i32, _p, _p, _p, _p, _f64, _i32, _p,
                                      _u32, _u64, _i32, _p, _p, _p, _p, _p, _p, _p, _p, _sz, _p]),
    'mfg_train_rollouts_pop': (_i32, [_p, _i64, _i64, _i32, _i32, _i32, _i64, _i64, _i32, _p, _p, _p, _p, _f64, _i32, _p, _u32, _u64,
                                      _i32, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _sz, _p]),
    'mfg_dist_available': (_i32, []),
    'mfg_dist_unique_id': (_i32, [_p]),
    'mfg_dist_init': (_i32, [_p, _i32, _i32, C.POINTER(C.c_void_p)]),
    'mfg_dist_destroy': (_i32, [_p]),
    'mfg_dist_abort': (_i32, [_p]),
    'mfg_dist_all_reduce': (_i32, [_p, _p, _i64, _p]),
    'mfg_train_rollouts_dist': (_i32, [_p, _p, _i64, _i64, _i32, _i32, _i64, _i64, _i32, _p, _p, _p, _p, _f64, _f64, _f64, _i32, _u64,
                                       _u32, _u64, _i32, _f64, _f64, _p, _p, _p, _p, _p, _p, _p, _p, _sz, _p]),
    'mfg_policy_logpdf': (_i32, [_p, _p, _i64, _i32, _p, _i32, _f64, _f64, _f64, _f64, _p, _p]),
    'mfg_backward_value': (_i32, [_p, _i64, _i32, _i32, _p, _p, _p, _p]),
    'mfg_reward_net_forward': (_i32, [_p, _p, _i64, _i32, _i32, _i32, _i32, _i32, _i32, _p, _p, _p, _p, _p, _p, _p, _p, _p,
                                     _p, C.c_float, _u64, _u64, _p, _p]),
    'mfg_reward_net_num_params': (_i64, [_i32, _i32, _i32, _i32, _i32, _i32]),
    'mfg_reward_net_param_offsets': (_i32, [_i32, _i32, _i32, _i32, _i32, _i32, C.POINTER(C.c_int64)]),
    'mfg_reward_net_train_workspace_bytes': (_sz, [_i32, _i32, _i32, _i32, _i32, _i32, _i64]),
    'mfg_reward_net_train_step': (_i32, [_p, _p, _p, _i32, _i32, _i32, _i32, _i32, _i32, _p, _p, C.POINTER(C.c_int32), _i32, _p, _p,
                                        C.POINTER(C.c_int32), _i32, _i32, _i32, C.c_float, _i32, _u64, _f64, _f64, _f64, _f64, _i64,
                                        _i32, _p, _p, _p, _sz, _p]),
    'mfg_reward_net_adam': (_i32, [_p, _p, _p, _p, _i64, _f64, _f64, _f64, _f64, _i64, _p]),
    'mfg_traj_log_z_pop': (_i32, [_p, _p, _i64, C.POINTER(C.c_int32), _i32, _i32, _i32, _p, _i32, _p, _i32, _i32, _f64, _f64, _f64,
                                 _f64, _p, _p, _sz, _p]),
}
# the resident step-mode episodes of a small-batch population: the per-step call's arguments
SIGNATURES['mfg_pop_resident_supported'] = (_i32, [_i32, _i64, _i32])
SIGNATURES['mfg_train_episodes_pop_resident'] = (_i32, list(SIGNATURES['mfg_train_episodes_pop'][1]))
# the importance-weighted training steps: the unweighted call's arguments with gen_log_z in front of the stream
SIGNATURES['mfg_reward_net_train_step_z'] = (_i32, SIGNATURES['mfg_reward_net_train_step'][1][:-1] + [_p, _p])


class RewardNetStruct(C.Structure):
    """mfg_reward_net_t of include/mfg_hip.h."""
    _fields_ = ([(n, C.c_int) for n in ('k1', 'f2', 'k2', 'n3', 'n4')]
                + [(n, C.c_void_p) for n in ('conv1_w', 'conv1_b', 'conv2_w', 'conv2_b', 'fc3_w', 'fc3_b', 'fc4_w', 'fc4_b',
                                             'out_w', 'out_b')]
                + [('keep_prob', C.c_float)])


SIGNATURES['mfg_train_episode_irl'] = (_i32, [_p, _p, _i64, _i32, _i32, _p, _f64, _f64, _p, _f64, _u64, _u32, _u64, _i32, _f64,
                                              _f64, C.POINTER(RewardNetStruct), _u64, _u64, _u64, _p, _p, _p, _p, _p, _p, _p,
                                              _sz, _p])

SIGNATURES['mfg_train_episode_irl_draw'] = (_i32, [_p, _i64] + SIGNATURES['mfg_train_episode_irl'][1])

SIGNATURES['mfg_train_rollout_irl'] = (_i32, [_p, _i64, _p, _i64, _i32, _i32, _p, _f64, _f64, _p, _f64, _u64, _u32, _u64, _i32, _f64,
                                              _f64, C.POINTER(RewardNetStruct), _u64, _u64, _p, _p, _p, _p, _p, _p, _p, _p, _p, _sz,
                                              _p])

class RnGeomStruct(C.Structure):
    """mfg_rn_geom_t of include/mfg_hip.h: one learner's n_fc3, n_fc4, keep_prob and l1_l2 flag (16 bytes)."""
    _fields_ = [('n3', C.c_int32), ('n4', C.c_int32), ('keep_prob', C.c_float), ('l1l2', C.c_int32)]


class RnTrainPlan(C.Structure):
    """mfg_rn_train_plan_t of include/mfg_hip.h: one update_reward of one learner of mfg_reward_net_train_steps_pop."""
    _fields_ = [('learner', C.c_int32), ('lr_t', C.c_float), ('key', C.c_uint64), ('lr', C.c_double), ('adam_step', C.c_int64),
                ('demo_rows', C.c_int32 * RN_TRAIN_MAX_TRAJ), ('gen_rows', C.c_int32 * RN_TRAIN_MAX_TRAJ)]


# the IRL population calls: ..., net, per_learner_net, net_stride, geom_host, geom_dev (the optional geometry table: two NULLs
# without one), rn_seed [K], rn_call0 [K], ...
SIGNATURES['mfg_train_episodes_irl_pop'] = (_i32, [_p, _i64, _p, _p, _i64, _i32, _i32, _i32, _i64, _i64, _i32, _p, _p, _p, _p, _f64,
                                                   _p, _u32, _u64, _i32, _p, _p, C.POINTER(RewardNetStruct), _i32, _i64, _p, _p,
                                                   _p, _p, _p, _p, _p, _p, _p, _p, _p, _sz, _p])

SIGNATURES['mfg_train_rollouts_irl_pop'] = (_i32, [_p, _i64, _i64, _i32, _i32, _i32, _i64, _i64, _i32, _p, _p, _p, _p, _f64, _p,
                                                   _u32, _u64, _i32, _p, _p, C.POINTER(RewardNetStruct), _i32, _i64, _p, _p, _p,
                                                   _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _sz, _p])

SIGNATURES['mfg_reward_net_forward_pop'] = (_i32, [_p, _p, _i64, _i64, _i64, _i32, C.POINTER(RewardNetStruct), _i32, _i64, _p, _p,
                                                   _i32, _p, _p, _i32, _u64, _p, _p, _sz, _p])

SIGNATURES['mfg_reward_net_train_steps_pop'] = (_i32, [_p, _p, _p, _i64, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _p, _p, _p, _p,
                                                       _i64, _p, _p, _i64, _p, _p, _sz, _i32, _i32, _i32, _i32, _i32, _i32,
                                                       C.c_float, _i32, _f64, _f64, _f64, _p, _p, _sz, _p])

SIGNATURES['mfg_reward_net_train_steps_pop_z'] = (_i32, SIGNATURES['mfg_reward_net_train_steps_pop'][1][:-1] + [_p, _p])


class PopControlStruct(C.Structure):
    """mfg_pop_control_t of include/mfg_hip.h: the per-learner activity states of a population (device arrays [K])."""
    _fields_ = [('state', C.c_void_p), ('status', C.c_void_p), ('theta_prev', C.c_void_p), ('episodes_run', C.c_void_p),
                ('stop_criteria', C.c_void_p), ('K', C.c_int32)]


SIGNATURES['mfg_ctx_set_pop_control'] = (_i32, [_p, C.POINTER(PopControlStruct)])

POP_VALIDATE_COLUMNS = 10       # MFG_POP_VALIDATE_COLUMNS: columns of a validation curve row


class PopValidateStruct(C.Structure):
    """mfg_pop_validate_t of include/mfg_hip.h: the held-out checks a population training call runs every `period` episodes."""
    _fields_ = ([(n, C.c_void_p) for n in ('emp32', 'emp64', 'curve', 'checks', 'best_value', 'best_check', 'since_best',
                                           'best_theta', 'best_w', 'workspace')]
                + [('workspace_bytes', C.c_size_t), ('N', C.c_int64)]
                + [(n, C.c_int32) for n in ('L', 'repeats', 'period', 'column', 'with_score', 'patience', 'max_checks', 'K')]
                + [('first_step', C.c_uint32)])


SIGNATURES['mfg_ctx_set_pop_validate'] = (_i32, [_p, C.POINTER(PopValidateStruct)])
SIGNATURES['mfg_pop_validate_workspace_bytes'] = (_sz, [_i64, _i32, _i32, _i32, _i32, _i32])


class PopEvolveStruct(C.Structure):
    """mfg_pop_evolve_t of include/mfg_hip.h: the exploit / explore steps a population training call runs behind its checks."""
    _fields_ = ([(n, C.c_void_p) for n in ('lr_critic', 'lr_actor', 'order', 'active', 'rank', 'parent', 'lr_log')]
                + [('seed', C.c_uint64)]
                + [(n, C.c_double) for n in ('factor_down', 'factor_up', 'lr_critic_min', 'lr_critic_max', 'lr_actor_min',
                                             'lr_actor_max')]
                + [(n, C.c_int32) for n in ('every', 'n_top', 'n_bottom', 'perturb', 'max_steps', 'K')])


SIGNATURES['mfg_ctx_set_pop_evolve'] = (_i32, [_p, C.POINTER(PopEvolveStruct)])

SIGNATURES['mfg_evaluate_pop_workspace_bytes'] =(_sz, [_i64, _i32, _i32, _i32, _i32, _i32])
SIGNATURES['mfg_evaluate_pop'] = (_i32, [_p, _p, _i64, _i32, _i32, _i32, _p, _p, _p, _p, _u32, _i32, _i32, _p, _p, _p, _sz, _p])

# the ensemble forecast: start32, N, H, d, K, theta, shift, alpha_scale, seed, first_step, repeats, precision, ranks (host), Q,
# emp32, emp64, mean, std, quant, curves, pi_traj, workspace, workspace_bytes, stream
SIGNATURES['mfg_forecast_pop_workspace_bytes'] = (_sz, [_i64, _i32, _i32, _i32, _i32, _i32])
SIGNATURES['mfg_forecast_pop'] = (_i32, [_p, _i64, _i32, _i32, _i32, _p, _p, _p, _p, _u32, _i32, _i32, C.POINTER(C.c_int32), _i32,
                                         _p, _p, _p, _p, _p, _p, _p, _p, _sz, _p])

# the proper scores of given members: traj, N, H, d, K, repeats, emp32, emp64, crps, less, equal, energy, summary, workspace,
# workspace_bytes, stream
SIGNATURES['mfg_forecast_score_workspace_bytes'] = (_sz, [_i64, _i32, _i32, _i32, _i32])
SIGNATURES['mfg_forecast_score'] = (_i32, [_p, _i64, _i32, _i32, _i32, _i32, _p, _p, _p, _p, _p, _p, _p, _p, _sz, _p])

# finite-population members.  step: counts, P, B, d, K, agents, seed, step, traj_offset, counts_next, pi_next, moves, stream;
# forecast: mfg_forecast_pop's arguments with counts0 for start32, `agents` behind K, counts_traj and actions behind pi_traj
SIGNATURES['mfg_agents_step_pop'] = (_i32, [_p, _p, _i64, _i32, _i32, _i32, _p, _u32, _u64, _p, _p, _p, _p])
SIGNATURES['mfg_forecast_agents_pop_workspace_bytes'] = (_sz, [_i64, _i32, _i32, _i32, _i32, _i32, _i32])
SIGNATURES['mfg_forecast_agents_pop'] = (_i32, [_p, _i64, _i32, _i32, _i32, _i32, _p, _p, _p, _p, _u32, _i32, _i32,
                                                C.POINTER(C.c_int32), _i32, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _sz, _p])

# the backward-equation check.  given: P, K, M, T, d, metrics, steps, V, workspace, workspace_bytes, stream; pop: start32, N, H,
# d, K, theta, shift, alpha_scale, seed, first_step, repeats, precision, metrics, steps, V, actions, pi_traj, workspace,
# workspace_bytes, stream
SIGNATURES['mfg_consistency_given_workspace_bytes'] = (_sz, [_i32, _i64, _i32, _i32])
SIGNATURES['mfg_consistency_given'] = (_i32, [_p, _i32, _i64, _i32, _i32, _p, _p, _p, _p, _sz, _p])
SIGNATURES['mfg_consistency_pop_workspace_bytes'] = (_sz, [_i64, _i32, _i32, _i32, _i32, _i32, _i32, _i32])
SIGNATURES['mfg_consistency_pop'] = (_i32, [_p, _i64, _i32, _i32, _i32, _p, _p, _p, _p, _u32, _i32, _i32, _p, _p, _p, _p, _p, _p,
                                            _sz, _p])

# the distribution summary of R rows: values, R, N, stride, bins, use_range, lo, hi, G, x_lo, x_hi, moments, counts, edges,
# density, status, workspace, workspace_bytes, stream; the mean action matrices: action, s_action, K, N, d, mean, workspace,
# workspace_bytes, stream
SIGNATURES['mfg_row_distribution_workspace_bytes'] = (_sz, [_i32, _i64, _i32, _i32])
SIGNATURES['mfg_row_distribution'] = (_i32, [_p, _i32, _i64, _i64, _i32, _i32, _f64, _f64, _i32, _f64, _f64, _p, _p, _p, _p, _p, _p,
                                             _sz, _p])
SIGNATURES['mfg_action_mean_pop_workspace_bytes'] = (_sz, [_i32, _i64, _i32])
SIGNATURES['mfg_action_mean_pop'] = (_i32, [_p, _i64, _i32, _i64, _i32, _p, _p, _sz, _p])


class RnInputGradStruct(C.Structure):
    """mfg_rn_input_grad_t of include/mfg_hip.h: the reward input-gradient block that rides on mfg_reward_net_forward_pop."""
    _fields_ = ([(n, C.c_void_p) for n in ('grad_state', 'grad_action', 'mean_state', 'mean_action', 'workspace')]
                + [('workspace_bytes', C.c_size_t), ('N', C.c_int64)]
                + [(n, C.c_int32) for n in ('K', 'd', 'reserved')])


SIGNATURES['mfg_rn_input_grad_workspace_bytes'] = (_sz, [_i32, _i64, _i32])
SIGNATURES['mfg_ctx_set_rn_input_grad'] = (_i32, [_p, C.POINTER(RnInputGradStruct)])

VAR_MAX_REGRESSORS = 512        # MFG_VAR_MAX_REGRESSORS: 1 + lag d of one model of mfg_var_fit_pop
VAR_MAX_D, VAR_MAX_HOURS, VAR_MAX_DAYS = 64, 64, 64     # its limits on d, Hd and the training / test days of one model
VAR_NONFINITE, VAR_PIVOT = 1, 2                         # MFG_VAR_NONFINITE / MFG_VAR_PIVOT: bits of a model's status


class VarModelStruct(C.Structure):
    """mfg_var_model_t of include/mfg_hip.h: one model of mfg_var_fit_pop (32 bytes)."""
    _fields_ = ([(n, C.c_int32) for n in ('lag', 'origin', 'n_train', 'n_test')]
                + [('ridge', C.c_double), ('ws_offset', C.c_int64)])


class VarFitStruct(C.Structure):
    """mfg_var_fit_t of include/mfg_hip.h: the descriptor of one mfg_var_fit_pop call; the stream is a member."""
    _fields_ = ([(n, C.c_void_p) for n in ('days', 'models_host', 'models', 'train_idx', 'test_idx', 'coef', 'sse', 'insample',
                                           'future', 'per_day', 'metrics', 'status', 'workspace')]
                + [('workspace_bytes', C.c_size_t), ('stream', C.c_void_p)]
                + [(n, C.c_int32) for n in ('D', 'Hd', 'd', 'K', 'train_stride', 'test_stride', 'M', 'S_max')])


SIGNATURES['mfg_var_fit_workspace_bytes'] = (_sz, [_i32, C.POINTER(VarModelStruct), _i32])
SIGNATURES['mfg_var_fit_pop'] = (_i32, [C.POINTER(VarFitStruct)])

RNN_MAX_D, RNN_MAX_HIDDEN, RNN_MAX_HOURS, RNN_MAX_DAYS = 64, 64, 64, 64     # the limits of one model of mfg_rnn_fit_pop
RNN_MAX_EPOCHS = 65535                                  # MFG_RNN_MAX_EPOCHS
RNN_ADAM, RNN_SGD = 0, 1                                # MFG_RNN_ADAM / MFG_RNN_SGD
RNN_NONFINITE, RNN_DIVERGED = 1, 2                      # MFG_RNN_NONFINITE / MFG_RNN_DIVERGED: bits of a model's status


class RnnModelStruct(C.Structure):
    """mfg_rnn_model_t of include/mfg_hip.h: one model of mfg_rnn_fit_pop (56 bytes)."""
    _fields_ = ([(n, C.c_int32) for n in ('hidden', 'epochs', 'n_train', 'n_val', 'n_test', 'reserved')]
                + [(n, C.c_double) for n in ('lr', 'wd', 'clip')] + [('ws_offset', C.c_int64)])


class RnnFitStruct(C.Structure):
    """mfg_rnn_fit_t of include/mfg_hip.h: the descriptor of one mfg_rnn_fit_pop call; the stream is a member."""
    _fields_ = ([(n, C.c_void_p) for n in ('days', 'models_host', 'models', 'train_idx', 'val_idx', 'test_idx', 'w0', 'weights',
                                           'loss', 'val', 'best_epoch', 'future', 'per_day', 'metrics', 'status', 'workspace')]
                + [('workspace_bytes', C.c_size_t), ('stream', C.c_void_p)]
                + [(n, C.c_int32) for n in ('D', 'Hd', 'd', 'K', 'train_stride', 'val_stride', 'test_stride', 'W_max', 'E_max',
                                            'C_max', 'optimizer', 'eval_every')])


SIGNATURES['mfg_rnn_fit_workspace_bytes'] = (_sz, [_i32, C.POINTER(RnnModelStruct), _i32, _i32])
SIGNATURES['mfg_rnn_fit_pop'] = (_i32, [C.POINTER(RnnFitStruct)])

DEMOS_MAX_C, DEMOS_MAX_WIDTH = 4096, 64         # MFG_DEMOS_MAX_C; the width limit of mfg_demos_from_logs (as the populations' d)
DEMOS_CHUNK = 8192                              # MFG_DEMOS_CHUNK: agents of one day that one workgroup of the counting pass owns
DEMOS_ORDERS = {'first_hour': 0, 'total': 1, 'given': 2}        # MFG_DEMOS_ORDER_*
DEMOS_EMPTY_ROWS = {'uniform': 0, 'identity': 1}                # MFG_DEMOS_EMPTY_*
DEMOS_LDS_UPDATES = {'plain': 0, 'combine': 1}                  # MFG_DEMOS_LDS_*
DEMOS_BAD_VALUE, DEMOS_EMPTY_HOUR, DEMOS_FAILED = 1, 2, 4       # bits of a day's status


class DemosStruct(C.Structure):
    """mfg_demos_t of include/mfg_hip.h: the descriptor of one mfg_demos_from_logs call; the stream is a member."""
    _fields_ = ([(n, C.c_void_p) for n in ('topic', 'order_given', 'state', 'action', 'counts', 'moves', 'order', 'present', 'left',
                                           'entered', 'status', 'workspace')]
                + [('workspace_bytes', C.c_size_t), ('stream', C.c_void_p), ('U', C.c_int64)]
                + [(n, C.c_int32) for n in ('N', 'H', 'C', 'd', 'width', 'order_mode', 'empty_row', 'order_given_rows', 'lds_update',
                                            'groups')])


SIGNATURES['mfg_demos_workspace_bytes'] = (_sz, [_i32, _i32, _i32, _i32])
SIGNATURES['mfg_demos_from_logs'] = (_i32, [C.POINTER(DemosStruct)])

DEMOS_BOOT_MAX_R = 1024                         # MFG_DEMOS_BOOT_MAX_R
DEMOS_BOOT_TAG = 0xB007                         # MFG_DEMOS_BOOT_TAG: the low 16 bits of the fourth counter word of a weight's draw
DEMOS_UNITS = {'agent_day': 0, 'agent': 1}      # MFG_DEMOS_UNIT_*
DEMOS_BOOT_TABLE = (1580030168, 3160060337, 3950075421, 4213413783, 4279248373, 4292415291, 4294609777, 4294923276, 4294962463,
                    4294966817, 4294967252, 4294967292)       # MFG_DEMOS_BOOT_TABLE: floor(2^32 CDF of Poisson(1))


class DemosBootStruct(C.Structure):
    """mfg_demos_boot_t of include/mfg_hip.h: the descriptor of one mfg_demos_bootstrap call; the stream is a member."""
    _fields_ = ([(n, C.c_void_p) for n in ('topic', 'rank', 'state', 'action', 'counts', 'moves', 'present', 'left', 'entered',
                                           'status', 'workspace')]
                + [('workspace_bytes', C.c_size_t), ('stream', C.c_void_p), ('U', C.c_int64), ('seed', C.c_uint64),
                   ('day_offset', C.c_int64)]
                + [(n, C.c_int32) for n in ('N', 'H', 'C', 'd', 'width', 'R', 'rank_rows', 'unit', 'empty_row', 'groups')])


class ReplicateBandsStruct(C.Structure):
    """mfg_replicate_bands_t of include/mfg_hip.h."""
    _fields_ = ([(n, C.c_void_p) for n in ('x', 'mean', 'std', 'quant', 'stream')]
                + [('cells', C.c_int64), ('R', C.c_int32), ('Q', C.c_int32), ('ranks', C.c_int32 * FORECAST_MAX_RANKS)])


SIGNATURES['mfg_demos_bootstrap_workspace_bytes'] = (_sz, [_i32, _i32, _i32, _i32, _i32])
SIGNATURES['mfg_demos_bootstrap'] = (_i32, [C.POINTER(DemosBootStruct)])
SIGNATURES['mfg_replicate_bands'] = (_i32, [C.POINTER(ReplicateBandsStruct)])

MOVES_LOGLIK_MAX_D = 64                         # the d limit of mfg_moves_loglik_pop
MOVES_LOGLIK_BAD_DATA, MOVES_LOGLIK_ZERO_ALPHA, MOVES_LOGLIK_BAD_POLICY, MOVES_LOGLIK_BAD_SET = 1, 2, 4, 8     # bits of status[k, n]


class MovesLoglikStruct(C.Structure):
    """mfg_moves_loglik_t of include/mfg_hip.h: the descriptor of one mfg_moves_loglik_pop call; the stream is a member."""
    _fields_ = ([(n, C.c_void_p) for n in ('state', 'moves', 'set_index', 'theta', 'shift', 'alpha_scale', 'll', 'll_day', 'grad',
                                           'grad_day', 'status', 'workspace')]
                + [('workspace_bytes', C.c_size_t), ('stream', C.c_void_p), ('state_stride', C.c_int64), ('moves_stride', C.c_int64)]
                + [(n, C.c_int32) for n in ('N', 'H', 'd', 'width', 'sets', 'policies')])


SIGNATURES['mfg_moves_loglik_workspace_bytes'] = (_sz, [_i32, _i32, _i32, _i32, _i32])
SIGNATURES['mfg_moves_loglik_pop'] = (_i32, [C.POINTER(MovesLoglikStruct)])

_lib = None


def lib():
    """Load libmfg_hip.so (once) and bind every symbol.  Raises MfgError when it is missing."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise MfgError('HIP extension not built: %s is missing (run __graft_entry__.build() / make -C %s)'
                           % (LIB_PATH, CSRC))
        # PyTorch-ROCm brings its own libamdhip64; whichever copy is loaded FIRST owns the process.  Loading this library
        # before torch binds it to /opt/rocm's runtime, torch then loads a second one, and kernels / symbols registered
        # with one runtime are unknown to the other ("h(z) table initialisation failed").  So torch goes first.
        import torch  # noqa: F401
        handle = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(handle, name)
            fn.restype = res
            fn.argtypes = args
        _lib = handle
    return _lib


def check(rc: int, what: str):
    if rc != 0:
        err = MfgError('%s failed (%d): %s' % (what, rc, lib().mfg_last_error().decode()))
        err.code = int(rc)
        raise err
