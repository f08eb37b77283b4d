"""CPU checks of AC_IRLPopulation's reward half: argument validation, the batch draws (the random.sample sequences of
AC_IRL.update_reward on each learner's own random.Random), lr_t of mfg_reward_net_train_steps_pop and the new bindings."""
import ctypes as C
import os
import random

import numpy as np
import pytest

T = 15
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('mfg_reward_net_train_steps_pop', 'mfg_reward_net_forward_pop', 'mfg_train_episodes_irl_pop', 'mfg_train_rollouts_irl_pop')


@pytest.fixture(scope='module')
def lib():
    from discrete_mean_field_game_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib


def _demos(d, n, steps=T):
    rs = np.random.RandomState(0)
    return [[(rs.rand(d), rs.rand(d, d)) for _ in range(steps)] for _ in range(n)]


def test_demonstrations_validation():
    from discrete_mean_field_game_amd.irl_population import check_demonstrations
    for bad in (None, [], [_demos(15, 1)[0][:14]], _demos(15, 2) + [_demos(15, 1, steps=16)[0]]):
        with pytest.raises(ValueError):
            check_demonstrations(bad, 15)
    s, a = check_demonstrations(_demos(21, 3), 21)
    assert s.shape == (3, T, 21) and a.shape == (3, T, 21, 21) and s.dtype == np.float32


def test_batch_limits():
    from discrete_mean_field_game_amd.irl_population import batch_fits
    assert batch_fits(5, 5, 16)
    assert batch_fits(5, 0, 8)
    assert not batch_fits(65, 0, 1)            # MFG_RN_TRAIN_MAX_TRAJ per batch half
    assert not batch_fits(40, 40, 16)          # c_n dz3_n beyond 60 KB of LDS


def test_draws_match_random_sample():
    from discrete_mean_field_game_amd.irl_population import draw_batches
    for seed, nd, ng in ((3, 7, 20), (11, 5, 4), (0, 2, 9)):
        mine = draw_batches(random.Random(seed), nd, ng, 12)
        state = random.getstate()
        try:
            random.seed(seed)
            ref = []
            for _ in range(12):        # AC_IRL.update_reward's two calls per update
                di = random.sample(range(nd), 5) if nd >= 5 else list(range(nd))
                gi = random.sample(range(ng), 5) if ng >= 5 else list(range(ng))
                ref.append((di, gi))
        finally:
            random.setstate(state)
        assert mine == ref


def test_plan_layout_and_lr_t(lib):
    """The plan entries have the C layout; the call writes lr_t with the single step's rounding before it touches the GPU (a
    too small plan_dev is refused after the plan is checked, so no HIP call is made here)."""
    from discrete_mean_field_game_amd import ops
    assert C.sizeof(lib.RnTrainPlan) == 544 and ops.rn_train_plan(1).itemsize == 544
    plan = ops.rn_train_plan(6)
    for i in range(6):
        plan[i]['learner'] = i % 3
        plan[i]['lr'] = [1e-4, 3e-3, 0.0][i % 3]
        plan[i]['adam_step'] = 1 + 7 * i
    dummy = C.c_void_p(16)
    rc = lib.lib().mfg_reward_net_train_steps_pop(dummy, dummy, dummy, 7296, 3, 21, 5, 2, 3, 8, 4, None, None, dummy, dummy, 10,
                                                 dummy, dummy, 10, plan.ctypes.data, dummy, 0, 2, 3, 5, 5, T, 5, 0.4, 1, 0.9,
                                                 0.999, 1e-8, dummy, dummy, 1 << 30, None)
    assert rc == -4                          # MFG_EWORKSPACE: plan_dev
    for e in plan:
        t = int(e['adam_step'])
        ref = np.float32(float(e['lr']) * np.sqrt(1.0 - 0.999 ** t) / (1.0 - 0.9 ** t))
        assert np.float32(e['lr_t']) == ref
    bad = plan.copy()
    bad[5]['learner'] = 1                     # learner 1 twice in update 1 (plan_dev_bytes 0: nothing can reach the GPU)
    assert lib.lib().mfg_reward_net_train_steps_pop(dummy, dummy, dummy, 7296, 3, 21, 5, 2, 3, 8, 4, None, None, dummy, dummy, 10,
                                                   dummy, dummy, 10, bad.ctypes.data, dummy, 0, 2, 3, 5, 5, T, 5, 0.4, 1, 0.9,
                                                   0.999, 1e-8, dummy, dummy, 1 << 30, None) == -1


def test_new_bindings_declared_and_exported(lib):
    text = open(os.path.join(ROOT, 'include', 'mfg_hip.h')).read()
    handle = lib.lib()
    for name in NEW:
        assert name + '(' in text
        assert name in lib.SIGNATURES
        assert getattr(handle, name) is not None
    assert handle.mfg_abi_version() == 18
