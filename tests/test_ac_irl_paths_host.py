"""Host tests (no GPU, no HIP call) of the two rules AC_IRL.train rests on: which of its four episode flows a configuration
takes (ac_irl.irl_train_path) and the Philox key of a call (reward_learning.philox_call_key)."""
import itertools

import pytest

torch = pytest.importorskip('torch')

ARGS = ('update_every', 'rng', 'batch', 'world', 'has_reward_fn', 'tracing', 'write_all', 'net_supported')
GRID = (('step', 'rollout'), ('philox', 'numpy'), (1, 2), (1, 2), (False, True), (False, True), (False, True), (False, True))


def _path(**kw):
    from discrete_mean_field_game_amd.ac_irl import irl_train_path
    cfg = dict(update_every='step', rng='philox', batch=2, world=1, has_reward_fn=False, tracing=False, write_all=False,
               net_supported=True)
    cfg.update(kw)
    return irl_train_path(**cfg)


def test_every_configuration_takes_the_stated_path():
    """All 256 combinations against the conditions, restated: the booleans AC_IRL.train computed inline before the flows
    became methods."""
    from discrete_mean_field_game_amd.ac_irl import irl_train_path
    seen = set()
    for combo in itertools.product(*GRID):
        update_every, rng, batch, world, has_reward_fn, tracing, write_all, net_supported = combo
        device_draw = rng == 'philox' and batch > 1
        fused = update_every == 'rollout' and rng == 'philox' and not write_all
        native_rollout = (fused and world == 1 and not has_reward_fn and not tracing and net_supported and device_draw)
        native_step = (update_every == 'step' and rng == 'philox' and world == 1 and not has_reward_fn and not tracing
                       and not write_all and net_supported)
        want = ('native_rollout' if native_rollout else 'native_step' if native_step else 'fused_rollout' if fused
                else 'stepwise')
        assert not (native_rollout and native_step)
        assert irl_train_path(**dict(zip(ARGS, combo))) == want, dict(zip(ARGS, combo))
        assert irl_train_path(*combo) == want                 # (the documented positional order)
        seen.add(want)
    assert len(list(itertools.product(*GRID))) == 256
    assert seen == {'native_rollout', 'native_step', 'fused_rollout', 'stepwise'}


def test_the_rows_the_gpu_tests_rely_on():
    rest = list(itertools.product((1, 2), (1, 2), (False, True), (False, True), (False, True), (False, True)))
    for mode in ('step', 'rollout'):
        for batch, world, fn, tracing, write_all, net in rest:          # rng='numpy' is always the per-step loop
            assert _path(update_every=mode, rng='numpy', batch=batch, world=world, has_reward_fn=fn, tracing=tracing,
                         write_all=write_all, net_supported=net) == 'stepwise'
    assert _path(update_every='step') == 'native_step'
    assert _path(update_every='rollout') == 'native_rollout'
    assert _path(update_every='step', tracing=True) == 'stepwise'                    # `ac.trace = []`
    assert _path(update_every='rollout', has_reward_fn=True) == 'fused_rollout'      # `reward_fn=`
    assert _path(update_every='step', batch=1) == 'native_step'                      # host draw, then the native episode
    assert _path(update_every='rollout', batch=1) == 'fused_rollout'                 # no device draw
    assert _path(update_every='rollout', world=2) == 'fused_rollout'
    for combo in itertools.product(*GRID[:7]):                                       # an unsupported network: never native
        assert not _path(**dict(zip(ARGS[:7], combo)), net_supported=False).startswith('native')


def test_philox_call_key_is_the_formula():
    from discrete_mean_field_game_amd import reward_learning as RL
    assert (RL.RN_SEED_OFFSET, RL.RT_SEED_OFFSET) == (0x5EED, 0x7EA1)
    for seed, call in ((13, 1), (2 ** 64 - 1, 2 ** 40), (0, 0)):
        for offset in (RL.RN_SEED_OFFSET, RL.RT_SEED_OFFSET):
            want = ((seed + offset) ^ (call * 0x9E3779B97F4A7C15)) % 2 ** 64
            got = RL.philox_call_key(seed, offset, call)
            assert got == want and 0 <= got < 2 ** 64 and isinstance(got, int)
    assert RL.philox_call_key(0, RL.RN_SEED_OFFSET, 0) == 0x5EED
    assert RL.philox_call_key(13, RL.RN_SEED_OFFSET, 1) == ((13 + 0x5EED) ^ 0x9E3779B97F4A7C15)
