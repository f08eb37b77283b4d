"""CPU checks of the resident step-mode population path (mfg_train_episodes_pop_resident): the shapes the library serves,
the rule that chooses the path, the constructor's and train()'s refusals as pure functions, and the binding."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def lib():
    from discrete_mean_field_game_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib


# (d, B, reward_kind) -> served: d = 21 tiles of 12, d = 15 tiles of 16, 1 .. 64 tiles; in-kernel rewards 0 / 1 only
TRUTH = [(21, 1, 0, 1), (21, 2, 0, 1), (21, 12, 1, 1), (21, 13, 0, 1), (21, 768, 0, 1), (21, 769, 0, 0), (21, 0, 0, 0),
         (21, -5, 0, 0), (15, 1, 0, 1), (15, 1024, 1, 1), (15, 1025, 0, 0), (20, 13, 0, 0), (22, 13, 0, 0), (16, 16, 0, 0),
         (64, 4, 0, 0), (128, 4, 0, 0), (21, 13, 2, 0), (15, 16, 2, 0), (21, 13, -1, 0), (21, 2 ** 40, 0, 0)]


@pytest.mark.parametrize('d,B,kind,want', TRUTH)
def test_supported_truth_table(lib, d, B, kind, want):
    assert lib.lib().mfg_pop_resident_supported(d, B, kind) == want


def test_host_restatement_agrees_with_the_library(lib):
    pytest.importorskip('torch')
    from discrete_mean_field_game_amd.population import resident_supported
    for d in (1, 14, 15, 16, 20, 21, 22, 40, 64):
        for B in (1, 2, 11, 12, 13, 16, 17, 767, 768, 769, 1023, 1024, 1025, 4096):
            assert resident_supported(d, B) == bool(lib.lib().mfg_pop_resident_supported(d, B, 0)), (d, B)
    assert lib.POP_RESIDENT_MAX_TILES == 64
    text = open(os.path.join(ROOT, 'include', 'mfg_hip.h')).read()
    assert re.search(r'#define\s+MFG_POP_RESIDENT_MAX_TILES\s+64\b', text)
    assert re.search(r'#define\s+MFG_POP_RESIDENT_EPISODES\s+64\b', text)


def test_rule_never_chooses_an_unsupported_shape(lib):
    pytest.importorskip('torch')
    from discrete_mean_field_game_amd.population import resident_rule
    for K in (1, 2, 16, 255, 256, 257, 512, 513, 4096, 65535):
        for d in (1, 15, 16, 20, 21, 40, 64):
            for B in (2, 12, 13, 16, 48, 96, 192, 256, 768, 769, 1024, 1025, 4096):
                r = resident_rule(K, d, B)
                assert r in (True, False)
                assert not r or lib.lib().mfg_pop_resident_supported(d, B, 0) == 1, (K, d, B)


def test_constructor_checks():
    pytest.importorskip('torch')
    from discrete_mean_field_game_amd.population import check_args, check_resident
    base = dict(K=4, d=21, batch=13, update_every='step', reward='mfg_ac2', precision='mixed', episode_steps=15)
    for resident in (None, True, False):
        check_args(resident=resident, **base)
    for kw in (dict(d=20), dict(batch=769), dict(update_every='rollout'), dict(d=15, batch=1025), dict(d=40)):
        args = dict(base, **kw)
        check_args(resident=None, **args)       # the rule falls back: only a forced resident path is refused
        check_args(resident=False, **args)
        with pytest.raises(ValueError):
            check_args(resident=True, **args)
    with pytest.raises(ValueError):
        check_resident('yes', 21, 13, 'step')
    check_resident(True, 15, 1024, 'step')


def test_train_call_checks():
    np = pytest.importorskip('numpy')
    pytest.importorskip('torch')
    from discrete_mean_field_game_amd.population import needs_control, stop_criteria_array, use_resident
    state = np.zeros(3, dtype=np.int32)
    assert not needs_control(stop_criteria_array(-1, 3), False, state)
    assert needs_control(stop_criteria_array(0.01, 3), False, state)
    assert needs_control(stop_criteria_array([-1, 0.0, -1], 3), False, state)
    assert needs_control(stop_criteria_array(-1, 3), True, state)
    assert needs_control(stop_criteria_array(-1, 3), False, np.array([0, 2, 0], dtype=np.int32))
    assert not needs_control(stop_criteria_array(-1, 3), False, np.array([0, 1, 0], dtype=np.int32))   # stopped, not failed
    # forced: runs resident whatever the rule says, refuses a controlled call
    assert use_resident(True, False, False) is True
    with pytest.raises(ValueError):
        use_resident(True, True, True)
    # the rule: followed, and silently off under a control block
    assert use_resident(None, True, False) is True
    assert use_resident(None, False, False) is False
    assert use_resident(None, True, True) is False
    for rule in (True, False):
        for control in (True, False):
            assert use_resident(False, rule, control) is False


def test_bound_with_the_per_step_parameter_list(lib):
    assert lib.SIGNATURES['mfg_train_episodes_pop_resident'] == lib.SIGNATURES['mfg_train_episodes_pop']
    assert lib.SIGNATURES['mfg_train_episodes_pop_resident'][1] is not lib.SIGNATURES['mfg_train_episodes_pop'][1]
    assert len(lib.SIGNATURES['mfg_pop_resident_supported'][1]) == 3
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'mfg_hip.h')).read(), flags=re.S)
    decl = {}
    for name in ('mfg_train_episodes_pop', 'mfg_train_episodes_pop_resident'):
        args = re.search(r'\b%s\s*\(([^;]*)\);' % name, text, flags=re.S).group(1)
        decl[name] = [re.sub(r'\s+', ' ', a).strip() for a in args.split(',')]
        assert getattr(lib.lib(), name) is not None
    assert decl['mfg_train_episodes_pop_resident'] == decl['mfg_train_episodes_pop']
    assert lib.lib().mfg_pop_resident_supported is not None


def test_abi_version_unchanged(lib):
    assert lib.lib().mfg_abi_version() == 18


def test_ops_wrapper_has_the_per_step_signature():
    pytest.importorskip('torch')
    import inspect
    from discrete_mean_field_game_amd import ops
    assert inspect.signature(ops.train_episodes_pop_resident) == inspect.signature(ops.train_episodes_pop)


def test_rule_follows_the_committed_measurement():
    """Every mixed-precision row of profiles/pop_resident_ab.txt: the rule chooses the resident path exactly where the
    table's verdict is `resident`."""
    pytest.importorskip('torch')
    from discrete_mean_field_game_amd.population import resident_rule
    rows = re.findall(r'^mixed d=\s*(\d+) K=\s*(\d+) Bk=\s*(\d+) .* (resident|per-step|tie)$',
                      open(os.path.join(ROOT, 'profiles', 'pop_resident_ab.txt')).read(), flags=re.M)
    assert len(rows) == 36
    for d, K, Bk, verdict in rows:
        assert resident_rule(int(K), int(d), int(Bk)) == (verdict == 'resident'), (d, K, Bk, verdict)
    # between the measured K from 512 learners on: a half-empty last round of 512 workgroups is not chosen at many tiles
    assert not resident_rule(513, 21, 768) and resident_rule(1024, 21, 768) and resident_rule(513, 21, 12)
    assert not resident_rule(15, 21, 12)       # below the smallest measured K
