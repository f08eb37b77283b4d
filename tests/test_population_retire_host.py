"""CPU checks of retiring learners of a population (mfg_ctx_set_pop_control): the control block's ctypes mirror has the C
compiler's layout, the new call is declared / bound / exported with the ABI number unchanged, train()'s stop_criteria is
broadcast and validated before any call, and a population's activity mirror starts out all active."""
import inspect
import os
import re

import pytest

np = pytest.importorskip('numpy')

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def lib():
    from discrete_mean_field_game_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib


def test_pop_control_struct_layout_matches_the_header(lib, tmp_path):
    """mfg_pop_control_t crosses the boundary by pointer: _lib.PopControlStruct must have the C compiler's size and field
    offsets (a small C program prints them from include/mfg_hip.h)."""
    import ctypes as C
    import subprocess
    fields = [n for n, _ in lib.PopControlStruct._fields_]
    assert fields == ['state', 'status', 'theta_prev', 'episodes_run', 'stop_criteria', 'K']
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "mfg_hip.h"\nint main(void){printf("%zu", sizeof(mfg_pop_control_t));\n'
    for f in fields:
        src += 'printf(" %%zu", offsetof(mfg_pop_control_t, %s));\n' % f
    src += 'return 0;}\n'
    c = tmp_path / 'layout.c'
    c.write_text(src)
    exe = str(tmp_path / 'layout')
    subprocess.run(['gcc', '-std=c99', '-I', os.path.join(ROOT, 'include'), str(c), '-o', exe], check=True)
    out = [int(x) for x in subprocess.run([exe], check=True, stdout=subprocess.PIPE).stdout.decode().split()]
    assert out[0] == C.sizeof(lib.PopControlStruct)
    assert out[1:] == [getattr(lib.PopControlStruct, f).offset for f in fields]


def test_set_pop_control_declared_bound_and_exported(lib):
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'mfg_hip.h')).read(), flags=re.S)
    decl = re.search(r'\bmfg_ctx_set_pop_control\s*\(([^;]*)\);', text, flags=re.S).group(1)
    assert len(decl.split(',')) == len(lib.SIGNATURES['mfg_ctx_set_pop_control'][1]) == 2
    assert getattr(lib.lib(), 'mfg_ctx_set_pop_control') is not None
    assert lib.lib().mfg_abi_version() == 18
    assert lib.STATUS_MIXED_RANGE == 1 and lib.STATUS_POP_NONFINITE == 2
    assert re.search(r'MFG_STATUS_POP_NONFINITE\s*=\s*2', text)


def test_set_pop_control_refuses_a_null_context(lib):
    """Checked before anything touches a device: no context, no block."""
    import ctypes as C
    blk = lib.PopControlStruct(1, 1, 1, 1, 1, 3)
    assert lib.lib().mfg_ctx_set_pop_control(None, C.byref(blk)) != 0
    assert b'context' in lib.lib().mfg_last_error()


def test_stop_criteria_broadcast_and_validation():
    pytest.importorskip('torch')
    from discrete_mean_field_game_amd.population import stop_criteria_array
    assert np.array_equal(stop_criteria_array(-1, 3), [-1.0, -1.0, -1.0])
    assert np.array_equal(stop_criteria_array(0.01, 2), [0.01, 0.01])
    a = stop_criteria_array([0.5, -1, 1e-3], 3)
    assert a.dtype == np.float64 and np.array_equal(a, [0.5, -1.0, 1e-3])
    with pytest.raises(ValueError):
        stop_criteria_array([0.1, 0.2], 3)
    with pytest.raises(ValueError):
        stop_criteria_array([0.1, float('nan'), 0.2], 3)
    with pytest.raises(ValueError):
        stop_criteria_array(float('nan'), 3)


def test_learner_state_before_any_training():
    """The activity mirror a population starts with: every learner active, nothing run, no status bit; clear() revives failed
    learners only and refuses an index outside the population."""
    pytest.importorskip('torch')
    from discrete_mean_field_game_amd.population import ACTIVE, FAILED, STOPPED, LearnerActivity
    act = LearnerActivity(4)
    for a in (act.state, act.episodes, act.status):
        assert a.dtype == np.int32 and np.array_equal(a, [0, 0, 0, 0])
    assert act.healthy() == [0, 1, 2, 3]
    act.state[:] = [ACTIVE, FAILED, STOPPED, FAILED]
    act.status[:] = [0, 1, 0, 2]
    assert act.healthy() == [0, 2]
    act.clear(1)
    assert np.array_equal(act.state, [ACTIVE, ACTIVE, STOPPED, FAILED]) and np.array_equal(act.status, [0, 0, 0, 2])
    act.clear()
    assert np.array_equal(act.state, [ACTIVE, ACTIVE, STOPPED, ACTIVE]) and not act.status.any()
    with pytest.raises(IndexError):
        act.clear(4)


@pytest.mark.parametrize('cls', ['population.ActorCriticPopulation', 'irl_population.AC_IRLPopulation'])
def test_train_takes_the_keywords_with_todays_defaults(cls):
    pytest.importorskip('torch')
    import importlib
    mod, name = cls.split('.')
    klass = getattr(importlib.import_module('discrete_mean_field_game_amd.' + mod), name)
    par = inspect.signature(klass.train).parameters
    for key, default in (('stop_criteria', -1), ('isolate', False)):
        assert par[key].kind is inspect.Parameter.KEYWORD_ONLY and par[key].default == default
    for attr in ('learner_state', 'episodes_run', 'learner_status'):
        assert isinstance(getattr(klass, attr), property)
    assert 'k' in inspect.signature(klass.clear_status).parameters
