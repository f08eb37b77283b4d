"""CPU checks of held-out validation inside a population training call (mfg_ctx_set_pop_validate): the validation block's
ctypes mirror has the C compiler's layout, the two functions are declared / bound / exported with the ABI number unchanged,
the workspace query behaves, Validation checks its arguments on the host and both train() methods take the keyword."""
import inspect
import os
import re

import pytest

np = pytest.importorskip('numpy')

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ['emp32', 'emp64', 'curve', 'checks', 'best_value', 'best_check', 'since_best', 'best_theta', 'best_w', 'workspace',
          'workspace_bytes', 'N', 'L', 'repeats', 'period', 'column', 'with_score', 'patience', 'max_checks', 'K', 'first_step']


@pytest.fixture(scope='module')
def lib():
    from discrete_mean_field_game_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib


def test_pop_validate_struct_layout_matches_the_header(lib, tmp_path):
    """mfg_pop_validate_t crosses the boundary by pointer: _lib.PopValidateStruct must have the C compiler's size and field
    offsets (a small C program prints them from include/mfg_hip.h)."""
    import ctypes as C
    import subprocess
    fields = [n for n, _ in lib.PopValidateStruct._fields_]
    assert fields == FIELDS
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "mfg_hip.h"\nint main(void){printf("%zu", '
           'sizeof(mfg_pop_validate_t));\n')
    for f in fields:
        src += 'printf(" %%zu", offsetof(mfg_pop_validate_t, %s));\n' % f
    src += 'return 0;}\n'
    c = tmp_path / 'layout.c'
    c.write_text(src)
    exe = str(tmp_path / 'layout')
    subprocess.run(['gcc', '-std=c99', '-I', os.path.join(ROOT, 'include'), str(c), '-o', exe], check=True)
    out = [int(x) for x in subprocess.run([exe], check=True, stdout=subprocess.PIPE).stdout.decode().split()]
    assert out[0] == C.sizeof(lib.PopValidateStruct)
    assert out[1:] == [getattr(lib.PopValidateStruct, f).offset for f in fields]


def test_pop_validate_declared_bound_and_exported(lib):
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'mfg_hip.h')).read(), flags=re.S)
    for name, nargs in (('mfg_ctx_set_pop_validate', 2), ('mfg_pop_validate_workspace_bytes', 6)):
        decl = re.search(r'\b%s\s*\(([^;]*)\);' % name, text, flags=re.S).group(1)
        assert len(decl.split(',')) == len(lib.SIGNATURES[name][1]) == nargs
        assert 'mfg_stream_t' not in decl            # host only: no stream, no row in the stream-order table
        assert getattr(lib.lib(), name) is not None
    assert lib.lib().mfg_abi_version() == 18
    assert lib.POP_VALIDATE_COLUMNS == 10 and re.search(r'MFG_POP_VALIDATE_COLUMNS\s+10', text)


def test_set_pop_validate_refuses_a_null_context(lib):
    """Checked before anything touches a device: no context, no block."""
    import ctypes as C
    blk = lib.PopValidateStruct(*([8] * 10), 1 << 20, 2, 4, 1, 1, 0, 0, 0, 1, 3, 0)
    assert lib.lib().mfg_ctx_set_pop_validate(None, C.byref(blk)) == -1
    assert b'context' in lib.lib().mfg_last_error()
    assert lib.lib().mfg_ctx_set_pop_validate(None, None) == -1


def test_pop_validate_workspace_bytes(lib):
    f = lib.lib().mfg_pop_validate_workspace_bytes
    ev = lib.lib().mfg_evaluate_pop_workspace_bytes
    for bad in ((0, 4, 21, 3, 1), (2, 0, 21, 3, 1), (2, 4, 0, 3, 1), (2, 4, 21, 0, 1), (2, 4, 21, 3, 0)):
        assert f(*bad, 0) == 0 and f(*bad, 1) == 0
    for N, Lr, d, K, R in ((2, 4, 21, 3, 3), (5, 16, 21, 16, 16), (1, 2, 15, 1, 1), (7, 16, 64, 5, 1024)):
        plain, score = f(N, Lr, d, K, R, 0), f(N, Lr, d, K, R, 1)
        assert plain >= ev(N, Lr, d, K, R, 0) > 0
        assert score > plain
        for s in (0, 1):
            assert f(N + 1, Lr, d, K, R, s) >= f(N, Lr, d, K, R, s)
            assert f(N, Lr, d, K + 1, R, s) >= f(N, Lr, d, K, R, s)
            assert f(N, Lr, d, K, R + 1, s) >= f(N, Lr, d, K, R, s)


def test_validation_checks_its_arguments_on_the_host():
    pytest.importorskip('torch')
    from discrete_mean_field_game_amd.population import VALIDATION_COLUMNS, Validation, validation_column
    assert VALIDATION_COLUMNS == ('mean_l1_final', 'std_l1_final', 'mean_l1_mean', 'std_l1_mean', 'mean_JSD_final',
                                  'std_JSD_final', 'mean_JSD_mean', 'std_JSD_mean', 'crps', 'energy')
    assert validation_column('JSD_mean') == 6 and validation_column('l1_final') == 0 and validation_column('std_l1_mean') == 3
    assert validation_column('crps') == 8 and validation_column('energy') == 9
    emp = np.random.RandomState(0).dirichlet(np.ones(21), size=(2, 4))
    v = Validation(emp=emp, period=2, repeats=3, metric='l1_final', patience=1)
    assert (v.period, v.repeats, v.column, v.patience, v.score) == (2, 3, 0, 1, False)
    assert Validation(emp=emp).column == 6 and Validation(emp=emp).rows(21).shape == (2, 4, 21)
    assert Validation(emp=emp, metric='crps', score=True).column == 8
    with pytest.raises(ValueError):
        Validation(emp=emp, period=0)
    with pytest.raises(ValueError):
        Validation(emp=emp, metric='accuracy')
    with pytest.raises(ValueError):
        Validation(emp=emp, metric='crps')
    with pytest.raises(ValueError):
        Validation(emp=emp, metric='energy', score=False)
    with pytest.raises(ValueError):
        Validation(emp=emp, patience=-1)
    with pytest.raises(ValueError):
        Validation(emp=emp, repeats=0)
    with pytest.raises(ValueError):
        Validation(emp=emp, indir='held_out')
    with pytest.raises(ValueError):
        Validation()
    with pytest.raises(ValueError):
        Validation(emp=emp[:, :1])
    with pytest.raises(ValueError):
        Validation(emp=emp).rows(15)


@pytest.mark.parametrize('cls', ['population.ActorCriticPopulation', 'irl_population.AC_IRLPopulation'])
def test_train_takes_validate_keyword_only(cls):
    pytest.importorskip('torch')
    import importlib
    mod, name = cls.split('.')
    klass = getattr(importlib.import_module('discrete_mean_field_game_amd.' + mod), name)
    par = inspect.signature(klass.train).parameters
    assert par['validate'].kind is inspect.Parameter.KEYWORD_ONLY and par['validate'].default is None
    assert callable(klass.restore_best)
