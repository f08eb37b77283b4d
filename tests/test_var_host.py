"""CPU: the VAR population call without a GPU -- the restatement itself (tests/var_ref.py), the cap on its own rounding error that
the GPU tolerances are built from, the descriptor structs against the C compiler, the two new symbols, the refusals of the
library and of the Python layer, and the cross-validation splits."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import var_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def lib():
    from discrete_mean_field_game_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib


# ---------------------------------------------------------------------------------------------------- the restatement
def test_regressor_layout_and_day_gather_on_a_hand_built_example():
    # 3 days of 2 hours, d = 2: value = 100 day + 10 hour + topic
    days = np.array([[[100 * D + 10 * h + j for j in range(2)] for h in range(2)] for D in range(3)], dtype=np.float64)
    Y = R.series(days, [2, 0])                        # day 2 then day 0: rows 200,201 | 210,211 | 0,1 | 10,11
    assert Y.tolist() == [[200, 201], [210, 211], [0, 1], [10, 11]]
    Z, X = R.design(Y, 2)
    # t = 2: [1, y_1, y_0]; t = 3: [1, y_2, y_1] -- lags run across the day boundary; regressor 1 + (l - 1) d + j
    assert Z.tolist() == [[1, 210, 211, 200, 201], [1, 0, 1, 210, 211]]
    assert X.tolist() == [[0, 1], [10, 11]]
    G, Cm = R.gram(Y, 2, 0.5)
    assert G[0, 0] == 2.5 and G[3, 1] == 200 * 210 + 210 * 0 and Cm[4, 1] == 201 * 1 + 211 * 11
    # forecast, origin 0 and 1, with coefficients that copy the row one back / two back
    B = np.zeros((5, 2))
    B[1, 0] = B[2, 1] = 1.0                           # y_t = y_{t-1}
    test = R.series(days, [1])
    assert R.forecast(Y, test, 2, B, 0, 2).tolist() == [[10, 11], [10, 11]]
    assert R.forecast(Y, test, 2, B, 1, 2).tolist() == [[100, 101], [100, 101]]
    B = np.zeros((5, 2))
    B[3, 0] = B[4, 1] = 1.0                           # y_t = y_{t-2}
    assert R.forecast(Y, test, 2, B, 0, 2).tolist() == [[0, 1], [10, 11]]
    assert R.forecast(Y, test, 2, B, 1, 2).tolist() == [[100, 101], [10, 11]]    # hour 1: two back of [.., 10 11, 100 101]


def test_jsd_is_the_oracles_and_leaves_its_inputs_alone():
    from oracle.mfg_oracle import JSD_synthetic
    rs = np.random.RandomState(0)
    P, Q = rs.dirichlet(np.ones(7), 5), rs.dirichlet(np.ones(7), 5)
    Q[2, 3], P[1, 0] = -0.25, 0.0
    P0, Q0 = P.copy(), Q.copy()
    assert np.allclose(R.jsd(P, Q), JSD_synthetic(P, Q), rtol=1e-13, atol=0)
    assert np.array_equal(P, P0) and np.array_equal(Q, Q0)
    per_day, met = R.metrics(Q[:4], P[:4], 2)
    assert per_day.shape == (2, 4) and met[0] == per_day[:, 0].mean() and met[7] == per_day[:, 3].std()


@pytest.mark.parametrize('case', [c for c in R.CASES if c[2] * R.HD - c[1] > 1 + c[1] * c[0]], ids=R.case_id)
def test_the_small_ridge_tends_to_the_minimum_norm_solution(case):
    """Overdetermined cases only: there the ridge forecast at lambda = 1e-8 lies within 1e-4 of the minimum-norm lstsq forecast
    (what statsmodels solves).  Underdetermined, the two differ by design and the recursion amplifies it."""
    days, tr, te = R.case_days(case)
    p = case[1]
    Y, X = R.series(days, tr), R.series(days, te)
    Z, T = R.design(Y, p)
    B_ls = np.linalg.lstsq(Z, T, rcond=1e-15)[0]
    diff = np.abs(R.forecast(Y, X, p, R.ridge_fit(Y, p, 1e-8), 0, R.HD) - R.forecast(Y, X, p, B_ls, 0, R.HD)).max()
    print('ridge vs lstsq %s: %.2e' % (R.case_id(case), diff))
    assert diff <= 1e-4


@pytest.mark.parametrize('case', R.CASES, ids=R.case_id)
def test_the_restatements_own_rounding_error_is_small(case):
    """The GPU test allows 64 x this gap: it must not be able to grow large enough to hide a failure."""
    for lam in R.RIDGES:
        for origin in (0, 1):
            assert R.longdouble_gap(case, lam, origin) <= 1e-9


def test_the_longdouble_fit_agrees_with_the_fp64_fit():
    days, tr, _ = R.case_days((15, 2, 8))
    Y = R.series(days, tr)
    a, b = R.ridge_fit(Y, 2, 1e-2), R.ridge_fit(Y, 2, 1e-2, np.longdouble)
    G, Cm = R.gram(Y, 2, 1e-2, np.longdouble)
    assert b.dtype == np.longdouble and np.abs(a - b).max() <= 1e-9 * np.abs(a).max()
    assert float(np.abs(G @ b - Cm).max()) <= 1e-17 * float(np.abs(G).max() * np.abs(b).max()) * G.shape[0]


# ---------------------------------------------------------------------------------------------------- the C boundary
@pytest.mark.parametrize('ctype,name', [('mfg_var_model_t', 'VarModelStruct'), ('mfg_var_fit_t', 'VarFitStruct')])
def test_struct_layouts_match_the_header(lib, tmp_path, ctype, name):
    st = getattr(lib, name)
    fields = [n for n, _ in st._fields_]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "mfg_hip.h"\nint main(void){printf("%%zu", sizeof(%s));\n' % ctype
    for f in fields:
        src += 'printf(" %%zu", offsetof(%s, %s));\n' % (ctype, f)
    src += 'return 0;}\n'
    c = tmp_path / 'layout.c'
    c.write_text(src)
    exe = str(tmp_path / 'layout')
    subprocess.run(['gcc', '-std=c99', '-I', os.path.join(ROOT, 'include'), str(c), '-o', exe], check=True)
    out = [int(x) for x in subprocess.run([exe], check=True, stdout=subprocess.PIPE).stdout.decode().split()]
    assert out[0] == C.sizeof(st)
    assert out[1:] == [getattr(st, f).offset for f in fields]
    text = open(os.path.join(ROOT, 'include', 'mfg_hip.h')).read()
    body = re.search(r'typedef struct \w+ \{([^}]*)\} %s;' % ctype, text).group(1)
    assert len(re.findall(r'[\w\]]\s*[,;]', body)) == len(fields)          # (no member of the header is missing from the mirror)


def test_the_new_symbols_are_declared_bound_and_exported(lib):
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'mfg_hip.h')).read(), flags=re.S)
    h = lib.lib()
    for name in ('mfg_var_fit_pop', 'mfg_var_fit_workspace_bytes'):
        assert re.search(r'\b%s\s*\(' % name, text) and name in lib.SIGNATURES and getattr(h, name) is not None
    assert 'mfg_stream_t stream;' in text and not re.search(r'mfg_var_fit_pop\s*\([^)]*mfg_stream_t', text)
    assert int(re.search(r'#define MFG_VAR_MAX_REGRESSORS (\d+)', text).group(1)) == lib.VAR_MAX_REGRESSORS == 512
    assert h.mfg_abi_version() == 18


def _table(lib, rows):
    t = (lib.VarModelStruct * len(rows))()
    for x, (lag, origin, ntr, nte, ridge) in zip(t, rows):
        x.lag, x.origin, x.n_train, x.n_test, x.ridge = lag, origin, ntr, nte, ridge
    return t


def test_workspace_layout(lib):
    h = lib.lib()
    t = _table(lib, [(1, 0, 2, 0, 1.0), (20, 0, 13, 3, 1.0), (2, 1, 8, 3, 1.0)])
    total = h.mfg_var_fit_workspace_bytes(3, t, 15)
    up = lambda m: (64 + (m + 15) * m * 8 + 255) // 256 * 256
    assert [x.ws_offset for x in t] == [0, up(16), up(16) + up(301)] and total == up(16) + up(301) + up(31)
    assert h.mfg_var_fit_workspace_bytes(0, t, 15) == 0 and h.mfg_var_fit_workspace_bytes(3, None, 15) == 0
    assert h.mfg_var_fit_workspace_bytes(3, t, 65) == 0 and h.mfg_var_fit_workspace_bytes(3, t, 26) == 0      # 1 + 20 x 26 > 512
    t[0].lag = 0
    assert h.mfg_var_fit_workspace_bytes(3, t, 15) == 0


def _fit(lib, rows, d=3, Hd=16, D=8, M=None, S_max=64, strides=(4, 4), ws_bytes=None, **nulls):
    """A descriptor whose device pointers are dummies: every refusal below happens before anything is launched or read."""
    h = lib.lib()
    t = _table(lib, rows)
    total = h.mfg_var_fit_workspace_bytes(len(rows), t, d)
    f = lib.VarFitStruct()
    for name in ('days', 'models', 'train_idx', 'test_idx', 'coef', 'sse', 'insample', 'future', 'per_day', 'metrics', 'status',
                 'workspace'):
        setattr(f, name, None if nulls.get(name) else 4096)
    f.models_host = C.addressof(t)
    f.workspace_bytes = total if ws_bytes is None else ws_bytes
    f.D, f.Hd, f.d, f.K, f.train_stride, f.test_stride = D, Hd, d, len(rows), strides[0], strides[1]
    f.M, f.S_max = (max([1 + r[0] * d for r in rows] + [1]) if M is None else M), S_max
    return f, t


GOOD = (2, 0, 3, 1, 1e-2)


@pytest.mark.parametrize('why,kw', [
    ('d = 0', dict(d=0)), ('d = 65', dict(d=65, rows=[(1, 0, 3, 1, 1e-2)])), ('Hd = 0', dict(Hd=0)), ('Hd = 65', dict(Hd=65)),
    ('D = 0', dict(D=0)), ('lag 0', dict(rows=[(0, 0, 3, 1, 1e-2)])), ('m = 514', dict(rows=[(171, 0, 64, 1, 1e-2)])),
    ('no training day', dict(rows=[(2, 0, 0, 1, 1e-2)])), ('65 training days', dict(rows=[(2, 0, 65, 1, 1e-2)], strides=(65, 4))),
    ('more training days than the table', dict(rows=[(2, 0, 5, 1, 1e-2)])), ('65 test days', dict(rows=[(2, 0, 3, 65, 1e-2)], strides=(4, 65), S_max=2000)),
    ('test days < 0', dict(rows=[(2, 0, 3, -1, 1e-2)])), ('n = 0', dict(rows=[(48, 0, 3, 1, 1e-2)])),
    ('rolling lag > T + 1', dict(rows=[(18, 1, 1, 1, 1e-2)])), ('origin 2', dict(rows=[(2, 2, 3, 1, 1e-2)])),
    ('ridge 0', dict(rows=[(2, 0, 3, 1, 0.0)])), ('ridge < 0', dict(rows=[(2, 0, 3, 1, -1.0)])),
    ('ridge inf', dict(rows=[(2, 0, 3, 1, float('inf'))])), ('ridge nan', dict(rows=[(2, 0, 3, 1, float('nan'))])),
    ('M too small', dict(M=6)), ('S_max too small', dict(S_max=15)), ('null days', dict(days=True)), ('null coef', dict(coef=True)),
    ('null status', dict(status=True)), ('null device table', dict(models=True)), ('null workspace', dict(workspace=True)),
    ('second model bad', dict(rows=[GOOD, (2, 0, 3, 1, 0.0)]))])
def test_the_library_refuses_with_einval_before_it_launches(lib, why, kw):
    kw = dict(kw)
    f, t = _fit(lib, kw.pop('rows', [GOOD]), **kw)
    assert lib.lib().mfg_var_fit_pop(C.byref(f)) == -1, why          # MFG_EINVAL


def test_the_library_checks_the_layout_and_the_workspace_size(lib):
    h = lib.lib()
    assert h.mfg_var_fit_pop(None) == -1
    f, t = _fit(lib, [GOOD, GOOD], ws_bytes=512)
    assert h.mfg_var_fit_pop(C.byref(f)) == -4                       # MFG_EWORKSPACE
    f, t = _fit(lib, [GOOD, GOOD])
    t[1].ws_offset += 256
    assert h.mfg_var_fit_pop(C.byref(f)) == -1 and b'ws_offset' in h.mfg_last_error()
    f, t = _fit(lib, [GOOD])
    f.workspace = 4100
    assert h.mfg_var_fit_pop(C.byref(f)) == -1 and b'aligned' in h.mfg_last_error()


# ---------------------------------------------------------------------------------------------------- the Python layer
def test_ops_argument_rules():
    from discrete_mean_field_game_amd import ops
    ok = dict(lags=[2], ridges=[1e-2], train_n=[3], test_n=[1], origins=[0])
    assert ops.check_var_fit_args((8, 16, 3), **ok) == (1, 8, 16, 3, 7, 16)
    assert ops.check_var_fit_args((8, 16, 3), [1, 15], [1.0, 2.0], [1, 1], [0, 4], [0, 1]) == (2, 8, 16, 3, 46, 64)
    for shape, bad in (((8, 16), {}), ((8, 16, 65), {}), ((8, 0, 3), {}), ((8, 65, 3), {}), ((0, 16, 3), {}),
                       ((8, 16, 3), dict(lags=[0])), ((8, 16, 3), dict(lags=[171], train_n=[64])), ((8, 16, 3), dict(lags=[48])),
                       ((8, 16, 3), dict(lags=[18], train_n=[1], origins=[1])), ((8, 16, 3), dict(origins=[2])),
                       ((8, 16, 3), dict(origins=['rolling'])), ((8, 16, 3), dict(train_n=[0])), ((8, 16, 3), dict(train_n=[65])),
                       ((8, 16, 3), dict(test_n=[65])), ((8, 16, 3), dict(test_n=[-1])), ((8, 16, 3), dict(ridges=[0.0])),
                       ((8, 16, 3), dict(ridges=[float('nan')])), ((8, 16, 3), dict(ridges=[float('inf')])),
                       ((8, 16, 3), dict(lags=[])), ((8, 16, 3), dict(lags=[1, 2]))):
        a = dict(ok)
        a.update(bad)
        with pytest.raises(ValueError):
            ops.check_var_fit_args(shape, **a)
    with pytest.raises(ValueError):
        ops.check_var_fit_args((8, 16, 3), train_stride=2, **ok)
    with pytest.raises(ValueError):
        ops.check_var_fit_args((8, 16, 3), test_stride=0, **ok)
    # (n >= 1 already keeps every lag below the rolling origin's own limit, lag <= T + 1: the last fitted lag is T - 1)
    assert ops.check_var_fit_args((8, 16, 3), [15], [1.0], [1], [1], [1])[4] == 46


def test_fit_population_argument_rules():
    from discrete_mean_field_game_amd import var as V
    days = R.synthetic_days(6, 16, 3, 1)
    out = V.check_population_args(days, [1, 2], 1e-2, [0, 1, 2], [[3], [4, 5]], 'rolling')
    assert out[6] == (2, 6, 16, 3, 7, 32) and out[2].tolist() == [1e-2, 1e-2] and out[5].tolist() == [1, 1]
    assert [t.tolist() for t in out[3]] == [[0, 1, 2]] * 2 and [t.tolist() for t in out[4]] == [[3], [4, 5]]
    assert V.check_population_args(days, [1], [1.0], [[5, 0]], None, ['train_end'])[6] == (1, 6, 16, 3, 4, 0)
    for args in ((days[0], [1], 1.0, [0], None, 'rolling'), (days, [], 1.0, [0], None, 'rolling'), (days, [1], 1.0, [6], None, 'rolling'),
                 (days, [1], 1.0, [-1], None, 'rolling'), (days, [1], 1.0, [], None, 'rolling'), (days, [1, 2], 1.0, [[0]], None, 'rolling'),
                 (days, [1], [1.0, 2.0], [0], None, 'rolling'), (days, [1], 1.0, [0], [7], 'rolling'), (days, [1], 1.0, [0], None, 'aic'),
                 (days, [1, 1], 1.0, [0], None, ['rolling']), (days, [1], 0.0, [0], None, 'rolling'), (days, [16], 1.0, [0], None, 'train_end')):
        with pytest.raises(ValueError):
            V.check_population_args(*args)
    assert V._hours(208) == 52 and V._hours(208, 48) == 16 and V._hours(17 * 16, 16) == 16
    with pytest.raises(ValueError):
        V._hours(67 * 67)


def test_the_var_class_checks_its_arguments_and_restates_jsd():
    from discrete_mean_field_game_amd import var as V
    v = V.var(d=3)
    with pytest.raises(ValueError):
        v.train(2, np.zeros((32, 3)), ridge=0.0)
    P, Q = np.array([0.5, 0.5, 0.0]), np.array([0.2, -0.1, 0.9])
    P0, Q0 = P.copy(), Q.copy()
    assert abs(v.JSD(P, Q) - float(R.jsd(P, Q))) <= 1e-15 and np.array_equal(P, P0) and np.array_equal(Q, Q0)
    assert not hasattr(v, 'check_stationarity') and not hasattr(v, 'plot')


def test_cross_validation_draws_the_references_splits():
    """var.py:126-127 on a seeded global state: `repetitions` draws per lag, lag-major, np.random.choice without replacement."""
    from discrete_mean_field_game_amd import var as V
    np.random.seed(5)
    want = []
    for _ in range(3 * 2):
        selected = np.random.choice(range(6), 6 - 2, replace=False)
        want.append((selected.tolist(), [x for x in range(6) if x not in selected]))
    np.random.seed(5)
    got = V.var.splits(6, 2, 6)
    assert [(s.tolist(), r) for s, r in got] == want
    again = V.var.splits(6, 2, 6, np.random.RandomState(5))
    assert [(s.tolist(), r) for s, r in again] == want
    assert all(len(r) == 2 and sorted(s.tolist() + r) == list(range(6)) for s, r in got)
