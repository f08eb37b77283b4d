"""CPU checks of the ensemble forecast (mfg_forecast_pop, ops.forecast_pop, population.forecast / forecast_ranks,
actor_critic.forecast): the entry is declared, bound and refuses bad arguments before anything is launched; the rank rule
floor(p (R - 1)); the Python-side argument rules that need no GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED, EWORKSPACE = -1, -3, -4


@pytest.fixture(scope='module')
def lib():
    from discrete_mean_field_game_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib


def test_forecast_ranks_pins():
    pytest.importorskip('torch')
    from discrete_mean_field_game_amd.population import forecast_ranks
    for R in (1, 2, 5, 256, 1024):
        assert forecast_ranks([0.0], R) == [0]
        assert forecast_ranks([1.0], R) == [R - 1]
    assert forecast_ranks([0.5], 5) == [2]
    assert forecast_ranks([0.5], 4) == [1]
    assert forecast_ranks((0.05, 0.5, 0.95), 256) == [12, 127, 242]
    assert forecast_ranks([0.9, 0.1, 0.9], 11) == [9, 1, 9]          # unsorted, repeated: kept as given
    assert forecast_ranks([], 7) == []
    assert forecast_ranks([0.0, 0.25, 0.5, 0.75, 1.0], 5) == [0, 1, 2, 3, 4]
    for bad in ([-0.01], [1.0001], [float('nan')], [0.5, 2.0]):
        with pytest.raises(ValueError):
            forecast_ranks(bad, 16)
    with pytest.raises(ValueError):
        forecast_ranks(np.linspace(0, 1, 9), 16)                     # more than MFG_FORECAST_MAX_RANKS
    with pytest.raises(ValueError):
        forecast_ranks([0.5], 0)


def test_declared_bound_and_exported(lib):
    raw = open(os.path.join(ROOT, 'include', 'mfg_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', raw, flags=re.S)
    for name in ('mfg_forecast_pop', 'mfg_forecast_pop_workspace_bytes'):
        decl = re.search(r'\b%s\s*\(([^;]*)\);' % name, text, flags=re.S).group(1)
        assert len(decl.split(',')) == len(lib.SIGNATURES[name][1]), name
        assert getattr(lib.lib(), name) is not None
    macros = dict(re.findall(r'#define (MFG_FORECAST_MAX_[A-Z]+) (\d+)', text))
    assert int(macros['MFG_FORECAST_MAX_RANKS']) == lib.FORECAST_MAX_RANKS == 8
    assert int(macros['MFG_FORECAST_MAX_REPEATS']) == lib.FORECAST_MAX_REPEATS >= 1024
    assert lib.lib().mfg_abi_version() == 18
    # the header comment cites the reference lines the call serves
    comment = raw[raw.index('Ensemble forecast'):raw.index('#define MFG_FORECAST_MAX_RANKS')]
    for cite in ('mfg_ac2.py:566-592', 'mfg_ac2.py:763', 'ac_irl.py:1663', 'var.py:294-327', 'THREE launches'):
        assert cite in comment, cite


def test_workspace_bytes(lib):
    h = lib.lib()
    N, H, d, K = 5, 6, 21, 3
    prev = 0
    for R in (1, 2, 3, 33, 64, 65, 257, 1024):
        kept = h.mfg_forecast_pop_workspace_bytes(N, H, d, K, R, 1)
        own = h.mfg_forecast_pop_workspace_bytes(N, H, d, K, R, 0)
        assert kept > prev                                           # monotone in R
        assert own == kept + K * N * R * H * d * 4                   # the trajectories live in the workspace when not given
        assert kept >= K * H * N * R * 2 * 8                         # the per-member (L1, JSD) of the curves
        prev = kept
    assert h.mfg_forecast_pop_workspace_bytes(0, H, d, K, 1, 0) == 0
    assert h.mfg_forecast_pop_workspace_bytes(N, H, d, K, 0, 0) == 0


def _call(lib, **kw):
    """mfg_forecast_pop with fake device addresses and NO workspace: every call must be refused before any launch."""
    a = dict(start=8, N=5, H=6, d=21, K=3, theta=8, shift=8, alpha=8, seed=8, first_step=0, repeats=4, precision=1,
             ranks=(0, 3, 1, 1), emp32=8, emp64=8, mean=8, std=8, quant=8, curves=8, traj=None, ws=8, ws_bytes=0)
    a.update(kw)
    Q = a['Q'] if 'Q' in a else len(a['ranks'])
    rk = (C.c_int32 * 16)(*a['ranks']) if a['ranks'] is not None else None
    return lib.lib().mfg_forecast_pop(a['start'], a['N'], a['H'], a['d'], a['K'], a['theta'], a['shift'], a['alpha'], a['seed'],
                                      a['first_step'], a['repeats'], a['precision'], rk, Q, a['emp32'], a['emp64'], a['mean'],
                                      a['std'], a['quant'], a['curves'], a['traj'], a['ws'], a['ws_bytes'], None)


@pytest.mark.parametrize('kw,code', [
    (dict(K=0), EINVAL), (dict(K=65536), EINVAL), (dict(d=65), EUNSUPPORTED), (dict(d=0), EINVAL), (dict(H=1), EINVAL),
    (dict(N=0), EINVAL), (dict(repeats=0), EINVAL), (dict(start=None), EINVAL), (dict(seed=None), EINVAL),
    (dict(mean=None), EINVAL), (dict(std=None), EINVAL), (dict(ws=None), EINVAL), (dict(precision=7), EINVAL),
    (dict(first_step=0xFFFFFFFF), EINVAL),
    (dict(ranks=(0, 4)), EINVAL),                                    # rank = R
    (dict(ranks=(-1,)), EINVAL),
    (dict(ranks=tuple(range(4)) * 2 + (0,)), EINVAL),                # Q = 9
    (dict(Q=-1), EINVAL),
    (dict(quant=None), EINVAL), (dict(ranks=None, Q=2), EINVAL),
    (dict(emp32=None), EINVAL), (dict(emp64=None), EINVAL),
    (dict(curves=None), EINVAL),                                     # emp given, no curves
    (dict(emp32=None, emp64=None), EINVAL),                          # curves given, no emp
    (dict(repeats=1025, ranks=(0, 1024)), EUNSUPPORTED),             # above MFG_FORECAST_MAX_REPEATS
    (dict(), EWORKSPACE),
    (dict(ranks=(), quant=None), EWORKSPACE),                        # Q = 0 without quant is legal
    (dict(emp32=None, emp64=None, curves=None), EWORKSPACE),         # no held-out rows is legal
    (dict(repeats=1024, ranks=(1023,)), EWORKSPACE),                 # the cap itself is served
])
def test_entry_refuses_before_launch(lib, kw, code):
    assert _call(lib, **kw) == code
    assert lib.lib().mfg_last_error()


def test_short_workspace_by_one_byte(lib):
    need = lib.lib().mfg_forecast_pop_workspace_bytes(5, 6, 21, 3, 4, 0)
    assert _call(lib, ws_bytes=need - 1) == EWORKSPACE
    assert str(need) in lib.lib().mfg_last_error().decode()


def test_ops_argument_rules():
    pytest.importorskip('torch')
    from discrete_mean_field_game_amd import ops
    ok = dict(start_shape=(5, 21), horizon=6, repeats=4, ranks=(0, 3, 1, 1), precision='mixed')
    assert ops.check_forecast_args(**ok) == (5, 21, 6, 4, [0, 3, 1, 1])
    assert ops.check_forecast_args(**dict(ok, emp32_shape=(5, 6, 21), emp64_shape=(5, 6, 21)))[0] == 5
    for bad in (dict(start_shape=(21,)), dict(start_shape=(5, 6, 21)), dict(horizon=1), dict(repeats=0), dict(repeats=1025),
                dict(ranks=(4,)), dict(ranks=(-1,)), dict(ranks=tuple(range(4)) * 2 + (0,)), dict(precision='half'),
                dict(emp32_shape=(5, 6, 21)), dict(emp64_shape=(5, 6, 21)),
                dict(emp32_shape=(5, 7, 21), emp64_shape=(5, 7, 21)), dict(emp32_shape=(4, 6, 21), emp64_shape=(4, 6, 21))):
        with pytest.raises(ValueError):
            ops.check_forecast_args(**dict(ok, **bad))


def test_forecast_refuses_tensors_off_the_device():
    torch = pytest.importorskip('torch')
    from discrete_mean_field_game_amd import ops
    z = torch.zeros(1, dtype=torch.float64)
    with pytest.raises(ValueError):
        ops.forecast_pop(torch.zeros(5, 21), z, z, z, torch.zeros(1, dtype=torch.int64), 6)


def test_population_forecast_argument_rules():
    pytest.importorskip('torch')
    from discrete_mean_field_game_amd import population
    pi0 = np.full((2, 21), 1.0 / 21)
    for kw in (dict(d=65), dict(d=21, repeats=0), dict(d=21, repeats=1025), dict(d=21, probs=(1.5,)), dict(d=21, precision='half'),
               dict(d=21, probs=np.linspace(0, 1, 9)), dict(d=21, emp=np.zeros((3, 6, 21))), dict(d=21, emp=np.zeros((2, 5, 21)))):
        with pytest.raises(ValueError):
            population.forecast([8.0], 0.5, 1e4, pi0, 6, **kw)
    with pytest.raises(ValueError):
        population.forecast([8.0], 0.5, 1e4, pi0, 1, d=21)
    with pytest.raises(ValueError):
        population.forecast([8.0], 0.5, 1e4, None, 6, d=21)          # neither start rows nor held-out rows
    with pytest.raises(ValueError):
        population.forecast([8.0, 9.0], [0.5, 0.4, 0.3], 1e4, pi0, 6, d=21)


def test_forecast_inputs_start_rows_from_emp():
    pytest.importorskip('torch')
    from discrete_mean_field_game_amd.population import _forecast_inputs
    emp = np.random.RandomState(0).dirichlet(np.ones(23), size=(3, 8))
    start, e = _forecast_inputs(None, emp, 21, 6)
    assert e.shape == (3, 6, 21) and np.array_equal(e, emp[:, :6, :21]) and np.array_equal(start, emp[:, 0, :21])
    start, e = _forecast_inputs(emp[0, 0], None, 21, 6)
    assert e is None and start.shape == (1, 21)


def test_numpy_rng_is_refused():
    pytest.importorskip('torch')
    from discrete_mean_field_game_amd.mfg_ac2 import check_forecast_rng
    check_forecast_rng('philox')
    with pytest.raises(ValueError, match='philox'):
        check_forecast_rng('numpy')
