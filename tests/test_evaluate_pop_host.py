"""CPU checks of the population evaluation (mfg_evaluate_pop, population.gridsearch / evaluate): the entry is declared, bound and
refuses bad arguments before anything is launched; the Python side refuses unusable test directories; the grid order and the
reference's list_tuples scan (mfg_ac2.py:673-689) on a fixed metric table."""
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


def test_declared_bound_and_exported(lib):
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'mfg_hip.h')).read(), flags=re.S)
    for name in ('mfg_evaluate_pop', 'mfg_evaluate_pop_workspace_bytes'):
        decl = re.search(r'\b%s\s*\(([^;]*)\);' % name, text, flags=re.S).group(1)
        assert len(decl.split(',')) == len(lib.SIGNATURES[name][1]), name
        assert getattr(lib.lib(), name) is not None
    assert lib.lib().mfg_abi_version() == 18


def test_workspace_bytes(lib):
    h = lib.lib()
    N, L, d, K, R = 5, 16, 21, 3, 2
    idx = K * 256                                 # one 256-byte index table per learner (N R = 10 entries)
    per_traj = K * N * R * 4 * 8
    assert h.mfg_evaluate_pop_workspace_bytes(N, L, d, K, R, 1) == idx + per_traj
    assert h.mfg_evaluate_pop_workspace_bytes(N, L, d, K, R, 0) == idx + per_traj + K * N * R * L * d * 4
    assert h.mfg_evaluate_pop_workspace_bytes(0, L, d, K, R, 0) == 0
    assert h.mfg_evaluate_pop_workspace_bytes(N, L, d, K, 0, 0) == 0


def _call(lib, **kw):
    """mfg_evaluate_pop with fake device addresses and NO workspace: every call must be refused before any launch."""
    a = dict(emp32=8, emp64=8, N=5, L=16, d=21, K=3, theta=8, shift=8, alpha=8, seed=8, first_step=0, repeats=1, precision=1,
             metrics=8, traj=None, ws=8, ws_bytes=0)
    a.update(kw)
    return lib.lib().mfg_evaluate_pop(a['emp32'], a['emp64'], a['N'], a['L'], a['d'], a['K'], a['theta'], a['shift'], a['alpha'],
                                      a['seed'], a['first_step'], a['repeats'], a['precision'], a['metrics'], a['traj'], a['ws'],
                                      a['ws_bytes'], None)


@pytest.mark.parametrize('kw,code', [(dict(K=0), EINVAL), (dict(K=65536), EINVAL), (dict(d=65), EUNSUPPORTED), (dict(d=0), EINVAL),
                                     (dict(L=1), EINVAL), (dict(N=0), EINVAL), (dict(repeats=0), EINVAL), (dict(emp32=None), EINVAL),
                                     (dict(seed=None), EINVAL), (dict(metrics=None), EINVAL), (dict(ws=None), EINVAL),
                                     (dict(precision=7), EINVAL), (dict(first_step=0xFFFFFFFF), EINVAL), (dict(), EWORKSPACE)])
def test_entry_refuses_before_launch(lib, kw, code):
    assert _call(lib, **kw) == code
    assert lib.lib().mfg_last_error()


def _files(tmp_path, monkeypatch, n, rows, d=21):
    monkeypatch.chdir(tmp_path)
    os.makedirs('test_normalized_round2')
    rs = np.random.RandomState(0)
    for j in range(n):
        np.savetxt('test_normalized_round2/day%d.csv' % j, rs.dirichlet(np.ones(d), size=rows), fmt='%.3e', delimiter=' ')


@pytest.mark.parametrize('kw', [dict(d=65), dict(repeats=0), dict(episode_length=1), dict(precision='half')])
def test_gridsearch_refuses_arguments(tmp_path, monkeypatch, kw):
    pytest.importorskip('torch')
    from discrete_mean_field_game_amd import population
    _files(tmp_path, monkeypatch, 2, 16)
    with pytest.raises(ValueError):
        population.gridsearch([8.0], [0.5], [1e4], 'test_normalized_round2', 'out.csv', **kw)
    assert not os.path.exists('out.csv')


def test_short_files_and_empty_directory(tmp_path, monkeypatch):
    pytest.importorskip('torch')
    from discrete_mean_field_game_amd import population
    _files(tmp_path, monkeypatch, 3, 12)
    with pytest.raises(ValueError, match='rows'):
        population.load_empirical('test_normalized_round2', 21, 16)
    assert population.load_empirical('test_normalized_round2', 21, 12).shape == (3, 12, 21)
    os.makedirs('empty')
    with pytest.raises(ValueError, match='no test files'):
        population.gridsearch([8.0], [0.5], [1e4], 'empty', 'out.csv')


def test_load_empirical_reads_like_actor_critic(tmp_path, monkeypatch):
    pytest.importorskip('torch')
    from discrete_mean_field_game_amd import population
    _files(tmp_path, monkeypatch, 4, 20, d=23)
    got = population.load_empirical('test_normalized_round2', 21, 16)
    names = os.listdir(os.getcwd() + '/test_normalized_round2')
    want = np.array([np.loadtxt('test_normalized_round2/' + f, delimiter=' ')[:, 0:21] for f in names])[:, :16]
    assert np.array_equal(got, want)


def test_grid_order_is_theta_major():
    pytest.importorskip('torch')
    from discrete_mean_field_game_amd import population
    pts = population.grid_points([1.0, 2.0], [0.1, 0.2, 0.3], [10.0, 20.0])
    assert len(pts) == 12
    assert pts[:3] == [(1.0, 0.1, 10.0), (1.0, 0.1, 20.0), (1.0, 0.2, 10.0)]
    assert pts[-1] == (2.0, 0.3, 20.0)
    assert population.grid_points([], [0.1], [1.0]) == []


def test_best_points_scan():
    pytest.importorskip('torch')
    from discrete_mean_field_game_amd import population
    pts = [(1.0, 0.1, 10.0), (1.0, 0.2, 10.0), (2.0, 0.1, 10.0), (2.0, 0.2, 10.0)]
    table = np.array([[0.5, 0, 0.3, 0, 0.02, 0, 0.04, 0],
                      [0.4, 0, 0.3, 0, 0.03, 0, 0.05, 0],
                      [0.6, 0, 0.2, 0, 0.02, 0, 0.06, 0],
                      [0.4, 0, 0.9, 0, 0.01, 0, 0.07, 0]])
    best = population.best_points(pts, table)
    assert best[0] == [0.4, 2.0, 0.2, 10.0]      # a tie goes to the later point (the reference's <=)
    assert best[1] == [0.2, 2.0, 0.1, 10.0]
    assert best[2] == [0.01, 2.0, 0.2, 10.0]
    assert best[3] == [0.04, 1.0, 0.1, 10.0]
    assert population.best_points([], []) == [[100, 0, 0, 0]] * 4
    # metrics above the reference's start value of 100 never replace it
    assert population.best_points(pts[:1], np.full((1, 8), 200.0))[0] == [100, 0, 0, 0]


def test_csv_rows_use_the_evaluate_format(tmp_path):
    pytest.importorskip('torch')
    from discrete_mean_field_game_amd import population
    from discrete_mean_field_game_amd.mfg_ac2 import actor_critic
    out = str(tmp_path / 'o.csv')
    population.write_eval_rows(out, 1, [(8.5, 0.25, 12000.0)], np.arange(8.0)[None] * 0.001)
    lines = open(out).read().split('\n')
    assert lines[0] + '\n' == actor_critic._EVAL_HEADER
    assert lines[1] == '8.500000,0.250000,12000.000000,0.000e+00,1.000e-03,2.000e-03,3.000e-03,4.000e-03,5.000e-03,6.000e-03,7.000e-03'
