"""CPU checks of the backward-equation check of K policies (mfg_consistency_given / mfg_consistency_pop, ops.consistency_*,
population.consistency, ActorCriticPopulation.evaluate_synthetic(_JSD), mfg_synthetic.sweep): the entries are declared, bound
and refuse bad arguments before anything is launched; the workspace sizes; the chunking under the byte budget; the sweep's
point order and CSV lines; the Python-side argument rules that need no GPU."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED, EWORKSPACE = -1, -3, -4
NAMES = ('mfg_consistency_given', 'mfg_consistency_given_workspace_bytes', 'mfg_consistency_pop',
         'mfg_consistency_pop_workspace_bytes')


@pytest.fixture(scope='module')
def lib():
    from discrete_mean_field_game_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib


def test_declared_bound_and_exported(lib):
    raw = open(os.path.join(ROOT, 'include', 'mfg_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', raw, flags=re.S)
    for name in NAMES:
        decl = re.search(r'\b%s\s*\(([^;]*)\);' % name, text, flags=re.S).group(1)
        assert len(decl.split(',')) == len(lib.SIGNATURES[name][1]), name
        assert getattr(lib.lib(), name) is not None
    assert lib.lib().mfg_abi_version() == 18
    # the header comment cites the reference lines the calls replace
    comment = raw[raw.index('Backward-equation check of K groups'):raw.index('size_t mfg_consistency_given_workspace_bytes')]
    for cite in ('mfg_synthetic.py:741-899', ':902-925', ':768-774', ':776-790', ':858-880', ':800-801', 'mfg_ac2.py:566-592',
                 'TWO launches', 'THREE launches'):
        assert cite in comment, cite


def test_workspace_bytes(lib):
    h = lib.lib()
    N, H, d = 5, 16, 21
    full = lambda K, R, **kw: h.mfg_consistency_pop_workspace_bytes(N, H, d, K, R, kw.get('steps', 0), kw.get('actions', 0),
                                                                    kw.get('traj', 0))
    prev = 0
    for K in (1, 2, 3, 200, 65535):
        b = full(K, 2)
        assert b > prev                                              # monotone in K
        assert b <= K * full(1, 2)                                   # what consistency_chunks relies on
        prev = b
    prev = 0
    for R in (1, 2, 3, 33, 64, 65, 257):
        b = full(3, R)
        assert b > prev                                              # monotone in R
        acts = 3 * N * R * (H - 1) * d * d * 4
        assert full(3, R, actions=1) == b - acts                     # the actions live in the workspace when not given
        assert full(3, R, steps=1) == b - 3 * N * R * (H - 1) * 2 * 8
        assert full(3, R, traj=1) < b
        assert full(3, R, steps=1, actions=1, traj=1) >= 3 * N * R * 4   # the start-index tables stay
        prev = b
    for bad in ((0, H, d, 3, 1), (N, 1, d, 3, 1), (N, H, 0, 3, 1), (N, H, d, 0, 1), (N, H, d, 3, 0)):
        assert h.mfg_consistency_pop_workspace_bytes(*bad, 0, 0, 0) == 0
    assert h.mfg_consistency_given_workspace_bytes(3, 7, 15, 0) == 3 * 7 * 15 * 2 * 8
    assert h.mfg_consistency_given_workspace_bytes(3, 7, 15, 1) == 0
    assert h.mfg_consistency_given_workspace_bytes(0, 7, 15, 0) == 0


def _given(lib, **kw):
    """mfg_consistency_given with fake device addresses and NO workspace: every call must be refused before any launch."""
    a = dict(P=8, K=3, M=7, T=3, d=21, metrics=8, steps=None, V=8, ws=8, ws_bytes=0)
    a.update(kw)
    return lib.lib().mfg_consistency_given(a['P'], a['K'], a['M'], a['T'], a['d'], a['metrics'], a['steps'], a['V'], a['ws'],
                                           a['ws_bytes'], None)


def _pop(lib, **kw):
    """mfg_consistency_pop with fake device addresses and NO workspace."""
    a = dict(start=8, N=5, H=6, d=21, K=3, theta=8, shift=8, alpha=8, seed=8, first_step=0, repeats=4, precision=1, metrics=8,
             steps=8, V=None, actions=None, traj=None, ws=8, ws_bytes=0)
    a.update(kw)
    return lib.lib().mfg_consistency_pop(a['start'], a['N'], a['H'], a['d'], a['K'], a['theta'], a['shift'], a['alpha'], a['seed'],
                                         a['first_step'], a['repeats'], a['precision'], a['metrics'], a['steps'], a['V'],
                                         a['actions'], a['traj'], a['ws'], a['ws_bytes'], None)


@pytest.mark.parametrize('kw,code', [
    (dict(K=0), EINVAL), (dict(K=65536), EINVAL), (dict(d=65), EUNSUPPORTED), (dict(d=0), EINVAL), (dict(T=0), EINVAL),
    (dict(M=0), EINVAL), (dict(P=None), EINVAL), (dict(metrics=None), EINVAL), (dict(ws=None), EINVAL),
    (dict(), EWORKSPACE), (dict(V=None), EWORKSPACE), (dict(d=64), EWORKSPACE),
])
def test_given_refuses_before_launch(lib, kw, code):
    assert _given(lib, **kw) == code
    assert lib.lib().mfg_last_error()


@pytest.mark.parametrize('kw,code', [
    (dict(K=0), EINVAL), (dict(K=65536), EINVAL), (dict(d=65), EUNSUPPORTED), (dict(d=0), EINVAL), (dict(H=1), EINVAL),
    (dict(N=0), EINVAL), (dict(repeats=0), EINVAL), (dict(start=None), EINVAL), (dict(theta=None), EINVAL),
    (dict(shift=None), EINVAL), (dict(alpha=None), EINVAL), (dict(seed=None), EINVAL), (dict(metrics=None), EINVAL),
    (dict(ws=None), EINVAL), (dict(precision=7), EINVAL), (dict(first_step=0xFFFFFFFF), EINVAL),
    (dict(), EWORKSPACE), (dict(steps=None), EWORKSPACE), (dict(actions=8, traj=8, V=8), EWORKSPACE),
    (dict(first_step=0xFFFFFFFF - 5), EWORKSPACE),                   # the last step that does not wrap
])
def test_pop_refuses_before_launch(lib, kw, code):
    assert _pop(lib, **kw) == code
    assert lib.lib().mfg_last_error()


def test_short_workspace_by_one_byte(lib):
    need = lib.lib().mfg_consistency_pop_workspace_bytes(5, 6, 21, 3, 4, 1, 0, 0)
    assert _pop(lib, ws_bytes=need - 1) == EWORKSPACE
    assert str(need) in lib.lib().mfg_last_error().decode()
    need = lib.lib().mfg_consistency_given_workspace_bytes(3, 7, 3, 0)
    assert _given(lib, ws_bytes=need - 1) == EWORKSPACE
    assert str(need) in lib.lib().mfg_last_error().decode()


def test_check_consistency_args():
    pytest.importorskip('torch')
    from discrete_mean_field_game_amd import ops
    ok = dict(start_shape=(5, 21), hours=16, repeats=4, precision='mixed', K=3, first_step=37)
    assert ops.check_consistency_args(**ok) == (5, 21, 16, 4)
    assert ops.check_consistency_args((1, 64), 2, 1, 'f64') == (1, 64, 2, 1)
    for bad in (dict(start_shape=(21,)), dict(start_shape=(5, 6, 21)), dict(start_shape=(0, 21)), dict(start_shape=(5, 65)),
                dict(start_shape=(5, 0)), dict(hours=1), dict(repeats=0), dict(precision='half'), dict(K=0), dict(K=65536),
                dict(first_step=-1), dict(first_step=0xFFFFFFFF - 14)):
        with pytest.raises(ValueError):
            ops.check_consistency_args(**dict(ok, **bad))


def test_consistency_pop_refuses_tensors_off_the_device():
    torch = pytest.importorskip('torch')
    from discrete_mean_field_game_amd import ops
    z = torch.zeros(1, dtype=torch.float64)
    with pytest.raises(ValueError):
        ops.consistency_pop(torch.zeros(5, 21), z, z, z, torch.zeros(1, dtype=torch.int64), 16)
    with pytest.raises(ValueError):
        ops.consistency_given(torch.zeros(1, 2, 3, 5, 5))


def test_chunks_cover_every_policy_once_within_the_budget(lib):
    pytest.importorskip('torch')
    from discrete_mean_field_game_amd import ops, population
    assert population.CONSISTENCY_BUDGET >= 1 << 20
    for K, per, budget in ((1, 10, 10), (7, 10, 35), (7, 10, 70), (7, 10, 1000), (200, 729400, 1 << 30), (1000, 3, 10),
                           (70000, 1, 1 << 30)):
        chunks = population.consistency_chunks(K, per, budget)
        flat = [k for c0, n in chunks for k in range(c0, c0 + n)]
        assert flat == list(range(K))                                # every policy exactly once, in order
        assert all(1 <= n <= lib.POP_MAX_K and n * per <= budget for _, n in chunks)
    # the real sizes: a chunk's workspace as the library counts it stays within the budget
    per = ops.consistency_pop_workspace_bytes(26, 16, 21, 1, 3)
    budget = 10 * per + 5
    for c0, n in population.consistency_chunks(64, per, budget):
        assert ops.consistency_pop_workspace_bytes(26, 16, 21, n, 3) <= budget
    assert population.consistency_chunks(200, ops.consistency_pop_workspace_bytes(26, 16, 21, 1, 1)) == [(0, 200)]
    with pytest.raises(ValueError):
        population.consistency_chunks(3, 11, 10)                     # one policy alone exceeds the budget
    with pytest.raises(ValueError):
        population.consistency_chunks(0, 1, 10)


def test_population_consistency_argument_rules():
    pytest.importorskip('torch')
    from discrete_mean_field_game_amd import population
    pi0 = np.full((2, 21), 1.0 / 21)
    for kw in (dict(d=65), dict(d=21, repeats=0), dict(d=21, hours=1), dict(d=21, precision='half'), dict(d=22),
               dict(d=21, first_step=-1)):
        with pytest.raises(ValueError):
            population.consistency([2.0], 0.0, 1e4, pi0, **kw)
    with pytest.raises(ValueError):
        population.consistency([2.0], 0.0, 1e4, None, d=21)
    with pytest.raises(ValueError):
        population.consistency([], 0.0, 1e4, pi0, d=21)
    with pytest.raises(ValueError):
        population.consistency([2.0, 3.0], [0.0, 0.1, 0.2], 1e4, pi0, d=21)


def test_sweep_order_and_csv_lines(tmp_path):
    pytest.importorskip('torch')
    from discrete_mean_field_game_amd import mfg_synthetic as S
    points = S.sweep_points(np.arange(0, 0.04, 0.02), np.arange(0, 0.15, 0.05))
    assert points == [(0.0, 0.0), (0.0, 0.05), (0.0, 0.1), (0.02, 0.0), (0.02, 0.05), (0.02, 0.1)]   # shift outermost
    assert len(S.sweep_points(np.arange(0, 0.04, 0.02), np.arange(0, 5.0, 0.05))) == 200               # the reference's sweep
    theta_final = np.array([0.1234, 1.0005, 2.25, 3.0, 4.4444, 5.55551])
    mean = np.array([0.25, 0.3333333, np.nan, 1e-4, 12.3456, 0.5])
    std = np.array([0.01, 0.02, np.nan, 0.04, 0.05, 0.06])
    table = S.sweep_table(points, theta_final, mean, std, [False, False, True, False, False, False])
    assert table.shape == (6, 5) and table[2, 3] == table[2, 4] == 900.0 and not np.isnan(table).any()
    out = str(tmp_path / 'synthetic.csv')
    S.write_sweep_rows(out, table)
    lines = open(out).read().split('\n')
    assert lines == ['Shift,theta_initial,theta_final,diff_mean,diff_std',
                     '0.000,0.000,0.123,0.250,0.010',
                     '0.000,0.050,1.000,0.333,0.020',
                     '0.000,0.100,2.250,900.000,900.000',
                     '0.020,0.000,3.000,0.000,0.040',
                     '0.020,0.050,4.444,12.346,0.050',
                     '0.020,0.100,5.556,0.500,0.060', '']
    S.write_sweep_rows(out, table[:1])                               # appends, header included, as the reference's __main__
    assert open(out).read().split('\n')[7:] == ['Shift,theta_initial,theta_final,diff_mean,diff_std',
                                                '0.000,0.000,0.123,0.250,0.010', '']


def test_sweep_start_table_resolution(tmp_path, monkeypatch):
    pytest.importorskip('torch')
    from discrete_mean_field_game_amd import mfg_synthetic as S
    from discrete_mean_field_game_amd import population
    rs = np.random.RandomState(3)
    given = rs.dirichlet(np.ones(23), size=5)
    assert np.array_equal(S.resolve_start_table(21, given), given[:, :21])
    files = rs.dirichlet(np.ones(23), size=3)
    os.makedirs(tmp_path / 'train_normalized')
    for n, row in enumerate(files):
        with open(tmp_path / 'train_normalized' / ('trend_distribution_day%d_reordered.csv' % (n + 1)), 'w') as f:
            f.write(' '.join('%.17g' % v for v in row) + '\n' + ' '.join('0' for _ in row) + '\n')
    assert np.array_equal(S.resolve_start_table(21, None, str(tmp_path / 'train_normalized')), files[:, :21])
    monkeypatch.chdir(tmp_path)
    assert np.array_equal(S.resolve_start_table(21), files[:, :21])              # cwd/train_normalized
    assert np.array_equal(S.resolve_start_table(21, given), given[:, :21])       # pi0 goes first
    os.makedirs(tmp_path / 'empty')
    monkeypatch.chdir(tmp_path / 'empty')
    assert np.array_equal(S.resolve_start_table(21), population.resolve_start_table(21))   # the synthetic table


def test_value_errors_without_a_gpu():
    pytest.importorskip('torch')
    from discrete_mean_field_game_amd import mfg_synthetic as S
    from discrete_mean_field_game_amd import population
    assert population.check_synthetic_eval('synthetic', 26, 1, 26, 1) == (1, 26, 1)
    assert population.check_synthetic_eval('synthetic', 4, 2, 2, 3) == (2, 2, 3)
    for bad in (('mfg_ac2', 26, 1, 26, 1), ('synthetic', 25, 1, 26, 1), ('synthetic', 26, 0, 26, 1), ('synthetic', 26, 5, 4, 1),
                ('synthetic', 26, 1, 26, 0)):
        with pytest.raises(ValueError):
            population.check_synthetic_eval(*bad)
    # the population methods check before they touch the device: stand-ins that hold only what the check reads
    pop = object.__new__(population.ActorCriticPopulation)
    pop.reward, pop.mat_pi0 = 'mfg_ac2', np.zeros((26, 21))
    for method in (pop.evaluate_synthetic, pop.evaluate_synthetic_JSD):
        with pytest.raises(ValueError, match='synthetic'):
            method(1, 26)
    pop.reward, pop.mat_pi0 = 'synthetic', np.zeros((4, 21))
    for method in (pop.evaluate_synthetic, pop.evaluate_synthetic_JSD):
        with pytest.raises(ValueError, match='days'):
            method(1, 26)
        with pytest.raises(ValueError, match='days'):
            method(0, 2)
        with pytest.raises(ValueError, match='repeats'):
            method(1, 4, repeats=0)
    # sweep: the day range against the resolved table, the metric, an empty grid -- all before a population is built
    pi0 = np.full((4, 21), 1.0 / 21)
    with pytest.raises(ValueError, match='days'):
        S.sweep([0.0], [1.0], batch=16, pi0=pi0)                     # the default days 1 .. 26 of a 4-row table
    with pytest.raises(ValueError, match='days'):
        S.sweep([0.0], [1.0], batch=16, pi0=pi0, day_first=3, day_last=2)
    with pytest.raises(ValueError, match='metric'):
        S.sweep([0.0], [1.0], batch=16, pi0=pi0, day_last=4, metric='kl')
    with pytest.raises(ValueError):
        S.sweep([], [1.0], batch=16, pi0=pi0, day_last=4)
    with pytest.raises(ValueError):
        S.check_sweep_args('jsd', 4, 1, 4, 0)
