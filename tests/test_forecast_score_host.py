"""CPU checks of the forecast scores (mfg_forecast_score, ops.forecast_score, population.forecast_score / gridsearch_score /
pit / covered, actor_critic.forecast_score): the entry is declared, bound and refuses bad arguments before anything is launched;
the NumPy restatement the GPU tests compare with (tests/forecast_score_ref.py) holds its own identities; the host helpers and
the argument rules that need no GPU."""
import os
import re

import numpy as np
import pytest

import forecast_score_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED, EWORKSPACE = -1, -3, -4
NAMES = ('mfg_forecast_score', 'mfg_forecast_score_workspace_bytes')


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
    assert int(re.search(r'#define MFG_FORECAST_SCORE_TILE (\d+)', text).group(1)) == lib.FORECAST_SCORE_TILE == ref.TILE
    assert lib.lib().mfg_abi_version() == 18
    # the header comment cites what the entry goes beyond
    comment = raw[raw.index('Proper scores of an ensemble forecast'):raw.index('#define MFG_FORECAST_SCORE_TILE')]
    for cite in ('mfg_ac2.py:595-670', 'var.py:330-416', 'mfg_forecast_pop', 'TWO launches', 'Gneiting'):
        assert cite in comment, cite


def test_the_unit_is_built_with_default_flags():
    mk = open(os.path.join(ROOT, 'discrete_mean_field_game_amd', 'csrc', 'Makefile')).read()
    units = re.search(r'^UNITS := (.*)$', mk, flags=re.M).group(1).split()
    assert 'mfg_forecast_score' in units
    assert 'mfg_forecast_score.h' in re.search(r'^HDRS := (.*)$', mk, flags=re.M).group(1).split()
    for var in ('NOSLP_UNITS', 'ILP_UNITS'):
        assert 'mfg_forecast_score' not in re.search(r'^%s :?= (.*)$' % var, mk, flags=re.M).group(1).split()


def test_workspace_bytes(lib):
    h = lib.lib()
    N, H, d, K = 5, 6, 21, 3
    prev = 0
    for R in (1, 2, 3, 33, 64, 65, 257, 1024):
        need = h.mfg_forecast_score_workspace_bytes(N, H, d, K, R)
        assert need >= prev and need >= K * N * H * 8                # monotone in R; the per-cell CRPS sums
        prev = need
    for empty in ((0, H, d, K, 4), (N, 0, d, K, 4), (N, H, 0, K, 4), (N, H, d, 0, 4), (N, H, d, K, 0)):
        assert h.mfg_forecast_score_workspace_bytes(*empty) == 0


def _call(lib, **kw):
    """mfg_forecast_score with fake device addresses and NO workspace: every call must be refused before any launch."""
    a = dict(traj=8, N=5, H=6, d=21, K=3, repeats=4, emp32=8, emp64=8, crps=8, less=8, equal=8, energy=8, summary=8, ws=8,
             ws_bytes=0)
    a.update(kw)
    return lib.lib().mfg_forecast_score(a['traj'], a['N'], a['H'], a['d'], a['K'], a['repeats'], a['emp32'], a['emp64'], a['crps'],
                                        a['less'], a['equal'], a['energy'], a['summary'], a['ws'], a['ws_bytes'], None)


@pytest.mark.parametrize('kw,code', [
    (dict(K=0), EINVAL), (dict(K=65536), EINVAL), (dict(d=0), EINVAL), (dict(d=65), EUNSUPPORTED), (dict(H=1), EINVAL),
    (dict(N=0), EINVAL), (dict(repeats=0), EINVAL), (dict(N=1 << 30), EINVAL),     # N H beyond the grid
    (dict(traj=None), EINVAL), (dict(emp32=None), EINVAL), (dict(emp64=None), EINVAL), (dict(crps=None), EINVAL),
    (dict(less=None), EINVAL), (dict(equal=None), EINVAL), (dict(summary=None), EINVAL), (dict(ws=None), EINVAL),
    (dict(repeats=1025), EUNSUPPORTED),                              # above MFG_FORECAST_MAX_REPEATS
    (dict(), EWORKSPACE),
    (dict(energy=None), EWORKSPACE),                                 # no energy score is legal
    (dict(repeats=1024), EWORKSPACE),                                # the cap itself is served
    (dict(d=64, repeats=1024), EWORKSPACE),
])
def test_entry_refuses_before_launch(lib, kw, code):
    assert _call(lib, **kw) == code
    assert lib.lib().mfg_last_error()


def test_short_workspace_by_one_byte(lib):
    need = lib.lib().mfg_forecast_score_workspace_bytes(5, 6, 21, 3, 4)
    assert need > 0
    assert _call(lib, ws_bytes=need - 1) == EWORKSPACE
    assert str(need) in lib.lib().mfg_last_error().decode()


# ---------------------------------------------------------------------------------------------- the restatement itself
def test_restatement_single_member():
    rs = np.random.RandomState(0)
    x, y = rs.dirichlet(np.ones(7), size=1), rs.dirichlet(np.ones(7))
    for c in range(7):
        assert ref.crps_column(x[:, c], y[c])[0] == abs(x[0, c] - y[c])
    assert ref.energy_cell(x, y)[0] == np.sqrt(((x[0] - y) ** 2).sum())


def test_restatement_all_members_equal_the_observation():
    y = np.random.RandomState(1).dirichlet(np.ones(21))
    x = np.tile(y, (33, 1))
    assert ref.energy_cell(x, y) == (0.0, 0.0)
    for c in range(21):
        assert ref.crps_column(x[:, c], y[c]) == (0.0, 0.0)
    assert ref.sorted_pair_sum(x[:, 0].astype(np.float32).astype(np.float64))[0] == 0.0   # exact for fp32 values: products and sums


def test_restatement_hand_example():
    # members 1 and 4, observation 2: E|X - y| = (1 + 2) / 2, E|X - X'| = (0 + 3 + 3 + 0) / 4: 1.5 - 0.75
    assert ref.crps_column(np.array([1.0, 4.0]), 2.0) == (0.75, 2.25)
    # members (0, 0) and (3, 4), observation (0, 0): (0 + 5) / 2 - (5 + 5) / 8
    assert ref.energy_cell(np.array([[0.0, 0.0], [3.0, 4.0]]), np.zeros(2)) == (1.25, 3.75)


@pytest.mark.parametrize('R', [2, 3, 64, 257, 1024])
def test_restatement_sorted_identity(R):
    x = np.random.RandomState(R).dirichlet(np.ones(21), size=R)[:, 3].astype(np.float32).astype(np.float64)
    x[R // 2] = x[0]                                                 # a tie
    double = np.abs(x[:, None] - x[None, :]).sum()
    got, terms = ref.sorted_pair_sum(x)
    assert abs(got - double) <= (ref.pairwise_depth(R) + ref.pairwise_depth(R * R) + 2) * ref.U * terms
    assert terms >= double


def test_restatement_energy_is_crps_in_one_dimension():
    rs = np.random.RandomState(5)
    x, y = rs.rand(65, 1), rs.rand(1)
    e, te = ref.energy_cell(x, y)
    c, tc = ref.crps_column(x[:, 0], y[0])
    assert abs(e - c) <= 40 * ref.U * tc and abs(te - tc) <= 40 * ref.U * tc


def test_restatement_score_shapes_and_chains():
    rs = np.random.RandomState(2)
    K, N, H, d, R = 2, 3, 2, 7, 5
    traj = rs.dirichlet(np.ones(d), size=(K, N * R, H)).astype(np.float32)
    emp64 = rs.dirichlet(np.ones(d), size=(N, H))
    out = ref.score(traj, emp64.astype(np.float32), emp64, N, R)
    assert out['crps'].shape == (K, N, H, d) and out['energy'].shape == (K, N, H) and out['summary'].shape == (K, H, 2)
    assert np.all(out['less'] + out['equal'] <= R) and np.all(out['crps'] >= 0) and np.all(out['energy'] >= 0)
    x = ref.members(traj[1], N, R)[2, :, 1, :].astype(np.float64)    # member r of start row n is row r N + n
    assert np.array_equal(x, traj[1, 2::N, 1, :].astype(np.float64))
    assert out['energy'][1, 2, 1] == ref.energy_cell(x, emp64[2, 1])[0]
    assert np.isnan(ref.score(traj, emp64.astype(np.float32), emp64, N, R, want_energy=False)['summary'][..., 1]).all()
    assert ref.crps_chain(1) == 7 and ref.crps_chain(65) == 8 and ref.crps_chain(1024) == 22
    assert ref.energy_chain(64) == 26 and ref.energy_chain(65) == 58 and ref.energy_chain(1024) == 136 * 16 + 10
    assert [ref.pairwise_depth(n) for n in (1, 8, 9, 128, 256, 1 << 20)] == [1, 8, 8, 19, 20, 32]


# -------------------------------------------------------------------------------------------------- host helpers, rules
def test_pit_and_covered():
    from discrete_mean_field_game_amd.population import covered, pit
    # members 1 2 2 3 5 (R = 5).  y = 2: less 1, equal 2; y = 0: below all; y = 9: above all; y = 4: between
    less, equal = np.array([1, 0, 5, 4]), np.array([2, 0, 0, 0])
    assert np.array_equal(pit(less, equal, 5), [0.4, 0.0, 1.0, 0.8])
    # the band of the order statistics 1 .. 3 is [2, 3]: holds y = 2 (a tie with x_(1)), not 0, 9 or 4
    assert covered(less, equal, 1, 3).tolist() == [True, False, False, False]
    # the whole range 0 .. 4 = [1, 5] holds 2 and 4
    assert covered(less, equal, 0, 4).tolist() == [True, False, False, True]
    # y = 3 = x_(3) alone: less 3, equal 1: inside 3 .. 3 and 1 .. 3, outside 0 .. 2
    assert covered(3, 1, 3, 3) and covered(3, 1, 1, 3) and not covered(3, 1, 0, 2)
    # against a sort: every y on a grid, every band
    x = np.array([1.0, 2.0, 2.0, 3.0, 5.0], dtype=np.float32)
    for y in np.arange(0.0, 6.5, 0.5, dtype=np.float32):
        lt, eq = int((x < y).sum()), int((x == y).sum())
        for lo in range(5):
            for hi in range(lo, 5):
                assert bool(covered(lt, eq, lo, hi)) == bool(x[lo] <= y <= x[hi]), (y, lo, hi)
    with pytest.raises(ValueError):
        pit(less, equal, 0)


def test_ops_argument_rules():
    pytest.importorskip('torch')
    from discrete_mean_field_game_amd import ops
    ok = dict(traj_shape=(3, 20, 6, 21), emp32_shape=(5, 6, 21), emp64_shape=(5, 6, 21), N=5, repeats=4)
    assert ops.check_forecast_score_args(**ok) == (3, 5, 6, 21, 4)
    for bad in (dict(repeats=0), dict(repeats=1025, traj_shape=(3, 5125, 6, 21)), dict(repeats=5), dict(N=0), dict(N=4),
                dict(traj_shape=(20, 6, 21)), dict(traj_shape=(0, 20, 6, 21)), dict(traj_shape=(3, 20, 1, 21), emp32_shape=(5, 1, 21),
                                                                                    emp64_shape=(5, 1, 21)),
                dict(traj_shape=(3, 20, 6, 65), emp32_shape=(5, 6, 65), emp64_shape=(5, 6, 65)), dict(emp32_shape=(5, 6, 20)),
                dict(emp64_shape=(4, 6, 21))):
        with pytest.raises(ValueError):
            ops.check_forecast_score_args(**dict(ok, **bad))


def test_forecast_score_refuses_tensors_off_the_device(lib):
    torch = pytest.importorskip('torch')
    from discrete_mean_field_game_amd import ops
    with pytest.raises(ValueError):
        ops.forecast_score(torch.zeros(1, 8, 6, 21), torch.zeros(2, 6, 21), torch.zeros(2, 6, 21, dtype=torch.float64), 2, 4)


def test_population_argument_rules(lib, tmp_path, monkeypatch):
    pytest.importorskip('torch')
    from discrete_mean_field_game_amd import population
    emp = np.random.RandomState(0).dirichlet(np.ones(21), size=(2, 6))
    for kw in (dict(d=21, repeats=0), dict(d=21, repeats=1025), dict(d=65), dict(d=21, precision='f32'), dict(d=21, horizon=1),
               dict(d=21, horizon=7), dict(d=21, pi0=np.ones((3, 21)) / 21), dict(d=21, budget=1000)):
        with pytest.raises(ValueError):
            population.forecast_score([8.0], 0.5, 1e4, emp, **kw)
    with pytest.raises(ValueError):
        population.forecast_score([8.0], 0.5, 1e4, None, d=21)       # nothing to score against
    with pytest.raises(ValueError):
        population.forecast_score([8.0, 9.0], [0.5, 0.4, 0.3], 1e4, emp, d=21)
    with pytest.raises(ValueError):
        population.forecast_score([], 0.5, 1e4, emp, d=21)
    # one policy's bytes: at least its members
    assert population.forecast_score_bytes(2, 6, 21, 256) >= 2 * 256 * 6 * 21 * 4
    # the grid search: rules ahead of the files, an empty grid launches nothing and writes nothing
    monkeypatch.chdir(tmp_path)
    os.makedirs('test_dir')
    np.savetxt('test_dir/day0.csv', emp[0], fmt='%.3e', delimiter=' ')
    for kw in (dict(repeats=0), dict(repeats=1025), dict(precision='f32'), dict(d=65), dict(episode_length=1), dict(episode_length=7)):
        with pytest.raises(ValueError):
            population.gridsearch_score([8.0], [0.5], [1e4], 'test_dir', 'out.csv', **dict(dict(d=21, episode_length=6), **kw))
    assert population.gridsearch_score([], [0.5], [1e4], 'test_dir', 'out.csv', d=21, episode_length=6) == [[float('inf'), 0, 0, 0]] * 4
    assert not os.path.exists('out.csv')


def test_score_columns_and_last_minimum():
    from discrete_mean_field_game_amd.population import best_score_points, score_columns
    s = np.zeros((2, 4, 2))
    s[0, :, 0], s[0, :, 1] = [0.0, 1.0, 2.0, 6.0], [0.0, 3.0, 3.0, 3.0]
    s[1, :, 0], s[1, :, 1] = [0.0, 3.0, 3.0, 3.0], [0.0, 4.0, 4.0, np.nan]
    t = score_columns(s)
    assert t[0].tolist() == [3.0, 6.0, 3.0, 3.0] and t[1, :2].tolist() == [3.0, 3.0] and np.isnan(t[1, 2:]).all()
    pts = [(8.0, 0.5, 1e4), (9.0, 0.4, 2e4)]
    best = best_score_points(pts, t)
    assert best[0] == [3.0, 9.0, 0.4, 2e4]                           # a tie: the last minimum in grid order
    assert best[1] == [3.0, 9.0, 0.4, 2e4] and best[2] == [3.0, 8.0, 0.5, 1e4] and best[3] == [3.0, 8.0, 0.5, 1e4]   # NaN never wins


def test_class_methods_exist_and_refuse_numpy_rng():
    pytest.importorskip('torch')
    from discrete_mean_field_game_amd import ac_irl, mfg_ac2, mfg_synthetic, population
    from discrete_mean_field_game_amd.irl_population import AC_IRLPopulation
    assert population.ActorCriticPopulation.forecast_score is AC_IRLPopulation.forecast_score is population._Population.forecast_score
    assert ac_irl.AC_IRL.forecast_score is mfg_ac2.actor_critic.forecast_score is mfg_synthetic.actor_critic.forecast_score
    for name in ('ForecastScore', 'forecast_score', 'gridsearch_score', 'pit', 'covered', 'forecast', 'gridsearch', 'Forecast'):
        assert hasattr(population, name), name
    fs = population.ForecastScore(np.zeros((2, 1, 2, 3)), np.zeros((2, 1, 2, 3), np.int32), np.ones((2, 1, 2, 3), np.int32), None,
                                  np.zeros((2, 2, 2)), 4)
    one = fs.learner(1)
    assert one.crps.shape == (1, 2, 3) and one.energy is None and one.repeats == 4 and one.summary.shape == (2, 2)
