"""GPU checks of the forecast scores (mfg_forecast_score): CRPS, the rank counts and the energy score of given members against
the NumPy restatement of the definitions (tests/forecast_score_ref.py: the double sums, not the kernel's sorted form) within a
bound derived from the inputs; the repeats cap; K-independence and determinism; a non-finite member; the population and class
forms against ops.forecast_score on population.forecast's members; the grid search; refusals."""
import functools
import os

import numpy as np
import pytest

import forecast_score_ref as ref

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

EINVAL, EUNSUPPORTED, EWORKSPACE = -1, -3, -4
KEYS = ('crps', 'less', 'equal', 'energy', 'summary')


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.fail('-m gpu tests need a GPU')
    from discrete_mean_field_game_amd import ops
    ops.init()
    return torch.device('cuda', 0)


def _dims(R):
    """(K, N, H) of a given-members case: K <= 3, N <= 5, H <= 6, fewer cells where the restatement's R^2 d work grows."""
    return (3, 5, 6) if R <= 3 else (2, 3, 3) if R <= 65 else (2, 2, 2)


@functools.lru_cache(maxsize=None)
def _given(d, R, K, N, H, with_ref=True):
    """Seeded fp32 Dirichlet members [K, N R, H, d] and held-out rows, with a duplicated member, a member equal to the fp32
    observation in two columns, and one cell (k, n, l) = (0, 0, H - 1) whose members all equal an fp32-representable
    observation; the restatement on them (computed once, never changed)."""
    rs = np.random.RandomState(1000 * d + R)
    traj = rs.dirichlet(np.ones(d), size=(K, N * R, H)).astype(np.float32)
    emp64 = rs.dirichlet(np.ones(d), size=(N, H))
    emp64[0, H - 1] = emp64[0, H - 1].astype(np.float32).astype(np.float64)
    emp32 = emp64.astype(np.float32)
    if R >= 2:
        traj[:, N] = traj[:, 0]                                      # members 0 and 1 of start row 0
    for c in (0, d // 2):
        traj[:, (R - 1) * N + N - 1, :, c] = emp32[N - 1, :, c]      # the last member of the last start row
    traj[0, 0::N, H - 1, :] = emp32[0, H - 1]
    res = dict(traj=traj, emp32=emp32, emp64=emp64)
    if with_ref:
        res.update(ref=ref.score(traj, emp32, emp64, N, R))
    for v in (traj, emp32, emp64):
        v.setflags(write=False)
    return res


def _run(dev, traj, emp32, emp64, N, R, want_energy=True):
    from discrete_mean_field_game_amd import ops
    t = lambda a: torch.as_tensor(np.array(a), device=dev)     # (a copy: the shared inputs are read-only)
    out = ops.forecast_score(t(traj), t(emp32), t(emp64), N, R, want_energy=want_energy)
    torch.cuda.synchronize()
    return out


def _host(out):
    return {k: None if v is None else v.cpu().numpy() for k, v in out.items()}


def _check_against_ref(got, want, R, label):
    """Counts equal; crps, energy and summary within the restatement's derived bounds (each figure printed before it is asserted)."""
    assert np.array_equal(got['less'], want['less']) and np.array_equal(got['equal'], want['equal'])
    assert got['less'].dtype == np.int32 and got['equal'].dtype == np.int32
    for key in ('crps', 'energy', 'summary'):
        err, bound = np.abs(got[key] - want[key]), want[key + '_bound']
        print('%s %s: max error %.3e, bound there %.3e, largest error / bound %.3f'
              % (label, key, err.max(), bound.reshape(-1)[err.argmax()], (err / np.maximum(bound, 1e-300)).max()))
        assert np.all(np.isfinite(got[key]))
        assert np.all(err <= bound), key


# ---------------------------------------------------------------------------------------------------- 1. given members
@pytest.mark.parametrize('d', [7, 15, 21, 64])
@pytest.mark.parametrize('R', [1, 2, 3, 33, ref.TILE - 1, ref.TILE, ref.TILE + 1, 2 * ref.TILE, 130, 257])
def test_given_members_match_the_restatement(dev, d, R):
    from discrete_mean_field_game_amd import _lib
    assert _lib.FORECAST_SCORE_TILE == ref.TILE
    K, N, H = _dims(R)
    case = _given(d, R, K, N, H)
    got = _host(_run(dev, case['traj'], case['emp32'], case['emp64'], N, R))
    _check_against_ref(got, case['ref'], R, 'd=%d R=%d' % (d, R))
    # the cell whose members all equal the observation: exactly 0 / 0 / R
    assert np.all(got['crps'][0, 0, H - 1] == 0.0) and got['energy'][0, 0, H - 1] == 0.0
    assert np.all(got['less'][0, 0, H - 1] == 0) and np.all(got['equal'][0, 0, H - 1] == R)
    # the member that equals the observation in two columns is counted there
    assert np.all(got['equal'][:, N - 1, :, 0] >= 1) and np.all(got['equal'][:, N - 1, :, d // 2] >= 1)
    if R == 1:                                                       # one member: |x - y| and ||x - y||, nothing subtracted
        x = ref.members(case['traj'][1], N, 1)[:, 0].astype(np.float64)
        assert np.array_equal(got['crps'][1], np.abs(x - case['emp64']))
        np.testing.assert_allclose(got['energy'][1], np.sqrt(((x - case['emp64']) ** 2).sum(-1)), rtol=(d + 2) * ref.U, atol=0)


# ------------------------------------------------------------------------------------------------------------ 2. the cap
@pytest.mark.parametrize('d', [64, 21])
def test_at_the_repeats_cap(dev, d):
    K, N, H, R = 1, 1, 2, 1024
    case = _given(d, R, K, N, H)
    got = _host(_run(dev, case['traj'], case['emp32'], case['emp64'], N, R))
    _check_against_ref(got, case['ref'], R, 'cap d=%d' % d)
    assert np.all(got['crps'][0, 0, H - 1] == 0.0) and got['energy'][0, 0, H - 1] == 0.0 and np.all(got['equal'][0, 0, H - 1] == R)


# -------------------------------------------------------------------------------- 3. K-independence and determinism
@pytest.mark.parametrize('d,R', [(21, 130), (64, 65), (15, 3)])
def test_independent_of_K_and_deterministic(dev, d, R):
    K, N, H = 3, 2, 3
    case = _given(d, R, K, N, H, with_ref=False)
    args = (case['emp32'], case['emp64'], N, R)
    whole = _run(dev, case['traj'], *args)
    again = _run(dev, case['traj'], *args)
    for key in KEYS:
        assert torch.equal(whole[key], again[key]), key
    for k in range(K):
        for rep in range(2):
            one = _run(dev, case['traj'][k:k + 1], *args)
            for key in KEYS:
                assert torch.equal(one[key][0], whole[key][k]), (key, k, rep)
    lean = _run(dev, case['traj'], *args, want_energy=False)
    assert lean['energy'] is None
    for key in ('crps', 'less', 'equal'):
        assert torch.equal(lean[key], whole[key]), key
    assert torch.equal(lean['summary'][..., 0], whole['summary'][..., 0]) and bool(torch.isnan(lean['summary'][..., 1]).all())


# ------------------------------------------------------------------------------------------ 4. one non-finite value
@pytest.mark.parametrize('what', ['nan member', 'inf member', 'inf observation'])
def test_a_non_finite_value_stays_in_its_cell(dev, what):
    d, R, K, N, H = 21, 65, 3, 2, 3
    case = _given(d, R, K, N, H, with_ref=False)
    clean = _run(dev, case['traj'], case['emp32'], case['emp64'], N, R)
    traj, emp32, emp64 = case['traj'].copy(), case['emp32'].copy(), case['emp64'].copy()
    k, n, l = 1, 1, 1
    if what == 'inf observation':
        emp32[n, l, 4] = emp64[n, l, 4] = np.inf
        hit = np.zeros((K, N, H), dtype=bool)
        hit[:, n, l] = True
    else:
        traj[k, 40 * N + n, l, 2] = np.nan if what == 'nan member' else -np.inf
        hit = np.zeros((K, N, H), dtype=bool)
        hit[k, n, l] = True
    got = _run(dev, traj, emp32, emp64, N, R)
    mask = torch.as_tensor(hit, device=dev)
    assert bool(torch.isnan(got['crps'][mask]).all()) and bool(torch.isnan(got['energy'][mask]).all())
    assert bool((got['less'][mask] == -1).all()) and bool((got['equal'][mask] == -1).all())
    for key in ('crps', 'less', 'equal', 'energy'):
        assert torch.equal(got[key][~mask], clean[key][~mask]), key
    hours = torch.as_tensor(hit.any(axis=1), device=dev)            # [K, H]: the hour's means hold the cell
    assert bool(torch.isnan(got['summary'][hours]).all())
    assert torch.equal(got['summary'][~hours], clean['summary'][~hours])


# ---------------------------------------------------------------------------------------------------- 5. end to end
def _emp(d, seed, N, H):
    """N held-out matrices [H, d], fp32-representable; row 0 of each is a start row."""
    rs = np.random.RandomState(seed)
    return rs.dirichlet(np.ones(d), size=(N, H)).astype(np.float32).astype(np.float64)


@pytest.mark.parametrize('d,precision', [(21, 'mixed'), (15, 'f64'), (21, 'f64'), (15, 'mixed')])
def test_population_forecast_score_end_to_end(dev, d, precision):
    from discrete_mean_field_game_amd import ops, population
    K, N, H, R = 3, 4, 6, 33
    emp = _emp(d, 7 + d, N, H)
    th, sh, al = [7.0, 8.5, 9.5], [0.3, 0.2, 0.4], [1e4, 1.2e4, 9e3]
    kw = dict(d=d, seed=4321, repeats=R, precision=precision, first_step=11)
    fc = population.forecast(th, sh, al, None, H, emp=emp, want_traj=True, **kw)
    sc = population.forecast_score(th, sh, al, emp, horizon=H, **kw)
    assert isinstance(sc, population.ForecastScore) and sc.repeats == R
    direct = _host(ops.forecast_score(torch.as_tensor(fc.traj, device=dev), torch.as_tensor(emp.astype(np.float32), device=dev),
                                      torch.as_tensor(emp, device=dev), N, R))
    for key in KEYS:
        assert np.array_equal(getattr(sc, key), direct[key]), key
    assert sc.crps.shape == (K, N, H, d) and sc.energy.shape == (K, N, H) and sc.summary.shape == (K, H, 2)
    assert np.all(np.isfinite(sc.crps)) and np.all(np.isfinite(sc.energy)) and np.all(sc.crps >= 0)
    # hour 0: every member is the start row, which is the observation
    assert np.all(sc.crps[:, :, 0] == 0.0) and np.all(sc.energy[:, :, 0] == 0.0) and np.all(sc.summary[:, 0] == 0.0)
    assert np.all(sc.less[:, :, 0] == 0) and np.all(sc.equal[:, :, 0] == R)
    # the band of the forecast's own order statistics holds y exactly when the counts say so
    y32 = emp.astype(np.float32)[None]
    for a, b in ((0, 2), (0, 1), (1, 2), (1, 1)):
        inside = (fc.quantiles[:, :, :, a, :] <= y32) & (y32 <= fc.quantiles[:, :, :, b, :])
        assert np.array_equal(population.covered(sc.less, sc.equal, fc.ranks[a], fc.ranks[b]), inside), (a, b)
    p = population.pit(sc.less, sc.equal, R)
    assert np.all((p >= 0) & (p <= 1))
    # chunking under a small budget (one policy per chunk) changes nothing; the default horizon is emp's rows
    parts = population.forecast_score(th, sh, al, emp, budget=population.forecast_score_bytes(N, H, d, R), **kw)
    lean = population.forecast_score(th, sh, al, emp, want_energy=False, **kw)
    for key in KEYS:
        assert np.array_equal(getattr(parts, key), getattr(sc, key)), key
    assert lean.energy is None and np.array_equal(lean.crps, sc.crps) and np.isnan(lean.summary[..., 1]).all()
    one = sc.learner(2)
    assert np.array_equal(one.crps, sc.crps[2]) and np.array_equal(one.summary, sc.summary[2])


def test_mixed_range_raises_on_its_own_context(dev):
    from discrete_mean_field_game_amd import _lib, ops, population
    ops.clear_status()
    emp = _emp(21, 3, 2, 4)
    args = ([8.0, 150.0], 0.5, 1e4, emp)             # 150 (1/2 + 0.5) > 86: beyond mixed precision's fp32 range
    with pytest.raises(_lib.MfgError):
        population.forecast_score(*args, d=21, repeats=3)
    assert ops.status(synchronize=True) == 0         # the caller's status word is left alone
    sc = population.forecast_score(*args, d=21, repeats=3, precision='f64')
    assert np.all(np.isfinite(sc.crps)) and np.all(np.isfinite(sc.summary))


# ------------------------------------------------------------------------------------- 6. class methods, grid search
def _policies(K, seed):
    rs = np.random.RandomState(seed)
    return (rs.uniform(6.0, 10.0, K), rs.uniform(0.1, 0.5, K), rs.uniform(8000.0, 14000.0, K),
            rs.randint(0, 2 ** 40, K).astype(np.int64))


def _write_files(d, seed, N=3, rows=16):
    rs = np.random.RandomState(seed)
    os.makedirs('test_normalized_round2')
    for day in range(N):
        np.savetxt('test_normalized_round2/trend_distribution_day%d.csv' % (22 + day), rs.dirichlet(np.ones(d + 2), size=rows),
                   fmt='%.3e', delimiter=' ')


def _same_score(a, b):
    for key in KEYS:
        x, y = getattr(a, key), getattr(b, key)
        assert np.array_equal(x, y, equal_nan=True), key


def _check_population(pop, d):
    """pop.forecast_score against population.forecast_score at the learners' parameters, seeds and Philox step;
    learner(k).forecast_score (the K = 1 form); the Philox step; a failed learner."""
    from discrete_mean_field_game_amd import population
    K, R, H = pop.K, 5, 6
    learners = [pop.learner(k) for k in range(K)]
    step0 = pop._rng_step
    assert step0 > 0
    sc = pop.forecast_score(indir='test_normalized_round2', horizon=H, repeats=R)
    assert pop._rng_step == step0 + H - 1
    emp = population.load_empirical('test_normalized_round2', d, H)
    want = population.forecast_score(pop.thetas, pop.shifts, pop.alpha_scales, emp, d=d, horizon=H, seed=pop.seeds, repeats=R,
                                     precision=pop.precision, first_step=step0)
    _same_score(sc, want)
    assert np.all(np.isfinite(sc.crps)) and np.all(sc.less >= 0)
    assert np.all(sc.crps.sum(-1)[:, :, 1:] > 0) and np.all(sc.energy[:, :, 1:] > 0)
    pop._rng_step = step0
    pop.forecast(indir='test_normalized_round2', horizon=H, repeats=R)           # forecast() advances the step by as much
    assert pop._rng_step == step0 + H - 1
    for k, lk in enumerate(learners):
        own = lk.forecast_score(None, H, R, emp=emp)
        assert lk._rng_step == step0 + H - 1
        assert isinstance(own.crps, np.ndarray) and own.crps.shape == (emp.shape[0], H, d) and own.summary.shape == (H, 2)
        _same_score(own, sc.learner(k))
    with pytest.raises(ValueError):
        pop.forecast_score()                          # nothing to score against
    step = pop._rng_step
    with pytest.raises(ValueError):
        pop.forecast_score(emp=emp, horizon=H, repeats=2000)
    assert pop._rng_step == step
    # a failed learner is not launched: NaN rows, counts -1; the others as before
    pop._rng_step = step0
    pop._act.state[1] = population.FAILED
    part = pop.forecast_score(emp=emp, horizon=H, repeats=R, want_energy=False)
    assert pop._rng_step == step0 + H - 1 and part.energy is None
    assert np.isnan(part.crps[1]).all() and np.isnan(part.summary[1]).all() and np.all(part.less[1] == -1) and np.all(part.equal[1] == -1)
    for k in (0, 2):
        assert np.array_equal(part.crps[k], sc.crps[k]) and np.array_equal(part.less[k], sc.less[k])
    pop._act.clear(1)


def test_actor_critic_population_forecast_score(dev, tmp_path, monkeypatch):
    from discrete_mean_field_game_amd.population import ActorCriticPopulation
    monkeypatch.chdir(tmp_path)
    d, K, B = 21, 3, 64
    _write_files(d, 5)
    th, sh, al, sd = _policies(K, 6)
    rs = np.random.RandomState(7)
    pop = ActorCriticPopulation(th, sh, al, d, batch=B, seeds=sd, w0=rs.rand(K, d * (d + 1) // 2 + d + 1) * 0.1,
                                pi0=rs.dirichlet(np.ones(d), size=16), update_every='step')
    pop.train(1)
    _check_population(pop, d)


def test_ac_irl_population_forecast_score(dev, tmp_path, monkeypatch):
    from discrete_mean_field_game_amd.irl_population import AC_IRLPopulation
    from discrete_mean_field_game_amd.networks import RewardNet
    monkeypatch.chdir(tmp_path)
    d, K, B = 15, 3, 64
    _write_files(d, 8)
    th, sh, al, sd = _policies(K, 9)
    torch.manual_seed(1)
    net = RewardNet(d=d, n_fc3=8, n_fc4=4, keep_prob=1.0).to(dev)
    rs = np.random.RandomState(2)
    pop = AC_IRLPopulation(th, sh, al, d, batch=B, reward_nets=net, seeds=sd, w0=rs.rand(K, d * (d + 1) // 2 + d + 1) * 0.1,
                           pi0=rs.dirichlet(np.ones(d), size=9))
    pop.train(1)
    _check_population(pop, d)


def test_gridsearch_score(dev, tmp_path, monkeypatch):
    from discrete_mean_field_game_amd import population
    monkeypatch.chdir(tmp_path)
    d, Lh, R, seed = 7, 4, 8, 99
    _write_files(d, 3, N=2, rows=5)
    grid = ([7.0, 9.0], [0.2, 0.4], [9000.0, 12000.0])
    best = population.gridsearch_score(*grid, 'test_normalized_round2', 'score.csv', d=d, seed=seed, episode_length=Lh, repeats=R)
    points = population.grid_points(*grid)
    assert len(points) == 8 and points[1] == (7.0, 0.2, 12000.0)
    par = np.array(points)
    emp = population.load_empirical('test_normalized_round2', d, Lh)
    fc = population.forecast(par[:, 0], par[:, 1], par[:, 2], None, Lh, d=d, seed=seed, repeats=R, emp=emp, want_traj=True)
    want = ref.score(fc.traj, emp.astype(np.float32), emp, emp.shape[0], R)
    table = np.stack([want['crps'][:, :, 1:].mean(axis=(1, 2, 3)), want['crps'][:, :, -1].mean(axis=(1, 2)),
                      want['energy'][:, :, 1:].mean(axis=(1, 2)), want['energy'][:, :, -1].mean(axis=1)], axis=1)
    lines = open('score.csv').read().splitlines()
    assert lines[0] + '\n' == population.SCORE_HEADER == 'theta,shift,alpha_scale,crps_mean,crps_final,energy_mean,energy_final\n'
    assert lines[1:] == [(population.SCORE_FMT % (tuple(p) + tuple(row))).rstrip('\n') for p, row in zip(points, table)]
    assert len(best) == 4
    for q in range(4):
        last_min = max(i for i in range(8) if table[i, q] <= table[:, q].min())
        assert best[q][1:] == list(points[last_min])
        np.testing.assert_allclose(best[q][0], table[last_min, q], rtol=1e-12, atol=0)
    again = population.gridsearch_score(*grid, 'test_normalized_round2', 'score.csv', d=d, seed=seed, episode_length=Lh, repeats=R)
    assert again == best
    both = open('score.csv').read().splitlines()
    assert both == lines + lines[1:]                  # a second call appends, under the one header


# ----------------------------------------------------------------------------------------------------------- 7. refusals
def _raw_call(dev, **kw):
    """mfg_forecast_score through the binding with real device buffers that hold a sentinel; returns (code, buffers)."""
    from discrete_mean_field_game_amd import _lib, ops
    d, K, N, H, R = 21, 2, 3, 4, 4
    a = dict(R=R, d=d, H=H, K=K, short=0, emp32=True)
    a.update(kw)
    case = _given(d, R, K, N, H, with_ref=False)
    t = lambda x: torch.as_tensor(np.array(x), device=dev)
    traj, e32, e64 = t(case['traj']), t(case['emp32']), t(case['emp64'])
    bufs = {'crps': torch.full((K, N, H, d), -7.0, dtype=torch.float64, device=dev),
            'less': torch.full((K, N, H, d), -7, dtype=torch.int32, device=dev),
            'equal': torch.full((K, N, H, d), -7, dtype=torch.int32, device=dev),
            'energy': torch.full((K, N, H), -7.0, dtype=torch.float64, device=dev),
            'summary': torch.full((K, H, 2), -7.0, dtype=torch.float64, device=dev)}
    ws = ops.forecast_score_workspace(N, H, d, K, R, dev)
    rc = _lib.lib().mfg_forecast_score(traj.data_ptr(), N, a['H'], a['d'], a['K'], a['R'], e32.data_ptr() if a['emp32'] else None,
                                       e64.data_ptr(), bufs['crps'].data_ptr(), bufs['less'].data_ptr(), bufs['equal'].data_ptr(),
                                       bufs['energy'].data_ptr(), bufs['summary'].data_ptr(), ws.data_ptr(),
                                       ws.numel() * 8 - a['short'], None)
    torch.cuda.synchronize()
    return rc, bufs


@pytest.mark.parametrize('kw,code', [(dict(R=1025), EUNSUPPORTED), (dict(d=65), EUNSUPPORTED), (dict(R=0), EINVAL), (dict(H=1), EINVAL),
                                     (dict(K=0), EINVAL), (dict(emp32=False), EINVAL), (dict(short=1), EWORKSPACE)])
def test_refusals_launch_nothing(dev, kw, code):
    from discrete_mean_field_game_amd import _lib
    rc, bufs = _raw_call(dev, **kw)
    assert rc == code
    assert _lib.lib().mfg_last_error()
    for name, t in bufs.items():
        assert bool((t == -7).all()), name
    rc, bufs = _raw_call(dev)                         # the same buffers' shapes, good arguments: everything is written
    assert rc == 0
    for name, t in bufs.items():
        assert not bool((t == -7).any()), name
