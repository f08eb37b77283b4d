"""-m gpu: the ensemble forecast (mfg_forecast_pop, ops.forecast_pop, population.forecast, the populations' and
actor_critic's forecast()).  The members are torch.equal to single ops.rollout calls; mean, std, the order statistics and the
error curves match NumPy on those members (the trajectories the same call returns); learner k's outputs do not depend on K;
bad arguments are refused before anything is launched; the classes give what population.forecast gives at their learners'
parameters, seeds and Philox step.
"""
import ctypes as C
import functools
import os

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

H = 6
EINVAL, EUNSUPPORTED, EWORKSPACE = -1, -3, -4


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.fail('-m gpu tests need a GPU')
    from discrete_mean_field_game_amd import ops
    ops.init()
    return torch.device('cuda', 0)


def _emp(d, seed, N, L=H):
    """N held-out matrices [L, d] as the files hold them ('%.3e' text), a few exact zeros included (the JSD's 1e-100 branch);
    row 0 of each is a start row."""
    rs = np.random.RandomState(seed)
    m = np.array([[[float('%.3e' % v) for v in row] for row in rs.dirichlet(np.ones(d), size=L)] for _ in range(N)])
    m[0, 0, d // 2] = 0.0
    m[0, min(3, L - 1):, d // 3] = 0.0
    m[-1, -1, 0] = 0.0
    m[-1, 0, d - 1] = 0.0
    return m


def _policies(K, seed):
    rs = np.random.RandomState(seed)
    seeds = rs.randint(0, 2 ** 40, K).astype(np.int64)
    th, sh, al = rs.uniform(6.0, 10.0, K), rs.uniform(0.1, 0.5, K), rs.uniform(8000.0, 14000.0, K)
    if K > 1:                        # two learners with the same policy on the same noise
        seeds[1], th[1], sh[1], al[1] = seeds[0], th[0], sh[0], al[0]
    return th, sh, al, seeds


def _dev_args(dev, th, sh, al, sd):
    f = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=dev)
    return f(th), f(sh), f(al), torch.as_tensor(np.ascontiguousarray(sd, dtype=np.int64), device=dev)


def _ranks(R):
    """(0, R - 1, R // 2, 1, 1): unsorted, with a repeat (rank 1 does not exist in an ensemble of one: R - 1 there)."""
    one = min(1, R - 1)
    return (0, R - 1, R // 2, one, one)


@functools.lru_cache(maxsize=None)
def _forecast(d, precision, K, N, R, Hh=H, first_step=37, with_emp=True):
    """One ops.forecast_pop call with the trajectories, as NumPy arrays (shared by the tests: computed once, never changed)."""
    from discrete_mean_field_game_amd import ops
    dev = torch.device('cuda', 0)
    emp = _emp(d, 100 + d + N, N, Hh)
    th, sh, al, sd = _policies(K, d + K)
    start32 = torch.as_tensor(emp[:, 0].astype(np.float32), device=dev)
    kw = {}
    if with_emp:
        kw = dict(emp32=torch.as_tensor(emp.astype(np.float32), device=dev), emp64=torch.as_tensor(emp.copy(), device=dev))
    out = ops.forecast_pop(start32, *_dev_args(dev, th, sh, al, sd), Hh, first_step=first_step, repeats=R, ranks=_ranks(R),
                           precision=precision, want_traj=True, **kw)
    res = {k: None if v is None else v.cpu().numpy() for k, v in out.items()}
    res.update(emp=emp, policies=(th, sh, al, sd), first_step=first_step, traj_dev=out['traj'])
    for v in res.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return res


def _members(traj_k, N, R):
    """[N R, H, d] -> [N, R, H, d]: member r of start state n is trajectory r N + n."""
    return traj_k.reshape(R, N, *traj_k.shape[1:]).transpose(1, 0, 2, 3)


# (d, precision, K, N, R): N R = 15, 5, 66, 5 trajectories, never a multiple of a rollout tile's 12 (d = 21), 16 (15), 36 (7), 4 (64)
MEMBER_CASES = [(21, 'mixed', 3, 5, 3), (15, 'f64', 1, 5, 1), (7, 'mixed', 3, 2, 33), (64, 'f64', 1, 1, 5)]


@pytest.mark.parametrize('d,precision,K,N,R', MEMBER_CASES)
def test_members_equal_single_rollouts(dev, d, precision, K, N, R):
    from discrete_mean_field_game_amd import ops
    f = _forecast(d, precision, K, N, R)
    th, sh, al, sd = f['policies']
    traj = f['traj_dev']
    assert traj.shape == (K, N * R, H, d)
    starts = torch.as_tensor(np.tile(f['emp'][:, 0], (R, 1)).astype(np.float32), device=dev)
    for k in range(K):
        ref = ops.rollout(starts, H - 1, torch.tensor([th[k]], dtype=torch.float64, device=dev), float(sh[k]), float(al[k]),
                          seed=int(sd[k]), first_step=f['first_step'], td=False, precision=precision)['pi_traj']
        assert torch.equal(traj[k], ref), 'learner %d' % k
        assert torch.equal(traj[k, :, 0], starts)            # row 0 of every member is its start row


def _check_moments(f, K, N, R):
    """mean / std against NumPy in float64 over the members.  Values lie in [0, 1], so any summation order of R terms stays
    within R 2^-53 of the exact sum and two orders within 2 R 2^-53 of each other: absolute for the mean; the sum of squares
    has positive terms only, hence the same bound relative for the std (2^-60 absolute for cells whose std is 0 or denormal)."""
    tol = 2.0 * R * 2.0 ** -53
    for k in range(K):
        m = _members(f['traj'][k], N, R).astype(np.float64)
        want_mean, want_std = np.mean(m, axis=1), np.std(m, axis=1)
        err_mean = np.max(np.abs(f['mean'][k] - want_mean))
        err_std = np.max(np.abs(f['std'][k] - want_std) - tol * np.abs(want_std))
        print('learner %d: max |mean - np.mean| = %.3e (tol %.3e), max std excess = %.3e (abs tol %.3e)'
              % (k, err_mean, tol, err_std, 2.0 ** -60))
        assert np.all(np.isfinite(f['mean'][k])) and np.all(np.isfinite(f['std'][k]))
        assert err_mean <= tol, k
        assert err_std <= 2.0 ** -60, k
        # row 0: R copies of the start row -- R x is exact for fp32 x, so the mean is x and every deviation 0
        start = f['emp'][:, 0].astype(np.float32).astype(np.float64)
        assert np.array_equal(f['mean'][k][:, 0], start)
        assert np.array_equal(f['std'][k][:, 0], np.zeros_like(start))


@pytest.mark.parametrize('d,precision,K,N,R', MEMBER_CASES + [(21, 'mixed', 2, 3, 257), (15, 'mixed', 2, 2, 130), (64, 'mixed', 2, 2, 65)])
def test_moments_match_numpy(dev, d, precision, K, N, R):
    _check_moments(_forecast(d, precision, K, N, R), K, N, R)


def _check_quant(f, K, N, R):
    ranks = list(_ranks(R))
    assert f['quant'].shape == (K, N, f['traj'].shape[2], len(ranks), f['traj'].shape[3])
    for k in range(K):
        m = _members(f['traj'][k], N, R)                                  # fp32 [N, R, H, d]
        want = np.sort(m, axis=1)[:, ranks].transpose(0, 2, 1, 3)         # [N, Q, H, d] -> [N, H, Q, d]
        assert np.array_equal(f['quant'][k], want), k


# R below, at and above a wave's 64 lanes and above a power of two, for every d
@pytest.mark.parametrize('d', [21, 15, 7, 64])
@pytest.mark.parametrize('R', [1, 2, 3, 33, 64, 65, 130, 257])
def test_order_statistics_match_numpy_sort(dev, d, R):
    K, N = 2, 2
    f = _forecast(d, 'mixed', K, N, R, 3)
    _check_quant(f, K, N, R)
    _check_moments(f, K, N, R)


# the cap: d = 64 goes in five chunks of 15, 15, 15, 15, 4 columns, d = 21 in two of 15 and 6 (the chunk rule on both sides)
@pytest.mark.parametrize('d,N', [(64, 1), (21, 1), (15, 2)])
def test_at_the_repeats_cap(dev, d, N):
    from discrete_mean_field_game_amd import _lib
    R = _lib.FORECAST_MAX_REPEATS
    f = _forecast(d, 'mixed', 1, N, R, 2)
    _check_quant(f, 1, N, R)
    _check_moments(f, 1, N, R)


def test_independent_of_K_and_deterministic(dev):
    from discrete_mean_field_game_amd import ops
    d, K, N, R = 21, 37, 3, 5
    f = _forecast(d, 'mixed', K, N, R)
    th, sh, al, sd = f['policies']
    emp = f['emp']
    start32 = torch.as_tensor(emp[:, 0].astype(np.float32), device=dev)
    e32, e64 = torch.as_tensor(emp.astype(np.float32), device=dev), torch.as_tensor(emp.copy(), device=dev)
    for k in (0, 17, 36):
        alone = ops.forecast_pop(start32, *_dev_args(dev, th[k:k + 1], sh[k:k + 1], al[k:k + 1], sd[k:k + 1]), H,
                                 first_step=f['first_step'], repeats=R, ranks=_ranks(R), emp32=e32, emp64=e64)
        assert alone['traj'] is None
        for key in ('mean', 'std', 'quant', 'curves'):
            assert np.array_equal(alone[key][0].cpu().numpy(), f[key][k]), (key, k)
    for key in ('mean', 'std', 'quant', 'curves', 'traj'):
        assert np.array_equal(f[key][0], f[key][1]), key       # the same policy on the same seed
        assert not np.array_equal(f[key][0], f[key][2]), key
    # without held-out rows and without ranks: the same moments, nothing else
    bare = ops.forecast_pop(start32, *_dev_args(dev, th, sh, al, sd), H, first_step=f['first_step'], repeats=R)
    assert bare['quant'] is None and bare['curves'] is None and bare['traj'] is None
    assert np.array_equal(bare['mean'].cpu().numpy(), f['mean']) and np.array_equal(bare['std'].cpu().numpy(), f['std'])


def _np_curves(emp, traj):
    """The per-step terms of mfg_ac2.py:631-666 on given trajectories [N R, H, d] (the project's JSD argument order: empirical
    first): mean and std over the members of the step's L1 and JSD, [H, 4]."""
    from oracle import mfg_oracle as O
    e32 = emp.astype(np.float32).astype(np.float64)
    N, Hh = emp.shape[0], emp.shape[1]
    l1 = np.zeros((traj.shape[0], Hh))
    jsd = np.zeros((traj.shape[0], Hh))
    for j in range(traj.shape[0]):
        mt = traj[j].astype(np.float64)
        for l in range(Hh):
            l1[j, l] = np.linalg.norm(mt[l] - emp[j % N, l], ord=1)
            jsd[j, l] = O.JSD(e32[j % N, l].copy(), mt[l].copy())
    return np.stack([l1.mean(0), l1.std(0), jsd.mean(0), jsd.std(0)], axis=1)


def _assert_curves(curves_k, emp, traj_k, what):
    """One policy's error curves against the restatement on its own members."""
    assert np.all(np.isfinite(curves_k)), what
    np.testing.assert_allclose(curves_k, _np_curves(emp, traj_k), rtol=1e-12, atol=1e-15, err_msg=what)


@pytest.mark.parametrize('d,precision,K,N,R', [(21, 'mixed', 3, 5, 3), (15, 'f64', 1, 5, 1), (7, 'mixed', 3, 2, 33), (64, 'f64', 1, 1, 5)])
def test_curves_match_numpy_and_evaluate_pop(dev, d, precision, K, N, R):
    from discrete_mean_field_game_amd import ops
    f = _forecast(d, precision, K, N, R)
    emp = f['emp']
    assert f['curves'].shape == (K, H, 4)
    for k in range(K):
        _assert_curves(f['curves'][k], emp, f['traj'][k], 'learner %d' % k)
    # the same quantities through the existing call: its final-row columns are step H - 1, its mean-row means the mean over l
    e32, e64 = torch.as_tensor(emp.astype(np.float32), device=dev), torch.as_tensor(emp.copy(), device=dev)
    metrics, traj = ops.evaluate_pop(e32, e64, *_dev_args(dev, *f['policies']), first_step=f['first_step'], repeats=R,
                                     precision=precision, want_traj=True)
    assert torch.equal(traj, f['traj_dev'])
    metrics = metrics.cpu().numpy()
    c = f['curves']
    np.testing.assert_allclose(c[:, H - 1][:, [0, 2]], metrics[:, [0, 4]], rtol=1e-12, atol=0)
    np.testing.assert_allclose(c[:, H - 1][:, [1, 3]], metrics[:, [1, 5]], rtol=1e-12, atol=1e-18)
    np.testing.assert_allclose(c[:, :, [0, 2]].mean(axis=1), metrics[:, [2, 6]], rtol=1e-12, atol=0)


def _raw_call(dev, **kw):
    """mfg_forecast_pop through the binding with real device buffers that hold a sentinel; returns (code, buffers)."""
    from discrete_mean_field_game_amd import _lib, ops
    d, K, N, R = 21, 2, 3, 4
    a = dict(R=R, ranks=(0, 3, 1), emp32=True, emp64=True, short=0)
    a.update(kw)
    emp = _emp(d, 5, N)
    th, sh, al, sd = _dev_args(dev, *_policies(K, 7))
    start32 = torch.as_tensor(emp[:, 0].astype(np.float32), device=dev)
    e32, e64 = torch.as_tensor(emp.astype(np.float32), device=dev), torch.as_tensor(emp.copy(), device=dev)
    Q = len(a['ranks'])
    Rb = max(a['R'], R)
    bufs = {'mean': torch.full((K, N, H, d), -7.0, dtype=torch.float64, device=dev),
            'std': torch.full((K, N, H, d), -7.0, dtype=torch.float64, device=dev),
            'quant': torch.full((K, N, H, max(Q, 1), d), -7.0, dtype=torch.float32, device=dev),
            'curves': torch.full((K, H, 4), -7.0, dtype=torch.float64, device=dev),
            'traj': torch.full((K, N * Rb, H, d), -7.0, dtype=torch.float32, device=dev)}
    ws = ops.forecast_pop_workspace(N, H, d, K, Rb, True, dev)
    rk = (C.c_int32 * 16)(*a['ranks'])
    rc = _lib.lib().mfg_forecast_pop(start32.data_ptr(), N, H, d, K, th.data_ptr(), sh.data_ptr(), al.data_ptr(), sd.data_ptr(), 0,
                                     a['R'], 1, rk, Q, e32.data_ptr() if a['emp32'] else None,
                                     e64.data_ptr() if a['emp64'] else None, bufs['mean'].data_ptr(), bufs['std'].data_ptr(),
                                     bufs['quant'].data_ptr(), bufs['curves'].data_ptr(), bufs['traj'].data_ptr(), ws.data_ptr(),
                                     ws.numel() * 8 - a['short'], None)
    torch.cuda.synchronize()
    return rc, bufs


@pytest.mark.parametrize('kw,code', [(dict(ranks=(0, 4)), EINVAL), (dict(ranks=(0, 1, 2, 3, 0, 1, 2, 3, 0)), EINVAL),
                                     (dict(emp32=False), EINVAL), (dict(emp64=False), EINVAL),
                                     (dict(R=1025), EUNSUPPORTED), (dict(short=8), EWORKSPACE)])
def test_refusals_launch_nothing(dev, kw, code):
    from discrete_mean_field_game_amd import _lib
    rc, bufs = _raw_call(dev, **kw)
    assert rc == code
    assert _lib.lib().mfg_last_error()
    for name, t in bufs.items():
        assert bool((t == -7.0).all()), name
    rc, bufs = _raw_call(dev)                       # the same buffers' shapes, good arguments: everything is written
    assert rc == 0
    for name, t in bufs.items():
        assert not bool((t == -7.0).any()), name


def test_mixed_range_raises_on_its_own_context(dev):
    from discrete_mean_field_game_amd import _lib, ops, population
    ops.clear_status()
    pi0 = _emp(21, 3, 2)[:, 0]
    args = ([8.0, 150.0], 0.5, 1e4, pi0, H)          # 150 (1/2 + 0.5) > 86: beyond mixed precision's fp32 range
    with pytest.raises(_lib.MfgError):
        population.forecast(*args, d=21, repeats=3)
    assert ops.status(synchronize=True) == 0         # the caller's status word is left alone
    fc = population.forecast(*args, d=21, repeats=3, precision='f64')
    assert fc.mean.shape == (2, 2, H, 21) and np.all(np.isfinite(fc.mean)) and np.all(np.isfinite(fc.quantiles))
    assert fc.curves is None and fc.traj is None and fc.ranks == (0, 1, 1) and fc.probs == (0.05, 0.5, 0.95)


def test_population_forecast_chunks_and_common_random_numbers(dev, monkeypatch):
    from discrete_mean_field_game_amd import population
    emp = _emp(21, 9, 3)
    th = [7.0, 8.5, 8.5, 9.5, 6.5]
    kw = dict(d=21, seed=12345, repeats=5, probs=(0.0, 0.5, 1.0), emp=emp)
    whole = population.forecast(th, 0.3, 1e4, None, H, **kw)
    assert whole.quantiles.shape == (5, 3, H, 3, 21) and whole.curves.shape == (5, H, 4)
    assert np.array_equal(whole.mean[1], whole.mean[2]) and np.array_equal(whole.curves[1], whole.curves[2])
    monkeypatch.setattr(population, 'FORECAST_CHUNK', 2)
    parts = population.forecast(th, 0.3, 1e4, None, H, **kw)
    for key in ('mean', 'std', 'quantiles', 'curves'):
        assert np.array_equal(getattr(parts, key), getattr(whole, key)), key
    # the bands are ordered and hold the mean's range: min <= median <= max, min <= mean <= max
    q = whole.quantiles.astype(np.float64)
    assert np.all(q[..., 0, :] <= q[..., 1, :]) and np.all(q[..., 1, :] <= q[..., 2, :])
    assert np.all(q[..., 0, :] <= whole.mean + 1e-15) and np.all(whole.mean <= q[..., 2, :] + 1e-15)


def _write_files(d, seed, N=3, rows=16):
    rs = np.random.RandomState(seed)
    os.makedirs('test_normalized_round2')
    os.makedirs('eval_mfg_round2')
    for day in range(N):
        np.savetxt('test_normalized_round2/trend_distribution_day%d.csv' % (22 + day), rs.dirichlet(np.ones(d + 2), size=rows),
                   fmt='%.3e', delimiter=' ')


def _same_forecast(a, b, keys=('mean', 'std', 'quantiles', 'curves')):
    for key in keys:
        x, y = getattr(a, key), getattr(b, key)
        assert (x is None) == (y is None), key
        if x is not None:
            assert np.array_equal(x, y), key


def _check_population(pop, d):
    """pop.forecast against population.forecast at the learners' parameters, seeds and Philox step; learner(k).forecast; the
    Philox step; an evaluate() after it."""
    from discrete_mean_field_game_amd import ops, population
    K, R, probs = pop.K, 5, (0.0, 0.5, 1.0)
    dev = pop.device
    learners = [pop.learner(k) for k in range(K)]
    twins = [pop.learner(k) for k in range(K)]
    step0 = pop._rng_step
    assert step0 > 0
    fc = pop.forecast(indir='test_normalized_round2', horizon=H, repeats=R, probs=probs, want_traj=True)
    assert pop._rng_step == step0 + H - 1
    emp = population.load_empirical('test_normalized_round2', d, H)
    want = population.forecast(pop.thetas, pop.shifts, pop.alpha_scales, None, H, d=d, seed=pop.seeds, repeats=R, probs=probs,
                               emp=emp, precision=pop.precision, first_step=step0, want_traj=True)
    _same_forecast(fc, want, ('mean', 'std', 'quantiles', 'curves', 'traj'))
    assert fc.curves.shape == (K, H, 4) and np.all(np.isfinite(fc.curves))
    pi0 = emp[:, 0]
    for k, lk in enumerate(learners):
        own = lk.forecast(pi0, H, R, probs, emp=emp, want_traj=True)
        assert lk._rng_step == step0 + H - 1
        assert isinstance(own.mean, np.ndarray) and own.mean.shape == (emp.shape[0], H, d)
        _same_forecast(own, fc.learner(k), ('mean', 'std', 'quantiles', 'curves', 'traj'))
        # member 0 of a single start row is the sample path generate_trajectory gives from the same state
        a, b = twins[k], pop.learner(k)
        b._rng_step = step0
        path = b.generate_trajectory(pi0[0], H)
        one = a.forecast(pi0[0], H, 3, want_traj=True)
        assert a._rng_step == step0 + H - 1 == b._rng_step
        assert np.array_equal(one.traj[0], path.astype(np.float32))
        a._rng_step = step0
        assert np.array_equal(a.forecast(pi0[0], H, 1).mean[0], path)        # an ensemble of one: its mean is the path
    # an evaluate() after the forecast runs on the NEXT Philox steps: it shares no noise with the forecast
    res = pop.evaluate(outfile='eval_mfg_round2/pop.csv')
    assert pop._rng_step == step0 + (H - 1) + 15
    emp16 = population.load_empirical('test_normalized_round2', d, 16)
    e32, e64 = torch.as_tensor(emp16.astype(np.float32), device=dev), torch.as_tensor(emp16, device=dev)
    f = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=dev)
    seeds = torch.as_tensor(pop.seeds.view(np.int64), device=dev)
    nxt = ops.evaluate_pop(e32, e64, f(pop.thetas), f(pop.shifts), f(pop.alpha_scales), seeds, first_step=step0 + H - 1,
                           precision=pop.precision).cpu().numpy()
    same = ops.evaluate_pop(e32, e64, f(pop.thetas), f(pop.shifts), f(pop.alpha_scales), seeds, first_step=step0,
                            precision=pop.precision).cpu().numpy()
    assert np.array_equal(res, nxt[:, 0::2])
    assert not np.array_equal(res, same[:, 0::2])


def test_actor_critic_population_forecast(dev, tmp_path, monkeypatch):
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
    with pytest.raises(ValueError):
        pop.forecast()                               # neither start rows nor a directory
    step = pop._rng_step
    with pytest.raises(ValueError):
        pop.forecast(pi0=np.full(d, 1.0 / d), repeats=2000)
    assert pop._rng_step == step


def test_ac_irl_population_forecast(dev, tmp_path, monkeypatch):
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
