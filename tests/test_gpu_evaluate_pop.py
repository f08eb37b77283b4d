"""-m gpu: the selection step for K policies (mfg_evaluate_pop, ops.evaluate_pop, ActorCriticPopulation.evaluate,
AC_IRLPopulation.evaluate, population.gridsearch).  The trajectories are torch.equal to single ops.rollout calls, the
metrics match a NumPy restatement of mfg_ac2.py:631-666 on those trajectories, and the classes give what their learners'
own evaluate() gives.
"""
import os

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

N_FILES, ROWS = 5, 16


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.fail('-m gpu tests need a GPU')
    from discrete_mean_field_game_amd import ops
    ops.init()
    return torch.device('cuda', 0)


def _emp(d, seed, N=N_FILES, L=ROWS):
    """N test matrices [L, d] as the files hold them ('%.3e' text), a few exact zeros included (the JSD's 1e-100 branch)."""
    rs = np.random.RandomState(seed)
    m = np.array([[[float('%.3e' % v) for v in row] for row in rs.dirichlet(np.ones(d), size=L)] for _ in range(N)])
    m[0, 3:, d // 2] = 0.0
    m[1, -1, 0] = 0.0
    return m


def _policies(K, seed):
    rs = np.random.RandomState(seed)
    seeds = rs.randint(0, 2 ** 40, K).astype(np.int64)
    if K > 1:
        seeds[1] = seeds[0]          # two learners on the same noise
    return rs.uniform(6.0, 10.0, K), rs.uniform(0.1, 0.5, K), rs.uniform(8000.0, 14000.0, K), seeds


def _dev_args(dev, th, sh, al, sd):
    f = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=dev)
    return f(th), f(sh), f(al), torch.as_tensor(np.ascontiguousarray(sd, dtype=np.int64), device=dev)


def _run(dev, emp, th, sh, al, sd, first_step, R, precision):
    from discrete_mean_field_game_amd import ops
    e64 = torch.as_tensor(emp, dtype=torch.float64, device=dev)
    e32 = torch.as_tensor(emp.astype(np.float32), device=dev)
    return ops.evaluate_pop(e32, e64, *_dev_args(dev, th, sh, al, sd), first_step=first_step, repeats=R, precision=precision,
                            want_traj=True)


def _np_metrics(emp, traj):
    """mfg_ac2.py:631-666 on given trajectories [N R, L, d] (the project's JSD argument order: empirical first)."""
    from oracle import mfg_oracle as O
    e32 = emp.astype(np.float32).astype(np.float64)
    N, L = emp.shape[0], emp.shape[1]
    cols = np.zeros((traj.shape[0], 4))
    for j in range(traj.shape[0]):
        me, mt, m32 = emp[j % N], traj[j].astype(np.float64), e32[j % N]
        cols[j, 0] = np.linalg.norm(mt[-1] - me[-1], ord=1)
        cols[j, 1] = np.mean(np.apply_along_axis(lambda row: np.linalg.norm(row, ord=1), 1, me - mt))
        cols[j, 2] = O.JSD(m32[-1], mt[-1])
        cols[j, 3] = sum(O.JSD(m32[l], mt[l]) for l in range(L)) / L
    out = []
    for q in range(4):
        out += [np.mean(cols[:, q]), np.std(cols[:, q])]
    return np.array(out)


def _assert_metrics(metrics_k, emp, traj_k, what):
    """One policy's eight metrics against the restatement on its own trajectories."""
    assert np.all(np.isfinite(metrics_k)), what
    np.testing.assert_allclose(metrics_k, _np_metrics(emp, traj_k), rtol=1e-12, atol=1e-15, err_msg=what)


# (d, precision, K, R): N R = 5 or 15 trajectories, never a multiple of a block's 12 (d = 21), 16 (15), 36 (7) or 4 (64)
CASES = [(21, 'mixed', 37, 1), (21, 'f64', 3, 3), (15, 'mixed', 3, 3), (15, 'f64', 1, 1), (7, 'mixed', 3, 1), (7, 'f64', 3, 3),
         (64, 'mixed', 1, 3), (64, 'f64', 3, 1)]


@pytest.mark.parametrize('d,precision,K,R', CASES)
def test_trajectories_equal_single_rollouts(dev, d, precision, K, R):
    from discrete_mean_field_game_amd import ops
    emp = _emp(d, 10 + d)
    th, sh, al, sd = _policies(K, d + K)
    first_step = 37
    _, traj = _run(dev, emp, th, sh, al, sd, first_step, R, precision)
    assert traj.shape == (K, N_FILES * R, ROWS, d)
    starts = torch.as_tensor(np.tile(emp[:, 0], (R, 1)).astype(np.float32), device=dev)
    for k in range(K):
        ref = ops.rollout(starts, ROWS - 1, torch.tensor([th[k]], dtype=torch.float64, device=dev), float(sh[k]), float(al[k]),
                          seed=int(sd[k]), first_step=first_step, td=False, precision=precision)['pi_traj']
        assert torch.equal(traj[k], ref), 'learner %d' % k


@pytest.mark.parametrize('d,precision,K,R', [(21, 'mixed', 3, 3), (15, 'f64', 3, 1), (7, 'mixed', 1, 3), (64, 'f64', 3, 3)])
def test_metrics_match_numpy_restatement(dev, d, precision, K, R):
    emp = _emp(d, 20 + d)
    th, sh, al, sd = _policies(K, 3 * d)
    metrics, traj = _run(dev, emp, th, sh, al, sd, 5, R, precision)
    metrics, traj = metrics.cpu().numpy(), traj.cpu().numpy()
    for k in range(K):
        _assert_metrics(metrics[k], emp, traj[k], 'learner %d' % k)


def test_deterministic_and_independent_of_K(dev):
    from discrete_mean_field_game_amd import ops
    d, K = 21, 37
    emp = _emp(d, 3)
    th, sh, al, sd = _policies(K, 4)
    m1, t1 = _run(dev, emp, th, sh, al, sd, 11, 3, 'mixed')
    m2, t2 = _run(dev, emp, th, sh, al, sd, 11, 3, 'mixed')
    assert torch.equal(m1, m2) and torch.equal(t1, t2)
    e64 = torch.as_tensor(emp, dtype=torch.float64, device=dev)
    e32 = torch.as_tensor(emp.astype(np.float32), device=dev)
    for k in (0, 17, 36):
        alone = ops.evaluate_pop(e32, e64, *_dev_args(dev, th[k:k + 1], sh[k:k + 1], al[k:k + 1], sd[k:k + 1]), first_step=11,
                                 repeats=3)
        assert torch.equal(alone[0], m1[k]), k


def _write_files(d, seed, N=N_FILES, rows=ROWS):
    rs = np.random.RandomState(seed)
    os.makedirs('test_normalized_round2')
    os.makedirs('eval_mfg_round2')
    for day in range(N):
        np.savetxt('test_normalized_round2/trend_distribution_day%d.csv' % (22 + day), rs.dirichlet(np.ones(d + 2), size=rows),
                   fmt='%.3e', delimiter=' ')


def _csv(path):
    return [line.split(',') for line in open(path).read().strip().split('\n')]


def _same_lines(pop_lines, own_lines):
    assert len(pop_lines) == len(own_lines)
    for a, b in zip(pop_lines, own_lines):
        assert a[:3] == b[:3]
        np.testing.assert_allclose([float(v) for v in a[3:]], [float(v) for v in b[3:]], rtol=1e-12, atol=0)


def test_actor_critic_population_evaluate_equals_learners(dev, tmp_path, monkeypatch):
    from discrete_mean_field_game_amd.population import ActorCriticPopulation
    monkeypatch.chdir(tmp_path)
    d, K, B, E = 21, 4, 64, 2
    _write_files(d, 5)
    th, sh, al, sd = _policies(K, 6)
    rs = np.random.RandomState(7)
    table = rs.dirichlet(np.ones(d), size=16)
    w0 = rs.rand(K, d * (d + 1) // 2 + d + 1) * 0.1
    pop = ActorCriticPopulation(th, sh, al, d, batch=B, seeds=sd, w0=w0, pi0=table, update_every='step')
    pop.train(E)
    learners = [pop.learner(k) for k in range(K)]
    thetas = pop.thetas
    res = pop.evaluate(outfile='eval_mfg_round2/pop.csv', write_header=1)
    assert res.shape == (K, 4)
    lines = _csv('eval_mfg_round2/pop.csv')
    assert ','.join(lines[0]).strip() == 'theta,shift,alpha_scale,mean_l1_final,std_l1_final,mean_l1_mean,std_l1_mean,' \
                                         'mean_JSD_final,std_JSD_final,mean_JSD_mean,std_JSD_mean'
    for k, lk in enumerate(learners):
        own = lk.evaluate(float(thetas[k]), float(sh[k]), float(al[k]), d, outfile='eval_mfg_round2/own.csv')
        np.testing.assert_allclose(res[k], own, rtol=1e-12, atol=1e-15)
    _same_lines(lines[1:], _csv('eval_mfg_round2/own.csv'))
    # the Philox step moved as each learner's own: the next training gives the same bits
    pop.train(E, first_episode=E)
    for k, lk in enumerate(learners):
        lk.train(E, first_episode=E)
        assert float(np.ravel(pop.thetas[k])[0]) == float(np.ravel(lk.theta)[0]), k
        assert np.array_equal(pop.w[k], np.ravel(lk.w)), k


def test_ac_irl_population_evaluate_equals_learners(dev, tmp_path, monkeypatch):
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
    learners = [pop.learner(k) for k in range(K)]
    thetas = pop.thetas
    res = pop.evaluate(outfile='eval_mfg_round2/pop.csv')
    for k, lk in enumerate(learners):
        own = lk.evaluate(float(thetas[k]), float(sh[k]), float(al[k]), d, outfile='eval_mfg_round2/own.csv')
        np.testing.assert_allclose(res[k], own, rtol=1e-12, atol=1e-15)
    _same_lines(_csv('eval_mfg_round2/pop.csv'), _csv('eval_mfg_round2/own.csv'))
    assert pop._rng_step == learners[0]._rng_step


def _fresh_point(theta, shift, alpha, d, seed, outfile):
    from discrete_mean_field_game_amd.mfg_ac2 import actor_critic
    state = np.random.get_state()
    ac = actor_critic(theta, shift, alpha, d, pi0=np.full((1, d), 1.0 / d), seed=seed, verbose=0)
    np.random.set_state(state)
    return ac.evaluate(theta, shift, alpha, d, outfile=outfile)


def test_gridsearch_equals_fresh_evaluations(dev, tmp_path, monkeypatch):
    from discrete_mean_field_game_amd import population
    monkeypatch.chdir(tmp_path)
    d, seed = 21, 12345
    _write_files(d, 13)
    thetas, shifts, alphas = [6.0, 8.5, 11.0], [0.15, 0.45], [7000.0, 13000.0]
    best = population.gridsearch(thetas, shifts, alphas, 'test_normalized_round2', 'eval_mfg_round2/grid.csv', d=d, seed=seed)
    lines = _csv('eval_mfg_round2/grid.csv')
    assert len(lines) == 12
    pts = [(t, s, a) for t in thetas for s in shifts for a in alphas]
    vals = []
    for (t, s, a), line in zip(pts, lines):
        assert line[:3] == [('%f' % v) for v in (t, s, a)]
        vals.append(_fresh_point(t, s, a, d, seed, 'eval_mfg_round2/fresh.csv'))
    _same_lines(lines, _csv('eval_mfg_round2/fresh.csv'))
    vals = np.array(vals)
    for idx in range(4):
        p = int(np.argmin(vals[:, idx]))
        assert sorted(vals[:, idx])[0] < sorted(vals[:, idx])[1] * (1 - 1e-9)     # no near-tie on this grid
        assert best[idx][1:] == list(pts[p]), idx
        np.testing.assert_allclose(best[idx][0], vals[p, idx], rtol=1e-12)
    # chunked: the same numbers, bit for bit
    monkeypatch.setattr(population, 'GRID_CHUNK', 5)
    best5 = population.gridsearch(thetas, shifts, alphas, 'test_normalized_round2', 'eval_mfg_round2/grid5.csv', d=d, seed=seed)
    assert best5 == best
    assert _csv('eval_mfg_round2/grid5.csv') == lines


def test_gridsearch_mixed_range(dev, tmp_path, monkeypatch):
    from discrete_mean_field_game_amd import _lib, ops, population
    monkeypatch.chdir(tmp_path)
    _write_files(21, 14)
    ops.clear_status()
    grid = ([8.0, 150.0], [0.5], [1e4])          # 150 (1/2 + 0.5) > 86: beyond mixed precision's fp32 range
    with pytest.raises(_lib.MfgError):
        population.gridsearch(*grid, 'test_normalized_round2', 'eval_mfg_round2/mixed.csv')
    assert not os.path.exists('eval_mfg_round2/mixed.csv')
    best = population.gridsearch(*grid, 'test_normalized_round2', 'eval_mfg_round2/f64.csv', precision='f64')
    assert len(_csv('eval_mfg_round2/f64.csv')) == 2 and all(np.isfinite(b[0]) for b in best)
    assert ops.status(synchronize=True) == 0
