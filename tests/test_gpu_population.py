"""-m gpu: a population of K independent learners (mfg_train_episodes_pop / mfg_train_rollouts_pop) gives learner k, bit for
bit in every output, what the single-learner call gives with B = Bk, that learner's seed, theta, w, shift, alpha_scale and
learning rates, and the same workspace slice (the reference trains such learners one after another: mfg_ac2.gridsearch,
mfg_ac2.py:673-689).  Every comparison is torch.equal.
"""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.fail('-m gpu tests need a GPU')
    from discrete_mean_field_game_amd import ops
    ops.init()
    return torch.device('cuda', 0)


def _L():
    from discrete_mean_field_game_amd import _lib
    return _lib


def _slice_bytes(N, d):
    n = int(_L().lib().mfg_workspace_bytes(N, d))
    return (max(n, 8) + 255) // 256 * 256


def _setup(dev, d, K, Bk, T, seed):
    rs = np.random.RandomState(seed)
    F = d * (d + 1) // 2 + d + 1
    mat = torch.as_tensor(rs.dirichlet(np.ones(d), size=64).astype(np.float32), device=dev)
    p = dict(theta=rs.uniform(6.5, 9.9, K), shift=rs.uniform(0.1, 0.2, K), alpha=rs.uniform(8000.0, 14000.0, K),
             lrc=rs.uniform(0.05, 0.15, K), lra=rs.uniform(5e-4, 2e-3, K), seed=rs.randint(0, 2 ** 40, K).astype(np.int64),
             w=rs.rand(K, F) * 0.1)
    if K > 1:
        p['seed'][1] = p['seed'][0]  # two learners share a seed
    return mat, p, F


def _t(x, dev, dtype=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=dtype, device=dev)


def _run_pop(dev, mode, mat, p, d, K, Bk, T, E, F, precision, kind, constant):
    from discrete_mean_field_game_amd import ops
    sb = _slice_bytes(Bk * T, d)
    theta, w = _t(p['theta'], dev), _t(p['w'], dev)
    G = torch.zeros(K, F + 3, dtype=torch.float64, device=dev)
    ws = torch.zeros(K, sb // 8, dtype=torch.float64, device=dev)
    acc = torch.zeros(K, E, dtype=torch.float64, device=dev)
    sc = dict(shifts=_t(p['shift'], dev), alpha_scales=_t(p['alpha'], dev), lr_critic=_t(p['lrc'], dev),
              lr_actor=_t(p['lra'], dev), seeds=_t(p['seed'], dev, torch.int64))
    if mode == 'step':
        pi = torch.zeros(K, Bk, d, dtype=torch.float32, device=dev)
        bufs = dict(scratch=torch.zeros_like(pi), reward=torch.zeros(K, Bk, dtype=torch.float32, device=dev),
                    delta=torch.zeros(K, Bk, dtype=torch.float64, device=dev), g=torch.zeros(K, Bk, dtype=torch.float64, device=dev))
        ops.train_episodes_pop(mat, pi, T, E, 0, constant, theta, sc['shifts'], sc['alpha_scales'], w, 1.0, sc['lr_critic'],
                               sc['lr_actor'], sc['seeds'], G, ws, bufs, reward_kind=kind, reward_acc=acc, precision=precision)
        out = dict(pi=pi, reward=bufs['reward'], delta=bufs['delta'], g=bufs['g'])
    else:
        bufs = dict(pi_traj=torch.zeros(K, Bk, T + 1, d, dtype=torch.float32, device=dev),
                    pi_last=torch.zeros(K, Bk, d, dtype=torch.float32, device=dev),
                    reward=torch.zeros(K, Bk, T, dtype=torch.float32, device=dev),
                    delta=torch.zeros(K, Bk, T, dtype=torch.float64, device=dev),
                    g=torch.zeros(K, Bk, T, dtype=torch.float64, device=dev))
        ops.train_rollouts_pop(mat, T, E, 0, constant, theta, sc['shifts'], sc['alpha_scales'], w, 1.0, G, ws, bufs,
                               sc['lr_critic'], sc['lr_actor'], sc['seeds'], reward_kind=kind, reward_acc=acc, precision=precision)
        out = dict(bufs)
    out.update(theta=theta, w=w, G=G, acc=acc)
    return out, sb


def _run_single(dev, mode, mat, p, k, d, Bk, T, E, F, precision, kind, constant, sb):
    from discrete_mean_field_game_amd import ops
    theta, w = _t(p['theta'][k:k + 1], dev), _t(p['w'][k], dev)
    G = torch.zeros(F + 3, dtype=torch.float64, device=dev)
    ws = torch.zeros(sb // 8, dtype=torch.float64, device=dev)
    acc = torch.zeros(E, dtype=torch.float64, device=dev)
    args = dict(reward_kind=kind, seed=int(p['seed'][k]) & (2 ** 64 - 1), reward_acc=acc, precision=precision)
    if mode == 'step':
        pi = torch.zeros(Bk, d, dtype=torch.float32, device=dev)
        bufs = dict(scratch=torch.zeros_like(pi), reward=torch.zeros(Bk, dtype=torch.float32, device=dev),
                    delta=torch.zeros(Bk, dtype=torch.float64, device=dev), g=torch.zeros(Bk, dtype=torch.float64, device=dev))
        ops.train_episodes(mat, pi, T, E, 0, constant, theta, float(p['shift'][k]), float(p['alpha'][k]), w, 1.0,
                           float(p['lrc'][k]), float(p['lra'][k]), G, ws, bufs, **args)
        out = dict(pi=pi, reward=bufs['reward'], delta=bufs['delta'], g=bufs['g'])
    else:
        bufs = dict(pi_traj=torch.zeros(Bk, T + 1, d, dtype=torch.float32, device=dev),
                    pi_last=torch.zeros(Bk, d, dtype=torch.float32, device=dev),
                    reward=torch.zeros(Bk, T, dtype=torch.float32, device=dev),
                    delta=torch.zeros(Bk, T, dtype=torch.float64, device=dev), g=torch.zeros(Bk, T, dtype=torch.float64, device=dev))
        ops.train_rollouts(mat, T, E, 0, constant, theta, float(p['shift'][k]), float(p['alpha'][k]), w, 1.0, G, ws, bufs,
                           float(p['lrc'][k]), float(p['lra'][k]), **args)
        out = dict(bufs)
    out.update(theta=theta[0], w=w, G=G, acc=acc)
    return out


def _check(dev, mode, d, K, Bk, precision='mixed', kind=0, constant=0, E=3, T=15, seed=0):
    mat, p, F = _setup(dev, d, K, Bk, T, seed + 1000 * d + 10 * K + Bk)
    pop, sb = _run_pop(dev, mode, mat, p, d, K, Bk, T, E, F, precision, kind, constant)
    for k in range(K):
        one = _run_single(dev, mode, mat, p, k, d, Bk, T, E, F, precision, kind, constant, sb)
        for key, ref in one.items():
            assert torch.equal(pop[key][k], ref), 'learner %d: %s differs (%s d=%d K=%d Bk=%d %s kind=%d)' % (
                k, key, mode, d, K, Bk, precision, kind)
    return pop, p


# d = 40: the gradient kernel k_grad_partial; d = 64: the matrix-core k_grad_mfma (one trajectory per wave in the core kernel)
GRID = [(21, 1, 1), (21, 3, 13), (21, 8, 1024), (21, 3, 4096), (15, 3, 1), (15, 8, 13), (15, 3, 1024), (40, 3, 13),
        (40, 8, 1024), (64, 3, 13), (64, 2, 1024)]


@pytest.mark.parametrize('mode', ['step', 'rollout'])
@pytest.mark.parametrize('d,K,Bk', GRID)
def test_population_matches_single(dev, mode, d, K, Bk):
    _check(dev, mode, d, K, Bk, constant=(Bk % 2))


@pytest.mark.parametrize('mode', ['step', 'rollout'])
@pytest.mark.parametrize('d,K,Bk,precision,kind', [(21, 3, 1024, 'f64', 0), (15, 3, 13, 'f64', 1), (21, 3, 1024, 'mixed', 1),
                                                   (40, 3, 13, 'mixed', 1)])
def test_population_precision_and_reward(dev, mode, d, K, Bk, precision, kind):
    _check(dev, mode, d, K, Bk, precision=precision, kind=kind)


@pytest.mark.parametrize('Bk', [6144, 6145, 8256])
def test_population_sums_paths(dev, Bk):
    # 6 144 trajectories at d = 21 = MFG_CORE_SUMS_MAX_ROWS tiles (the SUMS core variant); 6 145 the gradient kernel with its
    # in-kernel finish; 8 256: 33 gradient rows > MFG_GRAD_FUSE_MAX_ROWS (the separate row reduction)
    _check(dev, 'step', 21, 2, Bk, E=2)


def test_population_rollout_unfused(dev):
    # rollout mode at Bk = 4 096: 240 gradient rows over the B T samples > MFG_GRAD_FUSE_MAX_ROWS -> the separate row reduction
    _check(dev, 'rollout', 21, 2, 4096, E=2)


@pytest.mark.parametrize('mode', ['step', 'rollout'])
def test_population_independence(dev, mode):
    d, K, Bk, T, E = 21, 4, 256, 15, 2
    mat, p, F = _setup(dev, d, K, Bk, T, 7)
    a, _ = _run_pop(dev, mode, mat, p, d, K, Bk, T, E, F, 'mixed', 0, 0)
    q = {k: v.copy() for k, v in p.items()}
    q['theta'][2] = 9.5
    q['seed'][2] = 12345
    b, _ = _run_pop(dev, mode, mat, q, d, K, Bk, T, E, F, 'mixed', 0, 0)
    for k in range(K):
        for key in a:
            same = torch.equal(a[key][k], b[key][k])
            assert same == (k != 2), 'learner %d: %s %s' % (k, key, 'changed' if k != 2 else 'unchanged')


def test_population_errors(dev):
    from discrete_mean_field_game_amd import _lib as L
    lib = L.lib()
    d, K, Bk, T = 21, 2, 64, 15
    F = d * (d + 1) // 2 + d + 1
    f32 = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev)
    f64 = lambda *s: torch.zeros(*s, dtype=torch.float64, device=dev)
    mat = torch.full((8, d), 1.0 / d, dtype=torch.float32, device=dev)
    pi, scr, rew = f32(K, Bk, d), f32(K, Bk, d), f32(K, Bk)
    dl, g, theta, w, G = f64(K, Bk), f64(K, Bk), f64(K) + 8.0, f64(K, F), f64(K, F + 3)
    sh, al, lc, la = f64(K) + 0.16, f64(K) + 12000.0, f64(K) + 0.1, f64(K) + 1e-3
    seeds = torch.zeros(K, dtype=torch.int64, device=dev)
    sb = _slice_bytes(Bk * T, d)
    ws = f64(K, sb // 8)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(K_=K, d_=d, theta_ptr=None, wsb=sb):
        return lib.mfg_train_episodes_pop(mat.data_ptr(), 8, pi.data_ptr(), scr.data_ptr(), Bk, K_, d_, T, 1, 0, 0,
                                          theta.data_ptr() if theta_ptr is None else theta_ptr, sh.data_ptr(), al.data_ptr(),
                                          w.data_ptr(), 1.0, 0, seeds.data_ptr(), 0, 0, 1, lc.data_ptr(), la.data_ptr(),
                                          rew.data_ptr(), dl.data_ptr(), g.data_ptr(), G.data_ptr(), None, ws.data_ptr(), wsb,
                                          stream)
    before = theta.clone()
    assert call(K_=0) == -1
    assert call(d_=65) == -3
    assert call(theta_ptr=0) == -1
    assert call(wsb=256) == -4
    assert call(wsb=sb - 8) == -1  # not a multiple of 256
    torch.cuda.synchronize()
    assert torch.equal(theta, before), 'a refused call launched work'
    st = C.c_uint(0)
    assert lib.mfg_status(C.byref(st)) == 0 and st.value == 0
    assert call() == 0
    torch.cuda.synchronize()


def test_population_rollout_errors(dev):
    from discrete_mean_field_game_amd import _lib as L
    lib = L.lib()
    d, K, Bk, T = 21, 2, 64, 15
    F = d * (d + 1) // 2 + d + 1
    f32 = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev)
    f64 = lambda *s: torch.zeros(*s, dtype=torch.float64, device=dev)
    mat = torch.full((8, d), 1.0 / d, dtype=torch.float32, device=dev)
    traj, rew, dl, g = f32(K, Bk, T + 1, d), f32(K, Bk, T), f64(K, Bk, T), f64(K, Bk, T)
    theta, w, G = f64(K) + 8.0, f64(K, F), f64(K, F + 3)
    sh, al, lc, la = f64(K) + 0.16, f64(K) + 12000.0, f64(K) + 0.1, f64(K) + 1e-3
    seeds = torch.zeros(K, dtype=torch.int64, device=dev)
    sb = _slice_bytes(Bk * T, d)
    ws = f64(K, sb // 8)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(K_=K, d_=d, traj_ptr=None, wsb=sb, kind=0):
        return lib.mfg_train_rollouts_pop(mat.data_ptr(), 8, Bk, K_, d_, T, 1, 0, 0, theta.data_ptr(), sh.data_ptr(),
                                          al.data_ptr(), w.data_ptr(), 1.0, kind, seeds.data_ptr(), 0, 0, 0, lc.data_ptr(),
                                          la.data_ptr(), traj.data_ptr() if traj_ptr is None else traj_ptr, None,
                                          rew.data_ptr(), dl.data_ptr(), g.data_ptr(), G.data_ptr(), None, ws.data_ptr(), wsb,
                                          stream)
    before = theta.clone()
    assert call(K_=0) == -1
    assert call(d_=65) == -3
    assert call(traj_ptr=0) == -1
    assert call(kind=2) == -1      # external reward: not an in-kernel reward
    # the rollout rule: partial rows of the B T samples (no SUMS rows); 256 bytes hold none of them
    assert call(wsb=256) == -4
    assert call(wsb=sb + 8) == -1  # not a multiple of 256
    torch.cuda.synchronize()
    assert torch.equal(theta, before), 'a refused call launched work'
    st = C.c_uint(0)
    assert lib.mfg_status(C.byref(st)) == 0 and st.value == 0
    assert call() == 0
    torch.cuda.synchronize()


def _ep_reward(ac, E):
    return next(iter(ac._train_bufs.values()))['ep_reward'][:E].cpu().numpy()


@pytest.mark.parametrize('mode', ['step', 'rollout'])
def test_population_class_matches_actor_critic(dev, mode):
    from discrete_mean_field_game_amd import ActorCriticPopulation
    from discrete_mean_field_game_amd.mfg_ac2 import actor_critic
    d, Bk, E = 21, 96, 3
    thetas, shifts, alphas = [6.7, 9.8, 8.2], [0.12, 0.19, 0.16], [9000.0, 13500.0, 12000.0]
    seeds, lrc, lra = [5, 5, 11], [0.1, 0.07, 0.12], [1e-3, 2e-3, 6e-4]
    rs = np.random.RandomState(3)
    table = rs.dirichlet(np.ones(d), size=40)
    w0 = rs.rand(3, d * (d + 1) // 2 + d + 1)
    pop = ActorCriticPopulation(thetas, shifts, alphas, d, batch=Bk, seeds=seeds, w0=w0, pi0=table, update_every=mode)
    r1 = pop.train(E, lr_critic=lrc, lr_actor=lra)
    r2 = pop.train(E, lr_critic=lrc, lr_actor=lra, first_episode=E)
    assert r1.shape == (3, E) and r2.shape == (3, E)
    for k in range(3):
        ac = actor_critic(thetas[k], shifts[k], alphas[k], d, pi0=table, batch=Bk, seed=seeds[k], update_every=mode,
                          verbose=0)
        ac.w = w0[k]
        ac.train(E, lr_critic=lrc[k], lr_actor=lra[k])
        e1 = _ep_reward(ac, E).copy()
        ac.train(E, lr_critic=lrc[k], lr_actor=lra[k], first_episode=E)
        e2 = _ep_reward(ac, E)
        assert np.array_equal(pop.thetas[k], ac.theta[0]), 'learner %d: theta' % k
        assert np.array_equal(pop.w[k], ac.w.reshape(-1)), 'learner %d: w' % k
        assert np.array_equal(r1[k], e1) and np.array_equal(r2[k], e2), 'learner %d: per-episode returns' % k
    # learner(k): an actor_critic at learner 1's parameters and Philox position -- training it on equals training learner 1
    one = pop.learner(1)
    assert one._rng_step == 2 * E * 15 and np.array_equal(one.w.reshape(-1), pop.w[1])
    one.train(1, lr_critic=lrc[1], lr_actor=lra[1], first_episode=2 * E)
    pop.train(1, lr_critic=lrc, lr_actor=lra, first_episode=2 * E)
    assert np.array_equal(pop.thetas[1], one.theta[0]) and np.array_equal(pop.w[1], one.w.reshape(-1))
    assert pop.status() == 0
