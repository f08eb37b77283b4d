"""AC_IRLPopulation / mfg_train_*_irl_pop on the GPU: learner k of a population gives, bit for bit (torch.equal), what the
single-learner native IRL calls give with learner k's settings and reward network (step mode: mfg_train_episode_irl_draw per
episode; rollout mode: mfg_train_rollout_irl with the in-kernel start draw and MFG_TRAIN_APPLY), in theta, w, G, the returns,
the final states and the last step's P / reward / delta / g; learners are independent; split calls equal one call; the class's
learner(k) equals AC_IRL.train(stop_criteria=-1); one case is pinned to the fp64 oracle replay."""
import numpy as np
import pytest

torch = pytest.importorskip('torch')

pytestmark = pytest.mark.gpu
T = 15


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.fail('-m gpu tests need a GPU')
    return torch.device('cuda:0')


def _nets(d, n3, keep, count, seed0, dev):
    from discrete_mean_field_game_amd.networks import RewardNet
    out = []
    for j in range(count):
        torch.manual_seed(seed0 + j)
        net = RewardNet(d=d, n_fc3=n3, n_fc4=4, keep_prob=keep).to(dev)
        with torch.no_grad():          # non-zero biases: every tensor of the network matters
            for p in net.parameters():
                if p.dim() == 1:
                    p.uniform_(-0.2, 0.2)
        out.append(net)
    return out


def _table(d, seed=3):
    return np.random.RandomState(seed).dirichlet(np.ones(d), size=9)


def _population(mode, d, K, B, precision, nets, seeds, thetas, shifts, alphas, w0, dev):
    from discrete_mean_field_game_amd.irl_population import AC_IRLPopulation
    return AC_IRLPopulation(thetas, shifts, alphas, d, batch=B, reward_nets=nets if len(nets) > 1 else nets[0], seeds=seeds,
                            w0=w0, pi0=_table(d), update_every=mode, precision=precision, device=dev)


def _single(mode, d, B, precision, net, seed, theta, shift, alpha, w0, E, gamma, constant, lrc, lra, first_episode, dev, T=T):
    """Learner outputs from the single-learner native IRL calls, as AC_IRL.train issues them (T env steps per episode)."""
    from discrete_mean_field_game_amd import ops
    from discrete_mean_field_game_amd.parallel import lr_scales
    F = ops.num_features(d)
    mat = torch.as_tensor(np.ascontiguousarray(_table(d), dtype=np.float32), device=dev)
    th = torch.tensor([theta], dtype=torch.float64, device=dev)
    w = torch.as_tensor(np.ascontiguousarray(w0, dtype=np.float64), device=dev).clone()
    G = torch.zeros(F + 3, dtype=torch.float64, device=dev)
    acc = torch.zeros(E, dtype=torch.float64, device=dev)
    out = {}
    if mode == 'step':
        ws = ops.workspace(B, d, dev)
        bufs = dict(ops.episode_buffers(B, d, dev), P=torch.empty(B, 1, d, d, dtype=torch.float32, device=dev))
        pi = torch.empty(B, d, dtype=torch.float32, device=dev)
        for e in range(E):
            sc, sa = lr_scales(first_episode + 1 + e, constant)
            ops.train_episode_irl(pi, T, th, shift, alpha, w, gamma, lrc * sc, lra * sa, net, G, ws, bufs, seed=seed,
                                  first_step=e * T, rn_seed=seed + 0x5EED, rn_call0=e * T, rn_sample_offset=0,
                                  reward_acc=acc[e:e + 1], precision=precision, mat_pi0=mat)
        out.update(pi=pi, P=bufs['P'].view(B, d, d), reward=bufs['reward'], delta=bufs['delta'], g=bufs['g'])
    else:
        ws = ops.workspace(B * T, d, dev)
        bufs = {'pi_traj': torch.empty(B, T + 1, d, dtype=torch.float32, device=dev),
                'pi_last': torch.empty(B, d, dtype=torch.float32, device=dev),
                'P': torch.empty(B, T, d, d, dtype=torch.float32, device=dev),
                'reward': torch.empty(B * T, dtype=torch.float32, device=dev),
                'delta': torch.empty(B, T, dtype=torch.float64, device=dev),
                'g': torch.empty(B, T, dtype=torch.float64, device=dev)}
        for e in range(E):
            sc, sa = lr_scales(first_episode + 1 + e, constant)
            key = ((seed + 0x5EED) ^ ((e + 1) * 0x9E3779B97F4A7C15)) & 0xFFFFFFFFFFFFFFFF
            ops.train_rollout_irl(mat, None, T, th, shift, alpha, w, gamma, lrc * sc, lra * sa, net, G, ws, bufs, seed=seed,
                                  first_step=e * T, rn_key=key, rn_sample_offset=0, reward_acc=acc[e:e + 1],
                                  precision=precision)
        out.update(pi=bufs['pi_last'], pi_traj=bufs['pi_traj'], P=bufs['P'], reward=bufs['reward'].view(B, T),
                   delta=bufs['delta'], g=bufs['g'])
    out.update(theta=th, w=w, G=G, acc=acc * T if mode == 'rollout' else acc)
    return out


def _pop_outputs(pop, k):
    b = pop._bufs
    r = b['run']
    out = dict(theta=pop._theta[k:k + 1], w=pop._w[k], G=b['G'][k], P=r['P'][k], reward=r['reward'][k], delta=r['delta'][k],
               g=r['g'][k])
    if pop.update_every == 'step':
        out['pi'] = b['pi'][k]
    else:
        out['pi'] = r['pi_last'][k]
        out['pi_traj'] = r['pi_traj'][k]
    return out


def _settings(K, d):
    rs = np.random.RandomState(100 + K + d)
    thetas = 8.64 + 0.4 * rs.randn(K)
    shifts = 0.05 * rs.rand(K)
    alphas = 1e4 * (0.8 + 0.4 * rs.rand(K))
    seeds = [11 + 7 * k for k in range(K)]
    if K >= 3:
        seeds[2] = seeds[0]                      # two learners sharing a seed (they still differ: theta, net, ...)
    return thetas, shifts, alphas, seeds


# (mode, d, precision, per-learner nets, keep_prob, n_fc3, K, Bk, episodes, constant, first_episode)
CASES = [
    ('step', 21, 'mixed', True, 0.4, 8, 3, 1000, 2, 0, 0),
    ('rollout', 21, 'mixed', False, 0.4, 8, 3, 1000, 2, 1, 2),
    ('step', 15, 'f64', False, 1.0, 16, 1, 64, 2, 0, 3),
    ('rollout', 15, 'f64', True, 1.0, 16, 3, 64, 2, 0, 0),
    ('step', 15, 'mixed', True, 0.4, 8, 3, 1000, 1, 1, 5),
    ('rollout', 21, 'f64', False, 1.0, 16, 1, 1000, 1, 0, 1),
    ('step', 21, 'mixed', True, 0.4, 16, 16, 4096, 1, 0, 0),
    ('rollout', 21, 'mixed', True, 0.4, 8, 16, 4096, 1, 0, 0),
]


@pytest.mark.parametrize('case', CASES, ids=['-'.join(map(str, c)) for c in CASES])
def test_population_equals_single_learner_calls(dev, case):
    mode, d, precision, per, keep, n3, K, B, E, constant, fe = case
    from discrete_mean_field_game_amd import ops
    thetas, shifts, alphas, seeds = _settings(K, d)
    nets = _nets(d, n3, keep, K if per else 1, 40 + d, dev)
    np.random.seed(5)
    w0 = np.stack([np.random.randn(ops.num_features(d)) * 0.1 for _ in range(K)])
    lrc = [0.1 * (1 + 0.5 * k) for k in range(K)]
    lra = [0.001 * (1 + 0.25 * k) for k in range(K)]
    gamma = 0.9
    pop = _population(mode, d, K, B, precision, nets, seeds, thetas, shifts, alphas, w0, dev)
    ret = pop.train(E, gamma, constant, lrc, lra, first_episode=fe)
    torch.cuda.synchronize()
    for k in range(K):
        ref = _single(mode, d, B, precision, nets[k if per else 0], seeds[k], thetas[k], shifts[k], alphas[k], w0[k], E, gamma,
                      constant, lrc[k], lra[k], fe, dev)
        got = _pop_outputs(pop, k)
        for key, v in got.items():
            assert torch.equal(v, ref[key].view(v.shape)), (k, key)
        assert np.array_equal(ret[k], ref['acc'].cpu().numpy()), k


@pytest.mark.parametrize('mode', ['step', 'rollout'])
def test_even_T_population_equals_single_learner_calls(dev, mode):
    """The native population calls at an even number of env steps per episode (the class fixes T = 15): the step flow's buffer
    alternation and theta slots depend on the parity of T."""
    from discrete_mean_field_game_amd import ops
    Te, d, K, B, E, gamma, fe = 4, 21, 3, 1000, 2, 0.9, 0
    thetas, shifts, alphas, seeds = _settings(K, d)
    nets = _nets(d, 8, 0.4, K, 40 + d, dev)
    np.random.seed(5)
    F = ops.num_features(d)
    w0 = np.stack([np.random.randn(F) * 0.1 for _ in range(K)])
    lrc = [0.1 * (1 + 0.5 * k) for k in range(K)]
    lra = [0.001 * (1 + 0.25 * k) for k in range(K)]
    pop = _population(mode, d, K, B, 'mixed', nets, seeds, thetas, shifts, alphas, w0, dev)
    f32, f64 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.float64, device=dev)
    G = torch.zeros(K, F + 3, **f64)
    ws = torch.zeros(K, ops.pop_workspace_slice(B, d, Te) // 8, **f64)
    acc = torch.zeros(K, E, **f64)
    n = (K, B) if mode == 'step' else (K, B, Te)
    bufs = dict(P=torch.empty(*n, d, d, **f32), reward=torch.empty(*n, **f32), delta=torch.empty(*n, **f64),
                g=torch.empty(*n, **f64))
    args = (pop._theta, pop._shifts_dev, pop._alphas_dev, pop._w, gamma, torch.tensor(lrc, **f64), torch.tensor(lra, **f64),
            pop._seeds_dev, pop._net_struct, True, pop._rn_seeds_dev, torch.zeros(K, dtype=torch.int64, device=dev), G, ws, bufs)
    if mode == 'step':
        pi = torch.empty(K, B, d, **f32)
        bufs['scratch'] = torch.empty(K, B, d, **f32)
        ops.train_episodes_irl_pop(pop._mat_pi0_dev, pi, Te, E, fe + 1, 0, *args, reward_acc=acc, net_stride=pop._net_stride)
    else:
        bufs.update(pi_traj=torch.empty(K, B, Te + 1, d, **f32), pi_last=torch.empty(K, B, d, **f32))
        ops.train_rollouts_irl_pop(pop._mat_pi0_dev, Te, E, fe + 1, 0, *args, reward_acc=acc, net_stride=pop._net_stride)
        pi = bufs['pi_last']
    torch.cuda.synchronize()
    for k in range(K):
        ref = _single(mode, d, B, 'mixed', nets[k], seeds[k], thetas[k], shifts[k], alphas[k], w0[k], E, gamma, 0, lrc[k], lra[k],
                      fe, dev, T=Te)
        got = dict(theta=pop._theta[k:k + 1], w=pop._w[k], G=G[k], pi=pi[k], P=bufs['P'][k], reward=bufs['reward'][k],
                   delta=bufs['delta'][k], g=bufs['g'][k], acc=acc[k] * Te if mode == 'rollout' else acc[k])
        if mode == 'rollout':
            got['pi_traj'] = bufs['pi_traj'][k]
        for key, v in got.items():
            assert torch.equal(v, ref[key].view(v.shape)), (k, key)


@pytest.mark.parametrize('mode', ['step', 'rollout'])
def test_int_counter_equals_counter_array(dev, mode):
    """rn_call0 as an int is rn_call0 as K equal per-learner counters, bit for bit -- with per-learner networks in flat rows
    (net_stride > 0).  Bk = 40 is not a multiple of the reward-network launch's 16-sample groups."""
    from discrete_mean_field_game_amd import ops
    Te, d, K, B, E, gamma = 3, 15, 3, 40, 2, 0.9
    thetas, shifts, alphas, seeds = _settings(K, d)
    np.random.seed(5)
    F = ops.num_features(d)
    w0 = np.stack([np.random.randn(F) * 0.1 for _ in range(K)])
    f32, f64 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.float64, device=dev)

    def run(rn_call0):
        pop = _population(mode, d, K, B, 'mixed', _nets(d, 8, 0.4, K, 40 + d, dev), seeds, thetas, shifts, alphas, w0, dev)
        assert pop._net_stride > 0
        G = torch.zeros(K, F + 3, **f64)
        ws = torch.zeros(K, ops.pop_workspace_slice(B, d, Te) // 8, **f64)
        acc = torch.zeros(K, E, **f64)
        n = (K, B) if mode == 'step' else (K, B, Te)
        bufs = dict(P=torch.empty(*n, d, d, **f32), reward=torch.empty(*n, **f32), delta=torch.empty(*n, **f64),
                    g=torch.empty(*n, **f64))
        args = (pop._theta, pop._shifts_dev, pop._alphas_dev, pop._w, gamma, torch.full((K,), 0.1, **f64),
                torch.full((K,), 0.001, **f64), pop._seeds_dev, pop._net_struct, True, pop._rn_seeds_dev, rn_call0, G, ws, bufs)
        if mode == 'step':
            pi = torch.empty(K, B, d, **f32)
            bufs['scratch'] = torch.empty(K, B, d, **f32)
            ops.train_episodes_irl_pop(pop._mat_pi0_dev, pi, Te, E, 1, 0, *args, reward_acc=acc, net_stride=pop._net_stride)
        else:
            bufs.update(pi_traj=torch.empty(K, B, Te + 1, d, **f32), pi_last=torch.empty(K, B, d, **f32))
            ops.train_rollouts_irl_pop(pop._mat_pi0_dev, Te, E, 1, 0, *args, reward_acc=acc, net_stride=pop._net_stride)
            pi = bufs['pi_last']
        torch.cuda.synchronize()
        return dict(theta=pop._theta, w=pop._w, G=G, acc=acc, pi=pi, P=bufs['P'], reward=bufs['reward'], delta=bufs['delta'],
                    g=bufs['g'])
    a = run(7)
    b = run(torch.full((K,), 7, dtype=torch.int64, device=dev))
    for key in a:
        assert torch.equal(a[key], b[key]), key
    assert bool(a['acc'].abs().sum() > 0) and bool(torch.isfinite(a['theta']).all())


@pytest.mark.parametrize('Tn', [3, 4])
def test_given_start_states_equal_drawn_ones(dev, Tn):
    """mfg_train_episode_irl on given start states (final states copied back into `pi` after an odd number of steps) against
    mfg_train_episode_irl_draw, which draws the same states in its first step kernel and alternates its buffers instead."""
    from discrete_mean_field_game_amd import ops
    d, B, seed, step0, gamma = 21, 1000, 11, 30, 0.9
    net = _nets(d, 8, 0.4, 1, 61, dev)[0]
    mat = torch.as_tensor(np.ascontiguousarray(_table(d), dtype=np.float32), device=dev)
    F = ops.num_features(d)
    np.random.seed(6)
    w0 = torch.as_tensor(np.random.randn(F) * 0.1, device=dev)
    outs = []
    for drawn in (True, False):
        th = torch.tensor([8.64], dtype=torch.float64, device=dev)
        w = w0.clone()
        G = torch.zeros(F + 3, dtype=torch.float64, device=dev)
        acc = torch.zeros(1, dtype=torch.float64, device=dev)
        ws = ops.workspace(B, d, dev)
        bufs = dict(ops.episode_buffers(B, d, dev), P=torch.empty(B, 1, d, d, dtype=torch.float32, device=dev))
        pi = torch.empty(B, d, dtype=torch.float32, device=dev) if drawn else ops.draw_start(mat, B, seed, step0)[1]
        ops.train_episode_irl(pi, Tn, th, 0.02, 1e4, w, gamma, 0.1, 0.001, net, G, ws, bufs, seed=seed, first_step=step0,
                              rn_seed=seed + 0x5EED, rn_call0=7, rn_sample_offset=0, reward_acc=acc, precision='mixed',
                              mat_pi0=mat if drawn else None)
        torch.cuda.synchronize()
        outs.append(dict(pi=pi, theta=th, w=w, G=G, acc=acc, P=bufs['P'], reward=bufs['reward'], delta=bufs['delta'], g=bufs['g']))
    for key, v in outs[0].items():
        assert torch.equal(v, outs[1][key]), key
    assert float(outs[0]['theta']) != 8.64 and not torch.equal(outs[0]['w'], w0)


@pytest.mark.parametrize('mode', ['step', 'rollout'])
def test_learners_are_independent(dev, mode):
    from discrete_mean_field_game_amd import ops
    d, K, B = 21, 3, 256
    thetas, shifts, alphas, seeds = _settings(K, d)
    w0 = np.full((K, ops.num_features(d)), 0.01)
    a = _population(mode, d, K, B, 'mixed', _nets(d, 8, 0.4, K, 7, dev), seeds, thetas, shifts, alphas, w0, dev)
    ra = a.train(2, 0.9)
    nets = _nets(d, 8, 0.4, K, 7, dev)
    nets[1] = _nets(d, 8, 0.4, 1, 99, dev)[0]          # another network and theta for learner 1
    th = thetas.copy()
    th[1] += 0.5
    b = _population(mode, d, K, B, 'mixed', nets, seeds, th, shifts, alphas, w0, dev)
    rb = b.train(2, 0.9)
    for k in (0, 2):
        oa, ob = _pop_outputs(a, k), _pop_outputs(b, k)
        for key in oa:
            assert torch.equal(oa[key], ob[key]), (k, key)
        assert np.array_equal(ra[k], rb[k])
    assert not torch.equal(_pop_outputs(a, 1)['w'], _pop_outputs(b, 1)['w'])


@pytest.mark.parametrize('mode', ['step', 'rollout'])
def test_split_calls_equal_one_call(dev, mode):
    from discrete_mean_field_game_amd import ops
    d, K, B = 15, 3, 200
    thetas, shifts, alphas, seeds = _settings(K, d)
    w0 = np.full((K, ops.num_features(d)), 0.02)
    nets = _nets(d, 8, 0.4, K, 21, dev)
    a = _population(mode, d, K, B, 'mixed', nets, seeds, thetas, shifts, alphas, w0, dev)
    r1 = a.train(1, 0.9, first_episode=0)
    r2 = a.train(2, 0.9, first_episode=1)
    b = _population(mode, d, K, B, 'mixed', nets, seeds, thetas, shifts, alphas, w0, dev)
    r = b.train(3, 0.9)
    assert np.array_equal(np.concatenate([r1, r2], axis=1), r)
    oa, ob = _pop_outputs(a, 0), _pop_outputs(b, 0)
    for k in range(K):
        oa, ob = _pop_outputs(a, k), _pop_outputs(b, k)
        for key in oa:
            assert torch.equal(oa[key], ob[key]), (k, key)
    assert a._rng_step == b._rng_step and a._reward_calls == b._reward_calls


@pytest.mark.parametrize('mode', ['step', 'rollout'])
def test_learner_equals_ac_irl_train(dev, mode):
    from discrete_mean_field_game_amd.ac_irl import AC_IRL
    d, K, B, E = 21, 3, 128, 2
    thetas, shifts, alphas, seeds = _settings(K, d)
    nets = _nets(d, 8, 0.4, K, 60, dev)
    np.random.seed(9)
    pop = _population(mode, d, K, B, 'mixed', nets, seeds, thetas, shifts, alphas, None, dev)
    w0 = pop.w
    pop.train(E, 0.9, False, 0.1, 0.001)
    for k in range(K):
        ac = AC_IRL(float(thetas[k]), float(shifts[k]), float(alphas[k]), d, pi0=_table(d), demonstrations=[], batch=B,
                    seed=seeds[k], update_every=mode, precision='mixed', device=dev, verbose=0)
        ac.reward_net = pop.reward_net(k)
        ac.create_training_method()
        ac.w = w0[k]
        ac.train(max_episodes=E, stop_criteria=-1, gamma=0.9, constant=False, lr_critic=0.1, lr_actor=0.001)
        lk = pop.learner(k)
        assert float(np.ravel(lk.theta)[0]) == float(np.ravel(ac.theta)[0]), k
        assert np.array_equal(np.asarray(lk.w), np.asarray(ac.w)), k
        assert lk._rng_step == ac._rng_step and lk._reward_calls == ac._reward_calls
        for (n1, p1), (n2, p2) in zip(lk.reward_net.named_parameters(), ac.reward_net.named_parameters()):
            assert n1 == n2 and torch.equal(p1, p2)


def test_learner_leaves_np_random_alone(dev):
    d = 15
    thetas, shifts, alphas, seeds = _settings(2, d)
    pop = _population('step', d, 2, 64, 'mixed', _nets(d, 8, 0.4, 1, 3, dev), seeds, thetas, shifts, alphas, None, dev)
    np.random.seed(1234)
    before = np.random.get_state()[1].copy()
    pop.learner(1)
    assert np.array_equal(np.random.get_state()[1], before)


def test_population_learner_matches_oracle_replay(dev):
    """One learner of a step-mode population replayed by the fp64 oracle on its sampled actions (the reward network
    evaluated by its PyTorch module, keep_prob 1): the new kernels are pinned to the oracle, not only to themselves."""
    from discrete_mean_field_game_amd import ops
    from oracle import mfg_oracle as O
    from oracle.philox_ref import start_indices
    d, K, B, gamma, k = 15, 2, 10, 0.9, 1
    thetas, shifts, alphas = np.array([8.0, 8.64]), np.array([0.0, 0.0]), np.array([1e4, 1e4])
    seeds = [5, 13]
    nets = _nets(d, 8, 1.0, K, 77, dev)
    np.random.seed(31)
    w0 = np.stack([np.random.randn(ops.num_features(d)) * 0.05 for _ in range(K)])
    pop = _population('step', d, K, B, 'f64', nets, seeds, thetas, shifts, alphas, w0, dev)
    pop.train(1, gamma, False, 0.1, 0.001)
    mat = _table(d)
    pi = mat[start_indices(seeds[k], 0, np.arange(B), mat.shape[0])].astype(np.float32)
    w, theta = w0[k].copy(), float(thetas[k])
    sc, sa = O.lr_scales(1, False)
    disc = 1.0
    for t in range(T):
        th = torch.tensor([theta], dtype=torch.float64, device=dev)
        P = ops.sample_dirichlet(torch.as_tensor(pi, device=dev), th, 0.0, 1e4, seed=seeds[k], step=t, precision='f64')
        pn = O.transition(P.cpu().numpy(), pi).astype(np.float32)
        with torch.no_grad():
            r = nets[k](torch.as_tensor(pi, device=dev), P).reshape(-1).double().cpu().numpy()
        _, _, G_w, G_t, _ = O.batched_td_pg(pi, pn, P.cpu().numpy(), r, w, theta, 0.0, disc)
        w = w + 0.1 * sc * G_w / B
        theta = theta + 0.001 * sa * G_t / B
        disc *= gamma
        pi = pn
    assert abs(float(pop.thetas[k]) - theta) < 1e-7
    assert np.max(np.abs(pop.w[k] - w)) < 1e-6
    assert np.max(np.abs(pop._bufs['pi'][k].cpu().numpy() - pi)) < 1e-6


def _raw_call(pop, net_struct=None, ws=None, per=None):
    b = pop._buffers()
    from discrete_mean_field_game_amd import ops
    K = pop.K
    lr = torch.full((K,), 0.1, dtype=torch.float64, device=pop.device)
    ops.train_episodes_irl_pop(pop._mat_pi0_dev, b['pi'], T, 1, 1, 0, pop._theta, pop._shifts_dev, pop._alphas_dev, pop._w,
                               0.9, lr, lr, pop._seeds_dev, net_struct or pop._net_struct,
                               pop.per_learner_net if per is None else per, pop._rn_seeds_dev, 0, b['G'],
                               b['ws'] if ws is None else ws, b['run'])


def _struct_copy(st):
    from discrete_mean_field_game_amd import _lib as L
    out = L.RewardNetStruct()
    for name, _ in L.RewardNetStruct._fields_:
        setattr(out, name, getattr(st, name))
    return out


def test_refusals_before_any_launch(dev):
    from discrete_mean_field_game_amd import _lib as L
    d, K = 21, 2
    thetas, shifts, alphas, seeds = _settings(K, d)
    pop = _population('step', d, K, 64, 'mixed', _nets(d, 8, 0.4, K, 5, dev), seeds, thetas, shifts, alphas, None, dev)
    theta0, w0 = pop.thetas, pop.w
    # misaligned fc3 weights of learner 1 (per-learner stride moved by 4 bytes): not the matrix-core kernel
    st = _struct_copy(pop._net_struct)
    st.fc3_w = pop._net_struct.fc3_w + 4
    with pytest.raises(L.MfgError) as e:
        _raw_call(pop, net_struct=st)
    assert e.value.code == -3
    # a geometry the matrix-core kernel does not serve (n_fc4 > 32)
    st = _struct_copy(pop._net_struct)
    st.n4 = 33
    with pytest.raises(L.MfgError) as e:
        _raw_call(pop, net_struct=st)
    assert e.value.code == -3
    # one learner's slice too small for the partial rows
    small = torch.zeros(K, 256 // 8, dtype=torch.float64, device=dev)
    with pytest.raises(L.MfgError) as e:
        _raw_call(pop, ws=small)
    assert e.value.code == -4
    torch.cuda.synchronize()
    assert np.array_equal(pop.thetas, theta0) and np.array_equal(pop.w, w0)
