"""The reward half of AC_IRLPopulation on the GPU: mfg_reward_net_train_steps_pop equals K single mfg_reward_net_train_step
calls, mfg_reward_net_forward_pop equals per-learner mfg_reward_net_forward calls, and the class's update_reward /
reward_iteration / outerloop give learner k exactly (torch.equal / array_equal) what AC_IRL's methods give with learner k's
settings and the module `random` stream seeded with its host seed."""
import random
import types

import numpy as np
import pytest

torch = pytest.importorskip('torch')

pytestmark = pytest.mark.gpu
T = 15
NOT_COMPARED = ('np_random_key', 'np_random_pos', 'np_random_has_gauss', 'np_random_cached_gaussian', 'torch_rng_state',
                'torch_cuda_rng_state')


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.fail('-m gpu tests need a GPU')
    return torch.device('cuda:0')


def _nets(d, n3, reg, count, seed0, dev):
    from discrete_mean_field_game_amd.networks import RewardNet
    out = []
    for j in range(count):
        torch.manual_seed(seed0 + j)
        net = RewardNet(d=d, reg=reg, n_fc3=n3, n_fc4=4).to(dev)
        with torch.no_grad():
            for p in net.parameters():
                if p.dim() == 1:
                    p.uniform_(-0.2, 0.2)
        out.append(net)
    return out


def _table(d, seed=3):
    return np.random.RandomState(seed).dirichlet(np.ones(d), size=9)


def _demos(d, n, seed=5):
    rs = np.random.RandomState(seed)
    return [[(rs.dirichlet(np.ones(d)), rs.dirichlet(np.ones(d), size=d)) for _ in range(T)] for _ in range(n)]


def _population(d, K, nets, dev, mode='step', B=32, seeds=None, lr_reward=1e-3, demos=None, num_policies=3, host_seeds=None):
    from discrete_mean_field_game_amd.irl_population import AC_IRLPopulation
    seeds = list(range(11, 11 + K)) if seeds is None else seeds
    thetas = np.linspace(8.0, 9.0, K)
    return AC_IRLPopulation(thetas, 0.1, 1e4, d, batch=B, reward_nets=nets, seeds=seeds, pi0=_table(d), update_every=mode,
                            demonstrations=_demos(d, 7) if demos is None else demos, lr_reward=lr_reward,
                            num_policies=num_policies, host_seeds=host_seeds)


def _stores(d, K, rows, dev, seed=1, T=T):
    g = torch.Generator(device='cpu').manual_seed(seed)
    ds = torch.rand(rows, T, d, generator=g)
    da = torch.rand(rows, T, d, d, generator=g)
    gs = torch.rand(K, rows + 2, T, d, generator=g)
    ga = torch.rand(K, rows + 2, T, d, d, generator=g)
    return ds.to(dev), (da / da.sum(-1, keepdim=True)).to(dev), gs.to(dev), (ga / ga.sum(-1, keepdim=True)).to(dev)


def _compare(a, b, path=''):
    if isinstance(a, dict):
        assert set(a) == set(b), path
        for k in a:
            if k not in NOT_COMPARED:
                _compare(a[k], b[k], path + '/' + str(k))
    elif isinstance(a, torch.Tensor):
        assert torch.equal(a.cpu(), b.cpu()), path
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), path
        for i, (x, y) in enumerate(zip(a, b)):
            _compare(x, y, '%s[%d]' % (path, i))
    else:
        assert a == b, (path, a, b)


# ------------------------------------------------------------------ 1. the training steps
# batch = (n_demo, n_gen, steps): the last two leave the reference's 5 + 5 x 15 -- N = 153 is the first batch into the combine
# kernel's second round of column reads, with steps != 15; 3 + 40 x 4 has a different count in each half, more than 32 generated
# trajectories (the soft-max crosses lane 32) and N n3 = 2752 entries of c_n dz3_n, past the 2048 staged in registers
@pytest.mark.parametrize('reg,d,n3,K,U,batch', [
    pytest.param('none', 15, 8, 1, 1, (5, 5, 15), id='none-15-8-1-1'),
    pytest.param('dropout_l1l2', 21, 16, 3, 10, (5, 5, 15), id='dropout_l1l2-21-16-3-10'),
    pytest.param('dropout_l1l2', 15, 16, 16, 10, (5, 5, 15), id='dropout_l1l2-15-16-16-10'),
    pytest.param('none', 21, 8, 16, 1, (5, 5, 15), id='none-21-8-16-1'),
    pytest.param('dropout_l1l2', 21, 8, 3, 1, (5, 5, 15), id='dropout_l1l2-21-8-3-1'),
    pytest.param('none', 15, 8, 3, 2, (9, 8, 9), id='none-15-8-3-2-9x8x9'),
    pytest.param('dropout_l1l2', 15, 16, 3, 2, (3, 40, 4), id='dropout_l1l2-15-16-3-2-3x40x4')])
def test_train_steps_pop_equals_single_steps(dev, reg, d, n3, K, U, batch):
    nd, ng, T = batch
    from discrete_mean_field_game_amd import ops
    from discrete_mean_field_game_amd.reward_learning import RewardTrainer
    nets = _nets(d, n3, reg, K, 40, dev)
    trainers = [RewardTrainer(n, 1e-3 * (k + 1)) for k, n in enumerate(nets)]
    np_ = trainers[0].flat.numel()
    ld = (np_ + 63) // 64 * 64
    g = torch.Generator(device='cpu').manual_seed(K)
    flat = torch.zeros(K, ld, device=dev)
    m = torch.zeros(K, ld, device=dev)
    v = torch.zeros(K, ld, device=dev)
    for k, tr in enumerate(trainers):      # a different Adam history per learner
        tr.m.copy_((torch.rand(np_, generator=g) * 1e-3).to(dev))
        tr.v.copy_((torch.rand(np_, generator=g) * 1e-6).to(dev))
        tr.step_count = 3 * k
        flat[k, :np_] = tr.flat
        m[k, :np_] = tr.m
        v[k, :np_] = tr.v
    rows = max(9, nd, ng)
    ds, da, gs, ga = _stores(d, K, rows, dev, T=T)
    demo = types.SimpleNamespace(state=ds, action=da, steps=T)
    rs = random.Random(7)
    plan = ops.rn_train_plan(U * K)
    keep = nets[0].keep_prob if nets[0].use_dropout else 1.0
    for u in range(U):
        for k in range(K):
            e = plan[u * K + k]
            e['learner'] = k
            e['key'] = rs.getrandbits(64)
            e['lr'] = trainers[k].lr
            e['adam_step'] = trainers[k].step_count + 1 + u
            e['demo_rows'][:nd] = rs.sample(range(rows), nd)
            e['gen_rows'][:ng] = rs.sample(range(rows + 2), ng)
    stats = torch.zeros(K, 4, device=dev)
    ws = torch.empty(K * 1 << 20, dtype=torch.uint8, device=dev)
    plan_dev = torch.empty(plan.nbytes, dtype=torch.uint8, device=dev)
    ops.reward_net_train_steps_pop(flat, m, v, ld, K, trainers[0].dims, (ds, da), (gs, ga), plan, U, K, nd, ng, T, 5, keep,
                                   nets[0].use_l1l2, stats, ws, plan_dev)
    for k, tr in enumerate(trainers):
        gen = types.SimpleNamespace(state=gs[k], action=ga[k], steps=T)
        for u in range(U):
            e = plan[u * K + k]
            tr.step(demo, [int(r) for r in e['demo_rows'][:nd]], gen, [int(r) for r in e['gen_rows'][:ng]], 5, int(e['key']))
        assert torch.equal(flat[k, :np_], tr.flat), k
        assert torch.equal(m[k, :np_], tr.m) and torch.equal(v[k, :np_], tr.v), k
        assert torch.equal(stats[k], tr.stats), k
        assert np.float32(plan[k]['lr_t']) == np.float32(tr.lr * np.sqrt(1 - 0.999 ** int(plan[k]['adam_step']))
                                                         / (1 - 0.9 ** int(plan[k]['adam_step'])))


def test_train_steps_pop_subset_leaves_others_alone(dev):
    from discrete_mean_field_game_amd import ops
    from discrete_mean_field_game_amd.reward_learning import RewardTrainer
    d, K, U = 21, 4, 3
    nets = _nets(d, 8, 'dropout_l1l2', K, 70, dev)
    trainers = [RewardTrainer(n, 2e-3) for n in nets]
    np_ = trainers[0].flat.numel()
    ld = (np_ + 63) // 64 * 64
    flat = torch.zeros(K, ld, device=dev)
    for k, tr in enumerate(trainers):
        flat[k, :np_] = tr.flat
    m, v = torch.zeros_like(flat), torch.zeros_like(flat)
    stats = torch.full((K, 4), 7.0, device=dev)
    ds, da, gs, ga = _stores(d, K, 8, dev, seed=2)
    active = [3, 1]
    plan = ops.rn_train_plan(U * len(active))
    for u in range(U):
        for s, k in enumerate(active):
            e = plan[u * len(active) + s]
            e['learner'], e['key'], e['lr'], e['adam_step'] = k, 1000 * u + k, 2e-3, u + 1
            e['demo_rows'][:5] = [0, 2, 4, 6, 7]
            e['gen_rows'][:5] = [9, 1, 3, 5, 0]
    before = flat.clone()
    ops.reward_net_train_steps_pop(flat, m, v, ld, K, trainers[0].dims, (ds, da), (gs, ga), plan, U, len(active), 5, 5, T, 5, 0.4,
                                   True, stats, torch.empty(1 << 22, dtype=torch.uint8, device=dev),
                                   torch.empty(plan.nbytes, dtype=torch.uint8, device=dev))
    for k in (0, 2):
        assert torch.equal(flat[k], before[k]) and not m[k].any() and not v[k].any()
        assert torch.equal(stats[k], torch.full((4,), 7.0, device=dev))
    demo = types.SimpleNamespace(state=ds, action=da, steps=T)
    for k in active:
        tr = trainers[k]
        gen = types.SimpleNamespace(state=gs[k], action=ga[k], steps=T)
        for u in range(U):
            tr.step(demo, [0, 2, 4, 6, 7], gen, [9, 1, 3, 5, 0], 5, 1000 * u + k)
        assert torch.equal(flat[k, :np_], tr.flat) and torch.equal(m[k, :np_], tr.m) and torch.equal(stats[k], tr.stats)


# ------------------------------------------------------------------ 2. the forward
@pytest.mark.parametrize('d', [15, 21])
def test_forward_pop_equals_single_forward(dev, d):
    from discrete_mean_field_game_amd import ops
    K, N = 3, 50
    pop = _population(d, K, _nets(d, 8, 'dropout_l1l2', K, 90, dev), dev)
    ds, da, gs, ga = _stores(d, K, 4, dev)
    st, ac = ds.reshape(-1, d)[:N].contiguous(), da.reshape(-1, d, d)[:N].contiguous()
    pst = gs.reshape(K, -1, d)[:, :N].contiguous()
    pac = ga.reshape(K, -1, d, d)[:, :N].contiguous()
    keys = [123, 2 ** 63 + 5, 77]
    for s_in, a_in in ((st, ac), (pst, pac)):
        out = torch.full((K, N), -9.0, device=dev)
        ops.reward_net_forward_pop(pop._net_struct, True, K, s_in, a_in, [2, 0], [keys[2], keys[0]], out=out,
                                   net_stride=pop._net_stride)
        for k in (0, 2):
            x, y = (s_in, a_in) if s_in.dim() == 2 else (s_in[k], a_in[k])
            ref = ops.reward_net_forward(pop.reward_net(k), x, y, seed=keys[k])
            assert torch.equal(out[k], ref), k
        assert torch.equal(out[1], torch.full((N,), -9.0, device=dev))


# ------------------------------------------------------------------ 3. reward_iteration
def test_reward_iteration_equals_ac_irl(dev):
    d, K = 15, 3
    pop = _population(d, K, _nets(d, 8, 'none', K, 100, dev), dev, lr_reward=[1e-3, 0.0, 3e-3], host_seeds=[5, 6, 7])
    pop._gen_store.push(*pop._generate(8))
    singles = []
    for k in range(K):
        ac = pop.learner(k)                       # the module random stream now is Random(host_seed_k)
        ac.reward_iteration(max_iterations=60, stop_criteria=2e-4, iter_check=10)
        singles.append((ac, random.getstate()))
    its, last = pop.reward_iteration(max_iterations=60, stop_criteria=2e-4, iter_check=10)
    assert len(set(its.tolist())) > 1, its
    assert its[1] == 20                          # lr_reward = 0: the second check repeats the first average
    for k, (ac, rstate) in enumerate(singles):
        assert ac.reward_update_count == its[k]
        assert pop.host_random_state(k) == rstate
        _compare(pop.learner(k).state_dict(), ac.state_dict())


# ------------------------------------------------------------------ 4. outerloop
@pytest.mark.parametrize('mode,final', [('step', False), ('rollout', False), ('step', True), ('rollout', True)])
def test_outerloop_equals_ac_irl(dev, mode, final):
    d, K = 21, 2
    pop = _population(d, K, _nets(d, 8, 'dropout_l1l2', K, 130, dev), dev, mode=mode, lr_reward=[2e-3, 5e-4])
    kw = dict(num_iterations=2, num_gen_from_policy=2, max_reward_iterations=20, max_forward_episodes=3, gamma=0.9,
              lr_critic=0.1, lr_actor=0.001)
    singles = []
    for k in range(K):
        ac = pop.learner(k)
        ac.outerloop(final_training=final, **kw)
        singles.append((ac, ac.state_dict()))
    state = random.getstate()
    thetas = pop.outerloop(final_training=final, **kw)
    assert random.getstate() == state
    for k, (ac, st) in enumerate(singles):
        assert thetas[k] == float(np.ravel(ac.theta)[0])
        _compare(pop.learner(k).state_dict(), st)
    pop.train(2, 0.9)
    for k, (ac, _) in enumerate(singles):
        ac.train(2, -1, 0.9)
        lk = pop.learner(k)
        assert float(np.ravel(lk.theta)[0]) == float(np.ravel(ac.theta)[0])
        assert np.array_equal(np.asarray(lk.w), np.asarray(ac.w))
        assert lk._reward_calls == ac._reward_calls


# ------------------------------------------------------------------ 5. independence
def test_learners_are_independent(dev):
    d, K = 15, 3
    outs = []
    for seeds, lrs in (([11, 12, 13], [1e-3, 2e-3, 3e-3]), ([11, 99, 13], [1e-3, 9e-3, 3e-3])):
        np.random.seed(0)                          # the same initial critic weights (actor_critic.init_w draws them)
        pop = _population(d, K, _nets(d, 8, 'dropout_l1l2', K, 150, dev), dev, seeds=seeds, lr_reward=lrs,
                          host_seeds=[1, 2, 3])
        pop.outerloop(num_iterations=1, num_gen_from_policy=2, max_reward_iterations=20, max_forward_episodes=2,
                      final_training=False)
        outs.append(pop)
    a, b = outs
    assert not torch.equal(a._flat[1], b._flat[1])
    for k in (0, 2):
        assert torch.equal(a._flat[k], b._flat[k]) and torch.equal(a._adam_m[k], b._adam_m[k])
        assert a.thetas[k] == b.thetas[k] and np.array_equal(a.w[k], b.w[k])
        assert a._calls_k[k] == b._calls_k[k] and a.reward_update_count[k] == b.reward_update_count[k]


# ------------------------------------------------------------------ 6. side effects and refusals
def test_no_module_random_use_and_refusals(dev):
    from discrete_mean_field_game_amd import _lib as L
    from discrete_mean_field_game_amd import ops
    d, K = 21, 2
    random.seed(4)
    state = random.getstate()
    pop = _population(d, K, _nets(d, 8, 'dropout_l1l2', K, 170, dev), dev)
    pop._gen_store.push(*pop._generate(6))
    pop.update_reward()
    pop.reward_iteration(20, 1e-4, 10)
    assert random.getstate() == state
    flat, m = pop._flat.clone(), pop._adam_m.clone()
    shared = _population(d, K, _nets(d, 8, 'dropout_l1l2', 1, 170, dev)[0], dev)
    for call in (shared.update_reward, lambda: shared.reward_iteration(10), lambda: shared.outerloop(1)):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(ValueError):
        _population(d, K, _nets(d, 8, 'dropout_l1l2', K, 170, dev), dev, demos=[_demos(d, 1)[0][:14]])
    with pytest.raises(ValueError):
        _population(d, K, _nets(d, 8, 'dropout_l1l2', K, 170, dev), dev, demos=[])
    from discrete_mean_field_game_amd.irl_population import AC_IRLPopulation
    nodemo = AC_IRLPopulation([8.0, 8.5], 0.1, 1e4, d, batch=32, reward_nets=_nets(d, 8, 'dropout_l1l2', K, 170, dev),
                              pi0=_table(d))
    with pytest.raises(ValueError):
        nodemo.update_reward()
    with pytest.raises(ValueError):
        pop.reward_iteration(10, 1e-4, 0)
    # C level: every refusal before a launch, nothing written
    dims = pop._rn_dims
    ds, da = pop._demo_store.state, pop._demo_store.action
    gs, ga = pop._gen_store.state, pop._gen_store.action

    def call(plan, n_active=1, ws_bytes=1 << 22, n_demo=5, dims=dims):
        ops.reward_net_train_steps_pop(pop._flat, pop._adam_m, pop._adam_v, pop._net_stride, K, dims, (ds, da), (gs, ga), plan,
                                       len(plan) // n_active, n_active, n_demo, 5, T, 5, 0.4, True, pop._rt_stats,
                                       torch.empty(ws_bytes, dtype=torch.uint8, device=dev),
                                       torch.empty(plan.nbytes, dtype=torch.uint8, device=dev))

    def plan_of(learners):
        p = ops.rn_train_plan(len(learners))
        for i, k in enumerate(learners):
            p[i]['learner'], p[i]['lr'], p[i]['adam_step'] = k, 1e-3, 1
        return p
    cases = [(plan_of([K]), 1, {}, -1), (plan_of([0, 0]), 2, {}, -1), (plan_of([1]), 1, {'ws_bytes': 256}, -4),
             (plan_of([0]), 1, {'dims': dims[:4] + (17,) + dims[5:]}, -3), (plan_of([0]), 1, {'n_demo': 65}, -3)]
    neg = plan_of([1])
    neg[0]['gen_rows'][2] = -1
    cases.append((neg, 1, {}, -1))
    for plan, n_active, kw, code in cases:
        with pytest.raises(L.MfgError) as e:
            call(plan, n_active, **kw)
        assert e.value.code == code, (plan['learner'], kw)
    with pytest.raises(L.MfgError) as e:
        ops.reward_net_forward_pop(pop._net_struct, True, K, ds.reshape(-1, d), da.reshape(-1, d, d), [1, 1], [1, 2],
                                   net_stride=pop._net_stride)
    assert e.value.code == -1
    torch.cuda.synchronize()
    assert torch.equal(pop._flat, flat) and torch.equal(pop._adam_m, m)
