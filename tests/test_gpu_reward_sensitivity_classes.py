"""-m gpu: AC_IRLPopulation.reward_sensitivity / reward_heatmap and their AC_IRL forms: learner k is the single-learner class
bit for bit; the call leaves a population in the state reward_distribution leaves it in (counters, rewards, a following
train()); no theta changes and D_samp is untouched; chunks under a byte budget give the same bits; missing sets and failed
learners; reward_heatmap is one population forward over its nine pairs (the numbers of plot_reward_heatmap,
ac_irl.py:1378-1443)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
T, D, K = 15, 15, 3
N_TRAIN, N_TEST = 4, 3
POINTS = (('dropout', 8, 4), ('l1l2', 8, 4), ('dropout_l1l2', 6, 8))      # the last learner: another n_fc3 and n_fc4
U = 2.0 ** -52
FIELDS = ('grad_state', 'grad_action', 'gxi_state', 'gxi_action', 'status')


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.fail('-m gpu tests need a GPU')
    return torch.device('cuda:0')


def _nets(dev, seed0=800):
    from discrete_mean_field_game_amd.networks import RewardNet
    out = []
    for j, (reg, n3, n4) in enumerate(POINTS):
        torch.manual_seed(seed0 + j)
        net = RewardNet(d=D, reg=reg, n_fc3=n3, n_fc4=n4).to(dev)
        with torch.no_grad():
            for p in net.parameters():
                if p.dim() == 1:
                    p.uniform_(0.05, 0.3)
        out.append(net)
    return out


def _table(seed, n=9):
    return np.random.RandomState(seed).dirichlet(np.ones(D), size=n)


def _demos(n, seed):
    rs = np.random.RandomState(seed)
    return [[(rs.dirichlet(np.ones(D)), rs.dirichlet(np.ones(D), size=D)) for _ in range(T)] for _ in range(n)]


TABLE_TEST = _table(17, 6)


def _population(dev, with_test=True, thetas=(8.0, 8.5, 9.0), isolate=False):
    from discrete_mean_field_game_amd.irl_population import AC_IRLPopulation
    np.random.seed(4)
    pop = AC_IRLPopulation(np.array(thetas), 0.16, 1e4, D, batch=32, reward_nets=_nets(dev), seeds=[11, 12, 13], pi0=_table(3),
                           update_every='step', precision='mixed', device=dev, demonstrations=_demos(N_TRAIN, 5),
                           lr_reward=1e-3, num_policies=3, mixed_nets=True,
                           demonstrations_test=_demos(N_TEST, 8) if with_test else None)
    pop.train(1, 0.9, isolate=isolate)
    return pop


@pytest.fixture(scope='module')
def run(dev):
    """One population call with everything given, then the heatmap, and a twin population left where the first one started."""
    pop, twin = _population(dev), _population(dev)
    got = pop.reward_sensitivity(pi0_test=TABLE_TEST, dropout=True, want_samples=True)
    heat = pop.reward_heatmap()
    return pop, twin, got, heat


def test_shapes_and_means_of_the_returned_samples(run):
    _, _, got, _ = run
    sizes = (N_TRAIN * T, N_TEST * T, N_TRAIN * T, N_TRAIN * T)
    assert got.sets == ('demo_train', 'demo_test', 'gen_train', 'gen_test') and np.array_equal(got.count, sizes)
    assert got.grad_state.shape == (K, 4, D) and got.grad_action.shape == (K, 4, D, D)
    assert got.gxi_state.shape == (K, 4, D) and got.gxi_action.shape == (K, 4, D, D)
    assert got.status.shape == (K, 4) and not got.status.any()
    for s in range(4):
        gs, ga = got.samples[s]
        assert gs.shape == (K, sizes[s], D) and ga.shape == (K, sizes[s], D, D) and gs.dtype == np.float32
        assert got.rewards[s].shape == (K, sizes[s])
        for k in range(K):
            g = ga[k].astype(np.float64)
            assert np.abs(got.grad_action[k, s] - g.mean(0)).max() <= sizes[s] * U * np.abs(g).max()
            g = gs[k].astype(np.float64)
            assert np.abs(got.grad_state[k, s] - g.mean(0)).max() <= sizes[s] * U * np.abs(g).max()
    assert np.abs(got.grad_action).max() > 0 and not np.array_equal(got.grad_action[0], got.grad_action[1])
    one = got.learner(2)
    assert np.array_equal(one.grad_action, got.grad_action[2]) and np.array_equal(one.samples[1][0], got.samples[1][0][2])
    assert np.array_equal(one.rewards[3], got.rewards[3][2]) and one.status.shape == (4,)


def test_learner_k_is_ac_irl_bit_for_bit(run):
    pop, twin, got, heat = run
    for k in range(K):
        ac = twin.learner(k)
        ac.mat_pi0_test = TABLE_TEST.copy()
        ac.num_start_samples_test = TABLE_TEST.shape[0]
        theta0, calls0 = np.array(ac.theta, dtype=np.float64).copy(), ac._reward_calls
        ref = ac.reward_sensitivity(dropout=True, want_samples=True)
        for name in FIELDS:
            assert np.array_equal(getattr(got, name)[k], getattr(ref, name)), (k, name)
        assert np.array_equal(got.count, ref.count)
        for s in range(4):
            assert np.array_equal(got.rewards[s][k], ref.rewards[s]), (k, s)
            assert np.array_equal(got.samples[s][0][k], ref.samples[s][0]) and np.array_equal(got.samples[s][1][k], ref.samples[s][1])
        assert np.array_equal(np.array(ac.theta, dtype=np.float64), theta0) and ac._reward_calls == calls0 + 4
        r, states, actions = ac.reward_heatmap()
        assert np.array_equal(r, heat[0][k]) and np.array_equal(states, heat[1]) and np.array_equal(actions, heat[2][k])
        assert np.array_equal(np.array(ac.theta, dtype=np.float64), theta0)
        assert ac._rng_step == pop._rng_step and ac._gen_traj_counter == pop._gen_traj_counter
        assert np.array_equal(ac._reward_calls, pop._calls_k[k])


@pytest.mark.parametrize('dropout', [True, False])
def test_leaves_the_population_where_reward_distribution_leaves_it(dev, dropout):
    a, b = _population(dev), _population(dev)
    thetas, w, flat = b.thetas.copy(), b.w.copy(), b._flat.clone()
    store = (b._gen_store.version, list(b._gen_store.rows))
    geom = b._geom[0].copy()
    ra = a.reward_distribution(pi0_test=TABLE_TEST, want_rewards=True)
    rb = b.reward_sensitivity(pi0_test=TABLE_TEST, dropout=dropout)
    assert a._rng_step == b._rng_step and a._gen_traj_counter == b._gen_traj_counter and np.array_equal(a._calls_k, b._calls_k)
    for s in range(4):
        if dropout:
            assert np.array_equal(ra.rewards[s], rb.rewards[s]), s
        else:       # the learner without dropout (keep_prob = 1) is the same either way; the others are evaluated at keep_prob = 1
            assert np.array_equal(ra.rewards[s][1], rb.rewards[s][1]) and not np.array_equal(ra.rewards[s][0], rb.rewards[s][0])
    # no theta changes, no network changes, D_samp is untouched
    assert np.array_equal(b.thetas, thetas) and np.array_equal(b.w, w) and torch.equal(b._flat, flat)
    assert (b._gen_store.version, list(b._gen_store.rows)) == store and np.array_equal(b._geom[0], geom)
    a.train(2, 0.9)
    b.train(2, 0.9)
    assert np.array_equal(a.thetas, b.thetas) and np.array_equal(a.w, b.w)
    assert a._rng_step == b._rng_step and np.array_equal(a._calls_k, b._calls_k)


def test_chunks_under_a_budget_and_given_thetas(dev, run):
    _, twin, got, _ = run
    pop = _population(dev)
    per = 60 * (D + D * D) * 4 + 2 * 2 * (D + D * D) * 8          # one learner's workspace at N = 60: one learner per chunk
    small = pop.reward_sensitivity(pi0_test=TABLE_TEST, dropout=True, budget=per + 100)
    for name in FIELDS:
        assert np.array_equal(getattr(small, name), getattr(got, name)), name
    assert small.samples is None
    with pytest.raises(ValueError):
        pop.reward_sensitivity(pi0_test=TABLE_TEST, budget=per - 1)
    # given thetas move the generated sets only, and no theta changes
    thetas = pop.thetas.copy()
    other = pop.reward_sensitivity(thetas=[8.2, 8.3, 8.4], pi0_test=TABLE_TEST, dropout=False)
    plain = _population(dev)
    plain.reward_sensitivity(pi0_test=TABLE_TEST)                  # (to the same counters)
    plain = plain.reward_sensitivity(pi0_test=TABLE_TEST, dropout=False)
    assert np.array_equal(pop.thetas, thetas)
    for s in (0, 1):
        assert np.array_equal(other.grad_action[:, s], plain.grad_action[:, s])
    for s in (2, 3):
        assert not np.array_equal(other.grad_action[:, s], plain.grad_action[:, s])


def test_missing_sets_and_failed_learners(dev):
    pop = _population(dev, with_test=False)
    calls, step, traj = pop._calls_k.copy(), pop._rng_step, pop._gen_traj_counter
    got = pop.reward_sensitivity()
    assert np.array_equal(got.status, [[0, -1, 0, -1]] * K) and np.array_equal(got.count, [N_TRAIN * T, 0, N_TRAIN * T, 0])
    for s in (1, 3):
        assert np.isnan(got.grad_state[:, s]).all() and np.isnan(got.gxi_action[:, s]).all() and got.rewards[s] is None
    assert np.isfinite(got.grad_action[:, [0, 2]]).all()
    assert np.array_equal(pop._calls_k, calls + 2) and pop._rng_step == step + T and pop._gen_traj_counter == traj + N_TRAIN
    ref = _population(dev, isolate=True)
    bad = _population(dev, thetas=(8.0, 80.0, 9.0), isolate=True)
    assert np.array_equal(bad.learner_state, [0, 2, 0])
    got, want = bad.reward_sensitivity(pi0_test=TABLE_TEST), ref.reward_sensitivity(pi0_test=TABLE_TEST)
    assert np.array_equal(got.status[1], [1, 1, 1, 1])
    assert np.isnan(got.grad_state[1]).all() and np.isnan(got.gxi_action[1]).all() and np.isnan(got.rewards[0][1]).all()
    for k in (0, 2):
        for name in FIELDS:
            assert np.array_equal(getattr(got, name)[k], getattr(want, name)[k]), (k, name)
    h, hr = bad.reward_heatmap(), ref.reward_heatmap()
    assert np.isnan(h[0][1]).all() and np.isnan(h[2][1]).all()
    for k in (0, 2):
        assert np.array_equal(h[0][k], hr[0][k]) and np.array_equal(h[2][k], hr[2][k])


def test_heatmap_is_one_forward_over_its_nine_pairs(dev):
    from discrete_mean_field_game_amd import reward_dist
    from discrete_mean_field_game_amd.reward_learning import RN_SEED_OFFSET, philox_call_key
    pop, twin, third = _population(dev), _population(dev), _population(dev)
    calls, step, traj = pop._calls_k.copy(), pop._rng_step, pop._gen_traj_counter
    thetas = pop.thetas.copy()
    r, states, actions = pop.reward_heatmap()
    assert r.shape == (K, 3, 3) and r.dtype == np.float32 and states.shape == (3, D) and actions.shape == (K, 3, D, D)
    # the counters: one generation of one trajectory, one reward call; no theta is assigned
    assert np.array_equal(pop._calls_k, calls + 1) and pop._rng_step == step + T and pop._gen_traj_counter == traj + 1
    assert np.array_equal(pop.thetas, thetas)
    # the prototypes
    assert np.array_equal(states, reward_dist.heatmap_states(pop.mat_pi0, D))
    assert np.array_equal(states[0], pop.mat_pi0[0].astype(np.float32)) and np.array_equal(states[2], np.full(D, 1.0 / D, np.float32))
    table = torch.as_tensor(states[1:2].copy(), device=dev)
    _, ac = twin._generate(1, mat_dev=table, theta=torch.full((K,), 8.64, dtype=torch.float64, device=dev))
    a1 = ac[:, 0, 0].cpu().numpy()
    assert np.array_equal(actions[:, 0], a1) and np.array_equal(actions[:, 2], a1[:, :, ::-1])
    assert np.array_equal(actions[:, 1], np.full((K, D, D), 1.0 / D, np.float32))
    # mass moves to more popular (lower-index) topics under action 1
    assert (np.tril(a1, -1).sum((1, 2)) > np.triu(a1, 1).sum((1, 2))).all()
    # one _forward over the nine pairs, state-major
    st9 = np.repeat(states[None, :, None, :], 3, axis=2).repeat(K, axis=0).reshape(K, 9, D)
    ac9 = np.repeat(actions[:, None], 3, axis=1).reshape(K, 9, D, D)
    twin._calls_k += 1
    keys = [philox_call_key(twin.seeds[k], RN_SEED_OFFSET, twin._calls_k[k]) for k in range(K)]
    want = twin._forward(torch.as_tensor(st9, device=dev), torch.as_tensor(np.ascontiguousarray(ac9), device=dev), list(range(K)), keys)
    assert np.array_equal(r, want.cpu().numpy().reshape(K, 3, 3))
    # explicit states / actions skip the generation
    r3, s3, a3 = third.reward_heatmap(states=states, actions=actions)
    assert np.array_equal(r3, r) and np.array_equal(s3, states) and np.array_equal(a3, actions)
    assert third._rng_step == step and third._gen_traj_counter == traj and np.array_equal(third._calls_k, calls + 1)
    shared = third.reward_heatmap(states=states, actions=actions[0])
    assert shared[2].shape == (K, 3, D, D) and np.array_equal(shared[2][2], actions[0])
    with pytest.raises(ValueError):
        third.reward_heatmap(states=states[:2])
    with pytest.raises(ValueError):
        third.reward_heatmap(actions=actions[:2])


def test_refusals(dev):
    from discrete_mean_field_game_amd.ac_irl import AC_IRL
    ac = AC_IRL(8.5, 0.16, 1e4, D, pi0=_table(3), demonstrations=_demos(2, 5), rng='numpy', device=dev, verbose=0)
    with pytest.raises(ValueError):
        ac.reward_sensitivity()
    with pytest.raises(ValueError):
        ac.reward_heatmap()
