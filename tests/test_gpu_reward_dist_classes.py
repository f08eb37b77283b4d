"""-m gpu: AC_IRLPopulation.reward_distribution / action_heatmap and their AC_IRL forms (the numbers of plot_reward_distribution
and plot_action_heatmap, ac_irl.py:1046-1123, :1276-1289): the statistics equal NumPy / SciPy applied to the rewards the call
itself returns, the JSDs the reference's formula on the counts, learner k the single-learner class bit for bit; what the call
leaves alone and how far the counters move; missing sets and failed learners."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
T, D, K = 15, 15, 3
N_TRAIN, N_TEST = 4, 3
POINTS = (('dropout', 8, 4), ('l1l2', 8, 4), ('dropout_l1l2', 6, 8))      # the last learner: another n_fc3 and n_fc4
U = 2.0 ** -52


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
                    p.uniform_(-0.2, 0.2)
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
    """One population call with everything given, and its twin population left where the first one started."""
    pop, twin = _population(dev), _population(dev)
    before = (pop._calls_k.copy(), pop._rng_step, pop._gen_traj_counter)
    got = pop.reward_distribution(pi0_test=TABLE_TEST, want_rewards=True)
    heat = pop.action_heatmap()
    return pop, twin, got, (before, heat)


def _check_against_oracle(counts, edges, density, moments, xs, r, bins=20):
    from scipy.stats import gaussian_kde
    x = r.astype(np.float64)
    n = x.size
    c, e = np.histogram(x, bins)
    assert np.array_equal(counts, c) and np.array_equal(edges, e)
    assert moments[0] == n and moments[1] == x.min() and moments[2] == x.max()
    assert abs(moments[3] - x.mean()) <= n * U * np.abs(x).max()
    var = np.var(x, ddof=1)
    assert abs(moments[4] - var) <= 4 * n * U * var
    kde = gaussian_kde(x)
    assert abs(moments[5] - float(kde.covariance[0, 0])) <= (4 * n + 8) * U * var
    np.testing.assert_allclose(density, kde(xs), rtol=1e-11, atol=1e-300)


def test_statistics_are_the_oracles_on_the_returned_rewards(run):
    pop, _, got, _ = run
    assert got.sets == ('demo_train', 'demo_test', 'gen_train', 'gen_test')
    assert got.moments.shape == (K, 4, 6) and got.counts.shape == (K, 4, 20) and got.counts.dtype == np.int64
    assert got.edges.shape == (K, 4, 21) and got.density.shape == (K, 4, 200) and got.jsd.shape == (K, 3)
    assert got.status.shape == (K, 4) and not got.status.any()
    assert np.array_equal(got.xs, np.linspace(-0.1, 0.4, 200))
    sizes = (N_TRAIN * T, N_TEST * T, N_TRAIN * T, N_TRAIN * T)
    for s in range(4):
        assert got.rewards[s].shape == (K, sizes[s]) and got.rewards[s].dtype == np.float32
        for k in range(K):
            _check_against_oracle(got.counts[k, s], got.edges[k, s], got.density[k, s], got.moments[k, s], got.xs,
                                  got.rewards[s][k])
    # the learners' networks differ: so do their rewards
    assert not np.array_equal(got.rewards[0][0], got.rewards[0][1])


def test_jsd_is_the_reference_formula_on_the_counts(run):
    from scipy.stats import entropy
    _, _, got, _ = run
    for k in range(K):
        for j, (a, b) in enumerate(((0, 1), (0, 2), (1, 3))):
            P, Q = got.counts[k, a].astype(np.float64), got.counts[k, b].astype(np.float64)
            P[P == 0] = 1e-100
            Q[Q == 0] = 1e-100
            M = 0.5 * (P + Q)
            want = 0.5 * (entropy(P, M) + entropy(Q, M))
            assert abs(got.jsd[k, j] - want) <= 1e-14 * max(1.0, want), (k, j)
    assert (got.jsd > 0).all()


def test_learner_k_is_ac_irl_bit_for_bit(run):
    pop, twin, got, (_, heat) = run
    for k in range(K):
        ac = twin.learner(k)
        ac.mat_pi0_test = TABLE_TEST.copy()
        ac.num_start_samples_test = TABLE_TEST.shape[0]
        theta0, calls0 = np.array(ac.theta, dtype=np.float64).copy(), ac._reward_calls
        ref = ac.reward_distribution(want_rewards=True)
        for name in ('moments', 'counts', 'edges', 'density', 'jsd', 'status'):
            assert np.array_equal(getattr(got, name)[k], getattr(ref, name)), (k, name)
        assert np.array_equal(got.xs, ref.xs)
        for s in range(4):
            assert np.array_equal(got.rewards[s][k], ref.rewards[s]), (k, s)
        assert np.array_equal(np.array(ac.theta, dtype=np.float64), theta0) and ac._reward_calls == calls0 + 4
        demo_avg, gen_avg, diff = ac.action_heatmap()
        assert np.array_equal(gen_avg, heat[1][k]) and np.array_equal(demo_avg, heat[0]) and np.array_equal(diff, heat[2][k])
        assert ac._rng_step == pop._rng_step and ac._gen_traj_counter == pop._gen_traj_counter
        assert np.array_equal(ac._reward_calls, pop._calls_k[k])


def test_counters_advance_as_documented_and_state_is_left_alone(dev, run):
    pop, _, _, ((calls0, step0, traj0), _) = run
    # the fixture's reward_distribution (four forwards, two generations) and action_heatmap (one generation)
    calls1, step1, traj1 = pop._calls_k.copy(), pop._rng_step, pop._gen_traj_counter
    assert (calls1 - calls0 == 4).all() and step1 - step0 == 3 * T and traj1 - traj0 == 3 * N_TRAIN
    pop = _population(dev)
    calls1, step1, traj1 = pop._calls_k.copy(), pop._rng_step, pop._gen_traj_counter
    thetas, w = pop.thetas.copy(), pop.w.copy()
    store = (pop._gen_store.version, list(pop._gen_store.rows))
    flat = pop._flat.clone()
    again = pop.reward_distribution(thetas=[8.2, 8.3, 8.4], pi0_test=TABLE_TEST, num_bins=7, num_points=5, hist_range=(-1.0, 1.0))
    assert again.rewards is None and again.counts.shape == (K, 4, 7) and again.density.shape == (K, 4, 5)
    assert np.array_equal(again.edges[0, 0], np.linspace(-1.0, 1.0, 8)) and np.array_equal(again.edges[2, 3], again.edges[0, 0])
    assert np.array_equal(pop._calls_k, calls1 + 4) and pop._rng_step == step1 + 2 * T
    assert pop._gen_traj_counter == traj1 + 2 * N_TRAIN
    assert np.array_equal(pop.thetas, thetas) and np.array_equal(pop.w, w) and torch.equal(pop._flat, flat)
    assert (pop._gen_store.version, list(pop._gen_store.rows)) == store
    pop.action_heatmap(thetas=8.3)
    assert np.array_equal(pop._calls_k, calls1 + 4) and pop._rng_step == step1 + 3 * T
    assert pop._gen_traj_counter == traj1 + 3 * N_TRAIN and np.array_equal(pop.thetas, thetas)
    assert (pop._gen_store.version, list(pop._gen_store.rows)) == store


def test_given_thetas_change_the_generated_sets_only(dev):
    a, b = _population(dev), _population(dev)
    ra = a.reward_distribution(pi0_test=TABLE_TEST, want_rewards=True)
    rb = b.reward_distribution(thetas=[8.2, 8.3, 8.4], pi0_test=TABLE_TEST, want_rewards=True)
    for s in (0, 1):
        assert np.array_equal(ra.rewards[s], rb.rewards[s])
    for s in (2, 3):
        assert not np.array_equal(ra.rewards[s], rb.rewards[s])
    # ... and they are the policies rolled: a population that HOLDS these thetas generates the same sets
    c = _population(dev)
    c._theta.copy_(torch.as_tensor([8.2, 8.3, 8.4], dtype=torch.float64, device=dev))
    rc = c.reward_distribution(pi0_test=TABLE_TEST, want_rewards=True)
    for s in range(4):
        assert np.array_equal(rb.rewards[s], rc.rewards[s]), s


def test_missing_sets_are_nan_with_status_minus_one(dev):
    pop = _population(dev, with_test=False)
    calls, step, traj = pop._calls_k.copy(), pop._rng_step, pop._gen_traj_counter
    got = pop.reward_distribution(want_rewards=True)
    assert np.array_equal(got.status, [[0, -1, 0, -1]] * K)
    for s in (1, 3):
        assert np.isnan(got.moments[:, s]).all() and np.isnan(got.edges[:, s]).all() and np.isnan(got.density[:, s]).all()
        assert not got.counts[:, s].any() and got.rewards[s] is None
    assert np.isnan(got.jsd[:, [0, 2]]).all() and np.isfinite(got.jsd[:, 1]).all()
    assert np.isfinite(got.moments[:, [0, 2]]).all()
    assert np.array_equal(pop._calls_k, calls + 2) and pop._rng_step == step + T and pop._gen_traj_counter == traj + N_TRAIN
    # the sets that are there are those of the full call: the forwards come in the order of `sets`, a missing one has none
    full = _population(dev).reward_distribution(want_rewards=True)
    assert np.array_equal(full.rewards[0], got.rewards[0]) and np.array_equal(full.status, [[0, 0, 0, -1]] * K)


def test_failed_learner_gives_nan_rows_and_the_others_stand(dev):
    ref = _population(dev, isolate=True)
    pop = _population(dev, thetas=(8.0, 80.0, 9.0), isolate=True)
    assert np.array_equal(pop.learner_state, [0, 2, 0]) and np.array_equal(ref.learner_state, [0, 0, 0])
    got = pop.reward_distribution(pi0_test=TABLE_TEST, want_rewards=True)
    want = ref.reward_distribution(pi0_test=TABLE_TEST, want_rewards=True)
    assert np.array_equal(got.status[1], [1, 1, 1, 1]) and np.isnan(got.jsd[1]).all()
    assert np.isnan(got.moments[1]).all() and np.isnan(got.density[1]).all() and not got.counts[1].any()
    for k in (0, 2):
        for name in ('moments', 'counts', 'edges', 'density', 'jsd', 'status'):
            assert np.array_equal(getattr(got, name)[k], getattr(want, name)[k]), (k, name)
    h, hr = pop.action_heatmap(), ref.action_heatmap()
    assert np.isnan(h[1][1]).all() and np.isnan(h[2][1]).all() and np.array_equal(h[0], hr[0])
    for k in (0, 2):
        assert np.array_equal(h[1][k], hr[1][k]) and np.array_equal(h[2][k], hr[2][k])


def test_action_heatmap_is_numpys_mean(dev):
    pop, twin = _population(dev), _population(dev)
    demo_avg, gen_avg, diff = pop.action_heatmap()
    n = N_TRAIN * T
    want_demo = np.mean(pop._demo_np[1].astype(np.float64).reshape(n, D, D), axis=0)
    assert demo_avg.shape == (D, D) and np.abs(demo_avg - want_demo).max() <= n * U
    _, actions = twin._generate(N_TRAIN)               # the same keys: the twin stands where pop stood
    want_gen = np.mean(actions.cpu().numpy().astype(np.float64).reshape(K, n, D, D), axis=1)
    assert gen_avg.shape == (K, D, D) and np.abs(gen_avg - want_gen).max() <= n * U
    assert np.array_equal(diff, np.abs(demo_avg[None] - gen_avg))
    assert not np.array_equal(gen_avg[0], gen_avg[1])


def test_refusals(dev):
    from discrete_mean_field_game_amd.ac_irl import AC_IRL
    pop = _population(dev, with_test=False)
    calls, step = pop._calls_k.copy(), pop._rng_step
    for kw in (dict(num_bins=0), dict(num_bins=1025), dict(num_points=4097), dict(hist_range=(0.3, 0.3)), dict(thetas=[8.0, 8.1])):
        with pytest.raises(ValueError):
            pop.reward_distribution(**kw)
    assert np.array_equal(pop._calls_k, calls) and pop._rng_step == step        # refused before anything ran
    ac = AC_IRL(8.5, 0.16, 1e4, D, pi0=_table(3), demonstrations=_demos(2, 5), rng='numpy', device=dev, verbose=0)
    with pytest.raises(ValueError):
        ac.reward_distribution()
    with pytest.raises(ValueError):
        ac.action_heatmap()
