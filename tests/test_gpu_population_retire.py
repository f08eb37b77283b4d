"""Retiring learners of a population on the device (the control block of mfg_ctx_set_pop_control): early stop and isolation of
a diverged learner, bit for bit (array_equal) against the single-learner class and against the same population without a
criterion.  Shapes are the smallest at which the population wrappers differ: d = 15 / 21 (the compile-time-d SUMS and STEP
variants), d = 5 (the generic-d path), batch 48 (no multiple of a tile), K = 3 / 4, at most 12 episodes, both update modes,
mixed precision and one f64 case each."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip('torch')

pytestmark = pytest.mark.gpu
B = 48
GAMMA = 0.9
DEV = 'cuda:0'


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.fail('-m gpu tests need a GPU')
    return torch.device(DEV)


def _table(d, seed=3):
    return np.random.RandomState(seed).dirichlet(np.ones(d), size=9)


def _w0(K, d, seed=5):
    return np.random.RandomState(seed).randn(K, d * (d + 1) // 2 + d + 1) * 0.1


@functools.lru_cache(maxsize=None)
def _nets(d, K):
    from discrete_mean_field_game_amd.networks import RewardNet
    out = []
    for j in range(K):
        torch.manual_seed(40 + d + j)
        net = RewardNet(d=d, n_fc3=8, n_fc4=4, keep_prob=0.4).to(DEV)
        with torch.no_grad():          # non-zero biases: every tensor of the network matters
            for p in net.parameters():
                if p.dim() == 1:
                    p.uniform_(-0.2, 0.2)
        out.append(net)
    return out


def _irl_pop(mode, d, K, precision, thetas=None, shift=0.05, **kw):
    from discrete_mean_field_game_amd.irl_population import AC_IRLPopulation
    thetas = np.linspace(8.2, 9.0, K) if thetas is None else thetas
    return AC_IRLPopulation(thetas, shift, 1e4, d, batch=B, reward_nets=_nets(d, K), seeds=[11 + 7 * k for k in range(K)],
                            w0=_w0(K, d), pi0=_table(d), update_every=mode, precision=precision, device=DEV, **kw)


def _ac_pop(mode, d, K, precision, thetas=None, shift=0.16):
    from discrete_mean_field_game_amd import ActorCriticPopulation
    thetas = np.linspace(8.2, 9.0, K) if thetas is None else thetas
    return ActorCriticPopulation(thetas, shift, 12000.0, d, batch=B, seeds=[5 + 3 * k for k in range(K)], w0=_w0(K, d),
                                 pi0=_table(d), update_every=mode, precision=precision, device=DEV)


def _criteria(traces, E):
    """Stop criteria from the stop-free traces |theta_e - theta_{e-1}| (traces[k][e - 1], e = 1 .. E), chosen between trace
    values: learner 0 stops after episode 1 (twice its first step); the first other learner with an episode strictly inside
    (1, E) whose step is below all its earlier ones stops there (the midpoint of that step and the smallest before it); every
    other learner never stops (half its smallest step; the last learner of K > 3 has no criterion at all).  Returns (criteria,
    stopping episodes, the learner that stops inside)."""
    K = len(traces)
    c = np.full(K, -1.0)
    ep = [E] * K
    c[0] = 2.0 * traces[0][0]
    ep[0] = 1
    mid = None
    for k in range(1, K):
        inside = [e for e in range(2, E) if traces[k][e - 1] < min(traces[k][:e - 1])]
        if inside:
            mid, e1 = k, inside[0]
            c[k] = 0.5 * (traces[k][e1 - 1] + min(traces[k][:e1 - 1]))
            ep[k] = e1
            break
    assert mid is not None, 'no learner with a step strictly inside (1, %d) below all its earlier ones: %r' % (E, traces)
    for k in range(1, K):
        if k != mid and not (K > 3 and k == K - 1):
            c[k] = 0.5 * min(traces[k])
    return c, ep, mid


def _stops_at(trace, c):
    """The episode after which AC_IRL.train's rule (ac_irl.py:726) leaves a run with this trace (len(trace) if never)."""
    for e, step in enumerate(trace, 1):
        if step < c:
            return e
    return len(trace)


# ------------------------------------------------------------------ 1. early stop equals AC_IRL.train(stop_criteria=c_k)
def _single_irl(pop0, k, mode, d, precision, E, c):
    """AC_IRL.train(E, stop_criteria=c) with learner k's settings; returns the object, its per-episode returns and thetas."""
    from discrete_mean_field_game_amd.ac_irl import AC_IRL
    ac = AC_IRL(float(pop0.theta_initial[k]), float(pop0.shifts[k]), float(pop0.alpha_scales[k]), d, pi0=_table(d),
                demonstrations=[], batch=B, seed=int(pop0.seeds[k]), update_every=mode, precision=precision, device=DEV, verbose=0)
    ac.reward_net = pop0.reward_net(k)
    ac.create_training_method()
    ac.w = _w0(pop0.K, d)[k]
    rets, ths = [], []

    def report(list_reward, consecutive, pi, *files, scale=1.0):      # (called once per episode with consecutive=1)
        rets.append(float(torch.cat(list_reward).sum().cpu()) * scale)
        ths.append(float(ac._theta.cpu()[0]))
    ac._report_irl = report
    ac.train(max_episodes=E, stop_criteria=c, gamma=GAMMA, constant=False, lr_critic=0.1, lr_actor=0.001, consecutive=1)
    return ac, np.array(rets), np.array(ths)


@pytest.mark.parametrize('d,mode,precision', [(15, 'step', 'mixed'), (15, 'rollout', 'mixed'), (21, 'step', 'mixed'),
                                              (21, 'rollout', 'mixed'), (15, 'step', 'f64')])
def test_early_stop_equals_the_single_class(dev, d, mode, precision):
    K, E = 3, 10
    pop = _irl_pop(mode, d, K, precision)
    th0 = pop.theta_initial
    traces = []
    for k in range(K):
        _, _, ths = _single_irl(pop, k, mode, d, precision, E, -1)
        assert len(ths) == E
        traces.append(np.abs(np.diff(np.concatenate([[th0[k]], ths]))))
    c, ep, mid = _criteria(traces, E)
    assert ep[0] == 1 and 1 < ep[mid] < E and ep[3 - mid] == E         # one after episode 1, one inside, one never
    singles = [_single_irl(pop, k, mode, d, precision, E, float(c[k])) for k in range(K)]
    # the three stopping episodes, on the single-learner runs, before anything is compared
    assert [int(ac.episodes_run) for ac, _, _ in singles] == ep
    ret = pop.train(E, GAMMA, False, 0.1, 0.001, stop_criteria=c)
    assert np.array_equal(pop.episodes_run, ep)
    assert np.array_equal(pop.learner_state, [int(e < E) for e in ep]) and pop.status() == 0
    for k, (ac, rets, _) in enumerate(singles):
        assert np.array_equal(pop.thetas[k], float(np.ravel(ac.theta)[0])), 'learner %d: theta' % k
        assert np.array_equal(pop.w[k], np.asarray(ac.w).reshape(-1)), 'learner %d: w' % k
        assert np.array_equal(ret[k, :ep[k]], rets), 'learner %d: returns' % k
        assert not ret[k, ep[k]:].any(), 'learner %d: returns beyond its last episode' % k
        assert pop.list_policies[k] == [float(np.ravel(t)[0]) for t in ac.list_policies], 'learner %d: list_policies' % k


# ------------------------------------------------------------------ 2. / 3. prefix property, neighbours untouched
PREFIX_CASES = [('ac', 5, 'step', 'mixed'), ('ac', 5, 'rollout', 'mixed'), ('ac', 15, 'step', 'mixed'), ('ac', 21, 'step', 'mixed'),
                ('ac', 21, 'rollout', 'mixed'), ('ac', 15, 'rollout', 'f64'), ('irl', 15, 'step', 'mixed'),
                ('irl', 21, 'step', 'mixed'), ('irl', 21, 'rollout', 'mixed'), ('irl', 15, 'rollout', 'f64')]


@functools.lru_cache(maxsize=None)
def _prefix_runs(cls, d, mode, precision):
    """One case's runs, shared by the two tests below: the stop-free trace (one call per episode), the run with criteria and
    the stop-free runs of E, e_0 and e_1 episodes.  Returns (stopping episodes, {episodes: (thetas, w, returns)}, the same
    triple of the run with criteria, its episodes_run and learner_state)."""
    K, E = 4, 8
    make = (lambda: _ac_pop(mode, d, K, precision)) if cls == 'ac' else (lambda: _irl_pop(mode, d, K, precision))
    args = (GAMMA, 0, 0.1, 0.001)

    def snap(pop, ret):
        return pop.thetas, pop.w, ret

    tr = make()
    ths = [tr.thetas]
    for e in range(E):
        tr.train(1, *args, first_episode=e)
        ths.append(tr.thetas)
    traces = np.abs(np.diff(np.array(ths), axis=0)).T            # [K, E]
    c, ep, _ = _criteria([list(t) for t in traces], E)
    assert [_stops_at(traces[k], c[k]) for k in range(K)] == ep
    free = {}
    for n in sorted(set(ep)):
        p = make()
        free[n] = snap(p, p.train(n, *args))
    pop = make()
    got = snap(pop, pop.train(E, *args, stop_criteria=c))
    assert pop.status() == 0
    return ep, free, got, pop.episodes_run, pop.learner_state


@pytest.mark.parametrize('cls,d,mode,precision', PREFIX_CASES)
def test_a_stopped_learner_holds_the_prefix(dev, cls, d, mode, precision):
    """A learner that stopped after e_k episodes holds exactly what the same population holds after train(e_k)."""
    ep, free, got, episodes_run, state = _prefix_runs(cls, d, mode, precision)
    E = max(ep)
    stopped = [k for k in range(4) if ep[k] < E]
    assert len(stopped) == 2 and ep[0] == 1 and 1 < ep[stopped[1]] < E
    assert np.array_equal(episodes_run, ep) and np.array_equal(state, [int(e < E) for e in ep])
    for k in stopped:
        th, w, ret = free[ep[k]]
        assert np.array_equal(got[0][k], th[k]) and np.array_equal(got[1][k], w[k]), 'learner %d' % k
        assert np.array_equal(got[2][k, :ep[k]], ret[k]) and not got[2][k, ep[k]:].any(), 'learner %d: returns' % k


@pytest.mark.parametrize('cls,d,mode,precision', PREFIX_CASES)
def test_neighbours_of_a_stopped_learner_are_untouched(dev, cls, d, mode, precision):
    """Learners that never stop equal the same call with stop_criteria=-1."""
    ep, free, got, _, _ = _prefix_runs(cls, d, mode, precision)
    E = max(ep)
    th, w, ret = free[E]
    running = [k for k in range(4) if ep[k] == E]
    assert len(running) == 2
    for k in running:
        assert np.array_equal(got[0][k], th[k]) and np.array_equal(got[1][k], w[k]), 'learner %d' % k
        assert np.array_equal(got[2][k], ret[k]), 'learner %d: returns' % k


# ------------------------------------------------------------------ 4. / 5. / 7. isolation
ISO_D, ISO_E = 21, 6
ISO_HEALTHY, ISO_BAD = [8.5, 8.7, 9.0], [8.5, 80.0, 9.0]      # 80 (1 + 0.16) = 92.8 > 86


@functools.lru_cache(maxsize=None)
def _healthy_run(mode):
    pop = _ac_pop(mode, ISO_D, 3, 'mixed', ISO_HEALTHY)
    ret = pop.train(ISO_E, GAMMA, 0, 0.1, 0.001)
    return pop.thetas, pop.w, ret


def _assert_others_equal_healthy(pop, ret, mode):
    th, w, ref = _healthy_run(mode)
    for k in (0, 2):
        assert np.array_equal(pop.thetas[k], th[k]) and np.array_equal(pop.w[k], w[k]), 'learner %d' % k
        assert np.array_equal(ret[k], ref[k]), 'learner %d: returns' % k


@pytest.mark.parametrize('mode', ['rollout', 'step'])
def test_isolation_from_the_start(dev, mode):
    from discrete_mean_field_game_amd import _lib as L
    pop = _ac_pop(mode, ISO_D, 3, 'mixed', ISO_BAD)
    w0 = pop.w
    assert np.array_equal(pop.learner_state, [0, 0, 0])
    ret = pop.train(ISO_E, GAMMA, 0, 0.1, 0.001, isolate=True)         # does not raise
    assert np.array_equal(pop.learner_state, [0, 2, 0])
    assert pop.episodes_run[1] == 0 and np.array_equal(pop.episodes_run[[0, 2]], [ISO_E, ISO_E])
    assert pop.learner_status[1] & L.STATUS_MIXED_RANGE and not pop.learner_status[[0, 2]].any()
    assert pop.thetas[1] == 80.0 and np.array_equal(pop.w[1], w0[1]) and not ret[1].any()
    assert pop.status() == 0                                            # the context's word
    _assert_others_equal_healthy(pop, ret, mode)
    with pytest.raises(L.MfgError):
        pop.learner(1)
    # isolate=False: raises as it always did
    bad = _ac_pop(mode, ISO_D, 3, 'mixed', ISO_BAD)
    with pytest.raises(L.MfgError):
        bad.train(ISO_E, GAMMA, 0, 0.1, 0.001)
    assert bad.status() & L.STATUS_MIXED_RANGE


def test_isolation_in_mid_run(dev):
    """Learner 1 diverges inside the call (an lr_actor under which the single class raises within the same episodes): it is
    frozen at an episode boundary, the others hold the bits of the healthy run."""
    from discrete_mean_field_game_amd import _lib as L
    from discrete_mean_field_game_amd.mfg_ac2 import actor_critic
    ref = _ac_pop('step', ISO_D, 3, 'mixed', ISO_HEALTHY)
    big = None
    for lr in (1e2, 1e4, 1e6, 1e8):
        ac = actor_critic(ISO_HEALTHY[1], float(ref.shifts[1]), float(ref.alpha_scales[1]), ISO_D, pi0=_table(ISO_D), batch=B,
                          seed=int(ref.seeds[1]), update_every='step', verbose=0)
        ac.w = _w0(3, ISO_D)[1]
        try:
            ac.train(ISO_E, GAMMA, 0, lr_critic=0.1, lr_actor=lr)
        except L.MfgError:
            big = lr
            break
    assert big is not None, 'no lr_actor made the single learner leave the mixed-precision range'
    ret = ref.train(ISO_E, GAMMA, 0, 0.1, [0.001, big, 0.001], isolate=True)
    assert np.array_equal(ref.learner_state, [0, 2, 0]) and ref.episodes_run[1] < ISO_E
    assert ref.learner_status[1] != 0 and ref.status() == 0
    _assert_others_equal_healthy(ref, ret, 'step')


def test_a_failed_learner_under_a_criterion_raises_after_the_others_trained(dev):
    """isolate=False with a stop criterion (a controlled call): the diverged learner is booked to its own word and frozen, the
    context's word stays 0, the others finish the call, and train() raises afterwards -- in every later call too, until
    clear_status()."""
    from discrete_mean_field_game_amd import _lib as L
    pop = _ac_pop('step', ISO_D, 3, 'mixed', ISO_BAD)
    w0 = pop.w
    with pytest.raises(L.MfgError, match=r'learner\(s\) \[1\]'):
        pop.train(ISO_E, GAMMA, 0, 0.1, 0.001, stop_criteria=0.0)        # (|step| < 0 never holds: nobody stops)
    assert pop.status() == 0
    assert np.array_equal(pop.learner_state, [0, 2, 0]) and np.array_equal(pop.episodes_run, [ISO_E, 0, ISO_E])
    assert pop.learner_status[1] & L.STATUS_MIXED_RANGE
    assert pop.thetas[1] == 80.0 and np.array_equal(pop.w[1], w0[1])
    th, w, _ = _healthy_run('step')
    for k in (0, 2):
        assert np.array_equal(pop.thetas[k], th[k]) and np.array_equal(pop.w[k], w[k]), 'learner %d' % k
    before = pop.thetas
    with pytest.raises(L.MfgError, match=r'learner\(s\) \[1\]'):
        pop.train(1, GAMMA, 0, 0.1, 0.001, first_episode=ISO_E)          # a default call: not refused, learner 1 skipped
    assert pop.status() == 0 and np.array_equal(pop.learner_state, [0, 2, 0])
    assert pop.thetas[1] == 80.0 and pop.thetas[0] != before[0] and pop.thetas[2] != before[2]


@pytest.mark.parametrize('index,value', [(70, np.nan), (-1, np.inf)])
def test_a_non_finite_w_fails_the_learner_alone(dev, index, value):
    """The non-finite scan of k_pop_retire over w[F] (F = 136 at d = 15: two full strides of the wave and a tail of 8): one
    entry of learner 1's w, past the first stride or the very last, is set to NaN / inf on the host of an f64 population --
    which has no range predicate and no status word of its own to fire."""
    from discrete_mean_field_game_amd import _lib as L
    d, E = 15, 3
    ref = _ac_pop('rollout', d, 3, 'f64')
    ref_ret = ref.train(E, GAMMA, 0, 0.1, 0.001)
    pop = _ac_pop('rollout', d, 3, 'f64')
    pop._w[1, index] = value
    w0, th0 = pop.w, pop.thetas
    ret = pop.train(E, GAMMA, 0, 0.1, 0.001, isolate=True)
    assert np.array_equal(pop.learner_state, [0, 2, 0]) and np.array_equal(pop.episodes_run, [E, 0, E])
    assert np.array_equal(pop.learner_status, [0, L.STATUS_POP_NONFINITE, 0]) and pop.status() == 0
    assert pop.thetas[1] == th0[1] and np.array_equal(pop.w[1], w0[1], equal_nan=True) and not ret[1].any()
    for k in (0, 2):
        assert np.array_equal(pop.thetas[k], ref.thetas[k]) and np.array_equal(pop.w[k], ref.w[k]), 'learner %d' % k
        assert np.array_equal(ret[k], ref_ret[k]), 'learner %d: returns' % k


def test_a_plain_call_resets_what_the_last_controlled_call_reported(dev):
    pop = _ac_pop('step', 5, 3, 'mixed')
    pop.train(3, GAMMA, 0, 0.1, 0.001, stop_criteria=1e9)                # everybody stops after episode 1
    assert np.array_equal(pop.learner_state, [1, 1, 1]) and np.array_equal(pop.episodes_run, [1, 1, 1])
    pop.train(2, GAMMA, 0, 0.1, 0.001, first_episode=1)                  # no control block
    assert np.array_equal(pop.learner_state, [0, 0, 0]) and np.array_equal(pop.episodes_run, [2, 2, 2])


def test_clear_status_revives_a_learner(dev):
    pop = _ac_pop('step', ISO_D, 3, 'mixed', ISO_BAD)
    pop.train(1, GAMMA, 0, 0.1, 0.001, isolate=True)
    assert np.array_equal(pop.learner_state, [0, 2, 0])
    pop.train(1, GAMMA, 0, 0.1, 0.001, first_episode=1, isolate=True)  # failed persists: still frozen
    assert np.array_equal(pop.learner_state, [0, 2, 0]) and pop.thetas[1] == 80.0 and pop.episodes_run[1] == 0
    pop._theta[1:2].fill_(8.7)
    pop.clear_status(1)
    assert np.array_equal(pop.learner_state, [0, 0, 0]) and not pop.learner_status.any()
    pop.train(2, GAMMA, 0, 0.1, 0.001, first_episode=2, isolate=True)
    assert np.array_equal(pop.learner_state, [0, 0, 0]) and np.array_equal(pop.episodes_run, [2, 2, 2])
    assert pop.thetas[1] != 8.7 and np.isfinite(pop.thetas[1]) and pop.status() == 0
    assert pop.learner(1) is not None


# ------------------------------------------------------------------ 6. the outer loop with one learner failed from the start
def _demos(d, n, seed=5):
    rs = np.random.RandomState(seed)
    return [[(rs.dirichlet(np.ones(d)), rs.dirichlet(np.ones(d), size=d)) for _ in range(15)] for _ in range(n)]


def test_outerloop_completes_without_the_failed_learner(dev, tmp_path, monkeypatch):
    d, K = 15, 3
    kw = dict(demonstrations=_demos(d, 7), lr_reward=1e-3, num_policies=3)
    loop = dict(num_iterations=2, num_gen_from_policy=2, max_reward_iterations=10, max_forward_episodes=2, gamma=GAMMA,
                final_training=False)
    ref = _irl_pop('step', d, K, 'mixed', [8.0, 8.5, 9.0], shift=0.16, **kw)
    ref.outerloop(**loop)
    pop = _irl_pop('step', d, K, 'mixed', [8.0, 80.0, 9.0], shift=0.16, **kw)
    pop.outerloop(isolate=True, **loop)                                 # completes
    assert np.array_equal(pop.learner_state, [0, 2, 0]) and pop.status() == 0
    for k in (0, 2):
        assert np.array_equal(pop.thetas[k], ref.thetas[k]) and np.array_equal(pop.w[k], ref.w[k]), 'learner %d' % k
        assert torch.equal(pop._flat[k], ref._flat[k]), 'learner %d: reward network' % k
    assert pop.thetas[1] == 80.0
    rs = np.random.RandomState(1)
    (tmp_path / 'testdir').mkdir()
    for j in range(3):
        np.savetxt(str(tmp_path / 'testdir' / ('f%d.csv' % j)), rs.dirichlet(np.ones(d), size=16), delimiter=' ')
    monkeypatch.chdir(tmp_path)
    out = pop.evaluate(16, 'testdir', str(tmp_path / 'eval.csv'))
    assert out.shape == (K, 4) and np.isnan(out[1]).all() and np.isfinite(out[[0, 2]]).all()
    assert len(open(str(tmp_path / 'eval.csv')).read().strip().splitlines()) == 2      # no line for the failed learner
