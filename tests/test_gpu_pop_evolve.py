"""-m gpu: population-based training inside a population training call (mfg_ctx_set_pop_evolve; train(..., validate=V,
evolve=E)).

Everything is compared bit for bit (array_equal): exploit is copies, explore one fp64 multiply and a clamp.  The reference of
an evolved call is the host loop it replaces: train `period` episodes with plain calls, evaluate on the held-out rows, apply
the NumPy restatement of a step (tests/pop_evolve_ref.py) to theta, w and the rates, go on.  Shapes: batch 13 (no multiple of a
tile), T = 3, N = 2 held-out files of L = 4 rows, repeats = 3, 8 episodes with period 2 (four checks); d = 21 and d = 15."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip('torch')

import guard_bands as GB
import pop_evolve_ref as R
import stream_order as S

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
B, T, N, LR, REP, E, PERIOD = 13, 3, 2, 4, 3, 8, 2
GAMMA = 0.9
EINVAL, EUNSUPPORTED = -1, -3
INF, NAN = float('inf'), float('nan')
FACTORS, CRITIC_BOUNDS, ACTOR_BOUNDS, SEED = (0.8, 1.25), (1e-6, 10.0), (1e-8, 1.0), 0xC0FFEE1234567


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.fail('-m gpu tests need a GPU')
    return torch.device(DEV)


@functools.lru_cache(maxsize=None)
def _emp(d):
    return np.random.RandomState(17 + d).dirichlet(np.ones(d), size=(N, LR))


def _pop(mode, d=21, K=5, configs=None, precision='mixed'):
    """K learners; configs: the number of distinct (theta, seed, w) configurations (None: K, all different) -- learner k
    gets configuration k % configs, so with few of them many learners are exact duplicates."""
    from discrete_mean_field_game_amd import ActorCriticPopulation
    n = K if configs is None else configs
    F = d * (d + 1) // 2 + d + 1
    idx = np.arange(K) % n
    thetas = np.linspace(8.2, 9.0, n)[idx]
    w0 = (np.random.RandomState(5).randn(n, F) * 0.1)[idx]
    return ActorCriticPopulation(thetas, 0.16, 12000.0, d, batch=B, seeds=[int(5 + 3 * j) for j in idx], w0=w0,
                                 pi0=np.random.RandomState(3).dirichlet(np.ones(d), size=9), update_every=mode,
                                 precision=precision, device=DEV, episode_steps=T)


def _rates(K):
    return np.linspace(0.05, 0.15, K), np.linspace(5e-4, 2e-3, K)


def _validation(pop, emp=None, **kw):
    from discrete_mean_field_game_amd.population import Validation
    kw.setdefault('period', PERIOD)
    return Validation(emp=_emp(pop.d) if emp is None else emp, repeats=REP, **kw)


def _evolution(**kw):
    from discrete_mean_field_game_amd.population import Evolution
    kw.setdefault('factors', FACTORS)
    kw.setdefault('lr_critic_bounds', CRITIC_BOUNDS)
    kw.setdefault('lr_actor_bounds', ACTOR_BOUNDS)
    kw.setdefault('seed', SEED)
    return Evolution(**kw)


def _train(pop, n, lrc, lra, first_episode=0, **kw):
    return pop.train(n, GAMMA, False, lrc, lra, first_episode=first_episode, **kw)


def _hour_mean(summary, col):
    """Columns 8 / 9 restated: summary [K, L, 2]; the hours 1 .. L-1 added in order in fp64, divided by L - 1."""
    out = np.zeros(summary.shape[0])
    for k in range(summary.shape[0]):
        s = np.float64(0.0)
        for l in range(1, summary.shape[1]):
            s = s + summary[k, l, col]
        out[k] = s / np.float64(summary.shape[1] - 1)
    return out


def _check_rows(pop, score):
    """One check on the host, with the validated call's Philox step 0: the row [K, 10] (NaN scores without `score`)."""
    from discrete_mean_field_game_amd import ops
    emp = _emp(pop.d)
    emp64 = torch.as_tensor(emp, dtype=torch.float64, device=DEV)
    emp32 = torch.as_tensor(emp.astype(np.float32), device=DEV)
    metrics, traj = ops.evaluate_pop(emp32, emp64, pop._theta, pop._shifts_dev, pop._alphas_dev, pop._seeds_dev, first_step=0,
                                     repeats=REP, precision=pop.precision, want_traj=True)
    row = np.full((pop.K, 10), NAN)
    row[:, :8] = metrics.cpu().numpy()
    if score:
        summary = ops.forecast_score(traj, emp32, emp64, N, REP, want_energy=True)['summary'].cpu().numpy()
        row[:, 8], row[:, 9] = _hour_mean(summary, 0), _hour_mean(summary, 1)
    return row


def _put(pop, theta, w):
    pop._theta.copy_(torch.as_tensor(theta, device=DEV))
    pop._w.copy_(torch.as_tensor(w, device=DEV))


def _host_loop(pop, col, every, n_top, n_bottom, perturb=3, score=False, stop=None, episodes=E, bounds=None):
    """The loop an evolved call replaces, from Philox step L - 1 on (the validated call's first training step).  stop: the
    stop criteria [K] of a controlled call -- the population resets `stopped` with every train() call, so a learner that
    stopped in an earlier round is put back to what it held (learners are independent) and takes no further part."""
    from discrete_mean_field_game_amd.population import STOPPED
    K = pop.K
    pop._rng_step = LR - 1
    lrc, lra = _rates(K)
    Cn = episodes // PERIOD
    S_ = Cn // every
    bounds = bounds or (CRITIC_BOUNDS, ACTOR_BOUNDS)
    best = [np.full(K, INF), np.full(K, -1, np.int32), np.zeros(K, np.int32), np.full(K, NAN),
            np.full((K, pop.w.shape[1]), NAN)]           # best_value | best_check | since_best | best_theta | best_w
    curve = np.full((K, Cn, 10), NAN)
    rank, parent, lr = np.full((K, S_), -1, np.int32), np.full((K, S_), -1, np.int32), np.full((K, S_, 2), NAN)
    stopped, episodes_run, acc = np.zeros(K, bool), np.zeros(K, np.int64), []
    for c in range(Cn):
        th0, w0 = pop.thetas, pop.w
        if stop is None:
            a = _train(pop, PERIOD, lrc, lra, first_episode=c * PERIOD)
        else:
            a = _train(pop, PERIOD, lrc, lra, first_episode=c * PERIOD, stop_criteria=stop)
            th1, w1 = pop.thetas, pop.w
            th1[stopped], w1[stopped], a[stopped] = th0[stopped], w0[stopped], 0.0
            _put(pop, th1, w1)
            episodes_run += np.where(stopped, 0, pop.episodes_run)
            stopped |= pop.learner_state == STOPPED
        acc.append(a)
        active = ~stopped
        row = _check_rows(pop, score)
        curve[active, c] = row[active]
        theta, w = pop.thetas, pop.w
        for k in np.flatnonzero(active):                 # k_pop_validate_select's best tracking (patience 0)
            if np.isfinite(row[k, col]) and row[k, col] < best[0][k]:
                best[0][k], best[1][k], best[2][k], best[3][k], best[4][k] = row[k, col], c, 0, theta[k], w[k]
            else:
                best[2][k] += 1
        if (c + 1) % every == 0:
            s = (c + 1) // every - 1
            out = R.step(row[:, col], active, theta, w, lrc, lra, s=s, seed=SEED, n_top=n_top, n_bottom=n_bottom, perturb=perturb,
                         factors=FACTORS, lr_critic_bounds=bounds[0], lr_actor_bounds=bounds[1], extra=best)
            best, lrc, lra = out['extra'], out['lr_critic'], out['lr_actor']
            rank[:, s], parent[:, s], lr[:, s] = out['rank'], out['parent'], out['lr']
            _put(pop, out['theta'], out['w'])
    return dict(theta=pop.thetas, w=pop.w, acc=np.concatenate(acc, 1), curve=curve, rank=rank, parent=parent, lr=lr, lrc=lrc,
                lra=lra, best=best, stopped=stopped, episodes_run=episodes_run, step=pop._rng_step)


def _compare(pop, acc, ref):
    v, e = pop.validation, pop.evolution
    assert np.array_equal(e.rank, ref['rank']) and np.array_equal(e.parent, ref['parent'])
    assert np.array_equal(e.lr, ref['lr'], equal_nan=True)
    assert np.array_equal(e.lr_critic, ref['lrc']) and np.array_equal(e.lr_actor, ref['lra'])
    assert np.array_equal(v.curve, ref['curve'], equal_nan=True)
    assert np.array_equal(pop.thetas, ref['theta']) and np.array_equal(pop.w, ref['w'])
    assert np.array_equal(acc, ref['acc']) and pop._rng_step == ref['step']
    assert np.array_equal(v.best_value, ref['best'][0]) and np.array_equal(v.best_check, ref['best'][1])
    assert np.array_equal(v.best_theta, ref['best'][3], equal_nan=True) and np.array_equal(v.best_w, ref['best'][4], equal_nan=True)


# --------------------------------------------------- 1. against the host loop it replaces
@pytest.mark.parametrize('mode,d,every,metric', [('step', 21, 1, 'JSD_mean'), ('rollout', 21, 2, 'JSD_mean'),
                                                 ('rollout', 15, 1, 'crps'), ('step', 15, 2, 'l1_final')])
def test_evolved_call_equals_the_host_loop(dev, mode, d, every, metric):
    from discrete_mean_field_game_amd.population import validation_column
    K, score, col = 5, metric == 'crps', validation_column(metric)
    ref = _host_loop(_pop(mode, d, K), col, every, 2, 2, score=score)
    pop = _pop(mode, d, K)
    lrc, lra = _rates(K)
    acc = _train(pop, E, lrc, lra, validate=_validation(pop, metric=metric, score=score), evolve=_evolution(every=every, top=2, bottom=2))
    e = pop.evolution
    Sn = E // PERIOD // every
    assert e.rank.shape == e.parent.shape == (K, Sn) and e.lr.shape == (K, Sn, 2)
    _compare(pop, acc, ref)
    # the steps did something: two receivers per step, one learner in neither set, every rank taken once
    assert all(sorted(e.rank[:, s]) == list(range(K)) for s in range(Sn))
    assert ((e.parent != np.arange(K)[:, None]).sum(0) == 2).all()
    assert not np.array_equal(e.lr_critic, lrc) and not np.array_equal(e.lr_actor, lra)
    for k in range(K):
        assert e.lineage(k)[-1] == k and e.rank[e.lineage(k)[0], 0] < 3
    # best-iterate inheritance: restore_best() on a receiver gives the best (theta, w) of its lineage
    pop.restore_best()
    assert np.array_equal(pop.thetas, ref['best'][3]) and np.array_equal(pop.w, ref['best'][4])
    assert pop.status() == 0


# --------------------------------------------------- 2. the rank kernel past one wave and one tile
@pytest.mark.parametrize('K,metric', [(70, 'JSD_mean'), (300, 'crps')])
def test_ranks_of_many_duplicates_past_a_wave_and_a_tile(dev, K, metric):
    from discrete_mean_field_game_amd.population import validation_column
    score, col = metric == 'crps', validation_column(metric)
    pop = _pop('rollout', 21, K, configs=4)
    lrc, lra = np.full(K, 0.1), np.full(K, 0.001)
    ev = _evolution(top=0.25, bottom=0.25)
    n_top, n_bottom = ev.counts(K)
    _train(pop, 2, lrc, lra, validate=_validation(pop, metric=metric, score=score), evolve=ev)
    v, e = pop.validation, pop.evolution
    values = v.curve[:, 0, col]
    assert len(set(values.tolist())) == 4                # exact duplicates: equal values, ranked by index
    # (the arrays the step read are gone; the ranks, the donors and the rates follow from the values alone)
    out = R.step(values, np.ones(K, bool), np.zeros(K), np.zeros((K, 1)), lrc, lra, s=0, seed=SEED, n_top=n_top, n_bottom=n_bottom,
                 factors=FACTORS, lr_critic_bounds=CRITIC_BOUNDS, lr_actor_bounds=ACTOR_BOUNDS)
    assert out['replaced']
    assert np.array_equal(e.rank[:, 0], out['rank']) and np.array_equal(e.parent[:, 0], out['parent'])
    assert np.array_equal(e.lr[:, 0], out['lr']) and np.array_equal(e.lr_critic, out['lr_critic'])
    assert np.array_equal(e.lr_actor, out['lr_actor'])
    assert sorted(e.rank[:, 0]) == list(range(K)) and (e.parent[:, 0] != np.arange(K)).sum() == n_bottom
    # a receiver holds its donor's parameters: the same as a plain validated run's learner `donor`
    plain = _pop('rollout', 21, K, configs=4)
    _train(plain, 2, lrc, lra, validate=_validation(plain, metric=metric, score=score))
    assert np.array_equal(pop.thetas, plain.thetas[e.parent[:, 0]]) and np.array_equal(pop.w, plain.w[e.parent[:, 0]])


# --------------------------------------------------- 3. with a control block
# Learner 0 stops after its first episode, ahead of every step.  Learner 3 is a receiver of step 0 (it is asserted below) and
# has a criterion between its own |theta_e - theta_{e-1}| of episodes 0 and 1 (step mode 3e-3, 1.6e-3; rollout mode 1.2e-3,
# 5.4e-4) and that of episode 2, its first with the donor's theta (5.2e-4; 1.8e-4): it stops after episode 2 exactly when
# theta_prev was moved to the donor's theta with it -- against its old theta the difference would be of the order of the
# learners' spacing, 0.2.  From then on three learners are active and the steps only log.
STOP = {'step': np.array([1e9, -1.0, -1.0, 8e-4, -1.0]), 'rollout': np.array([1e9, -1.0, -1.0, 3e-4, -1.0])}


@pytest.mark.parametrize('mode', ['step', 'rollout'])
def test_with_a_control_block(dev, mode):
    from discrete_mean_field_game_amd.population import STOPPED
    K = 5
    ref = _host_loop(_pop(mode, 21, K), 6, 1, 2, 2, stop=STOP[mode])
    pop = _pop(mode, 21, K)
    lrc, lra = _rates(K)
    acc = _train(pop, E, lrc, lra, validate=_validation(pop), evolve=_evolution(top=2, bottom=2), stop_criteria=STOP[mode])
    e = pop.evolution
    _compare(pop, acc, ref)
    # the retired learner is neither donor nor receiver and its log stays -1 / NaN
    assert pop.learner_state[0] == STOPPED and pop.episodes_run[0] == 1
    assert (e.rank[0] == -1).all() and (e.parent[0] == -1).all() and np.isnan(e.lr[0]).all() and not (e.parent[1:] == 0).any()
    assert e.lr_critic[0] == lrc[0] and e.lr_actor[0] == lra[0]
    # the next early-stop decisions are the host loop's
    assert np.array_equal(pop.learner_state == STOPPED, ref['stopped']) and np.array_equal(pop.episodes_run, ref['episodes_run'])
    assert e.parent[3, 0] != 3 and abs(pop.thetas[3] - np.linspace(8.2, 9.0, K)[3]) > 0.1      # a receiver of step 0 ...
    assert pop.learner_state.tolist() == [1, 0, 0, 1, 0] and pop.episodes_run.tolist() == [1, E, E, 3, E]   # ... that stops next
    assert (e.parent[3, 1:] == -1).all() and np.array_equal(e.parent[[1, 2, 4], 1:], np.array([[1], [2], [4]]).repeat(3, 1))
    # theta_prev of a receiver is its donor's theta: a call that ends on its one step leaves it there to be read
    short = _pop(mode, 21, K)
    _train(short, PERIOD, lrc, lra, validate=_validation(short), evolve=_evolution(top=2, bottom=2),
           stop_criteria=np.array([1e9, -1.0, -1.0, -1.0, -1.0]))
    got = short.evolution.parent[:, 0]
    assert got[0] == -1 and (got[1:] != np.arange(1, K)).sum() == 2
    prev = short._ctl['theta_prev'].cpu().numpy()
    assert np.array_equal(prev[1:], short.thetas[got[1:]]) and np.array_equal(prev[1:], short.thetas[1:])


# --------------------------------------------------- 4. skipped steps
def test_too_few_active_learners_only_log(dev):
    K = 3
    stop = np.array([1e9, -1.0, -1.0])
    lrc, lra = _rates(K)
    plain = _pop('rollout', 21, K)
    acc_plain = _train(plain, E, lrc, lra, validate=_validation(plain), stop_criteria=stop)
    pop = _pop('rollout', 21, K)
    acc = _train(pop, E, lrc, lra, validate=_validation(pop), evolve=_evolution(top=2, bottom=1), stop_criteria=stop)
    e = pop.evolution
    assert (e.parent[0] == -1).all() and (e.parent[1] == 1).all() and (e.parent[2] == 2).all()
    assert sorted(e.rank[1:, 0]) == [0, 1] and (e.rank[0] == -1).all()
    assert np.array_equal(e.lr[1:], np.broadcast_to(np.stack([lrc, lra], 1)[1:, None], (2, 4, 2))) and np.isnan(e.lr[0]).all()
    assert np.array_equal(e.lr_critic, lrc) and np.array_equal(e.lr_actor, lra)
    assert np.array_equal(pop.thetas, plain.thetas) and np.array_equal(pop.w, plain.w) and np.array_equal(acc, acc_plain)
    assert np.array_equal(pop.validation.curve, plain.validation.curve, equal_nan=True)


def test_non_finite_values_only_log(dev):
    """Held-out fp64 rows full of NaN and an L1 column (the fp32 rows, which the rollouts start from, stay as they are):
    every value is NaN, the steps only log, and theta, w and the rates are those of the call with the validation block alone."""
    a, b = S.Bufs(dev, 0), S.Bufs(dev, 0)
    with_steps, without = _raw_build(a, nan_emp64=True, column=2), _raw_build(b, nan_emp64=True, column=2, bind_evolve=False)
    torch.cuda.synchronize()
    with_steps()
    without()
    torch.cuda.synchronize()
    got, want = a.compared(), b.compared()
    assert torch.isnan(got['val_curve'][:, :, 2]).all() and torch.isfinite(got['val_curve'][:, :, 6]).all()
    assert torch.equal(got['evo_parent'], torch.arange(RAW_K, dtype=S.I32, device=dev)[:, None].expand(RAW_K, RAW_E))
    assert torch.equal(got['evo_rank'], got['evo_parent'])               # all values non-finite: index order
    assert (want['evo_rank'] == -1).all()
    for name in ('thetas', 'w', 'lr_critic', 'lr_actor', 'reward_acc', 'val_curve', 'val_best_check'):
        assert S.same(got[name], want[name]), name
    assert S.same(got['lr_critic'], a.f64(*np.linspace(0.05, 0.15, RAW_K)))
    assert S.same(got['evo_lr_log'][:, :, 0], got['lr_critic'][:, None].expand(RAW_K, RAW_E))


# --------------------------------------------------- 5. perturb=() and the clamp
def test_without_perturbation_the_donors_rates_are_copied(dev):
    K = 5
    lrc, lra = _rates(K)
    pop = _pop('step', 21, K)
    _train(pop, 2, lrc, lra, validate=_validation(pop), evolve=_evolution(top=2, bottom=2, perturb=()))
    e = pop.evolution
    assert (e.parent[:, 0] != np.arange(K)).sum() == 2
    assert np.array_equal(e.lr_critic, lrc[e.parent[:, 0]]) and np.array_equal(e.lr_actor, lra[e.parent[:, 0]])
    assert np.array_equal(e.lr[:, 0, 0], e.lr_critic) and np.array_equal(e.lr[:, 0, 1], e.lr_actor)


def test_a_rate_at_its_bound_stays_there(dev):
    """Bounds [lr, lr] for every learner's common rate: whichever factor the coin picks, the clamp puts the rate back."""
    K = 5
    lrc, lra = np.full(K, 0.1), np.full(K, 0.001)
    pop = _pop('rollout', 21, K)
    _train(pop, E, lrc, lra, validate=_validation(pop), evolve=_evolution(top=2, bottom=2, lr_critic_bounds=(0.1, 0.1),
                                                                       lr_actor_bounds=(0.001, 0.001)))
    e = pop.evolution
    assert (e.parent != np.arange(K)[:, None]).any()
    assert (e.lr[:, :, 0] == 0.1).all() and (e.lr[:, :, 1] == 0.001).all()
    assert np.array_equal(e.lr_critic, lrc) and np.array_equal(e.lr_actor, lra)
    # one-sided: from the upper bound a rate can only fall or stay; from the lower one only rise or stay
    ref = _host_loop(_pop('rollout', 21, K), 6, 1, 2, 2, bounds=((1e-6, 0.15), (5e-4, 1.0)))
    pop = _pop('rollout', 21, K)
    l0, l1 = _rates(K)                                   # (learner 4 starts at 0.15, learner 0 at 5e-4: their bounds)
    acc = _train(pop, E, l0, l1, validate=_validation(pop), evolve=_evolution(top=2, bottom=2, lr_critic_bounds=(1e-6, 0.15),
                                                                            lr_actor_bounds=(5e-4, 1.0)))
    _compare(pop, acc, ref)
    assert (pop.evolution.lr[:, :, 0] <= 0.15).all() and (pop.evolution.lr[:, :, 1] >= 5e-4).all()


# --------------------------------------------------- 6. refusals
def _raises(code, fn):
    from discrete_mean_field_game_amd._lib import MfgError
    with pytest.raises(MfgError) as e:
        fn()
    assert e.value.code == code, str(e.value)


def test_python_refusals(dev):
    from discrete_mean_field_game_amd import ActorCriticPopulation
    K = 5
    lrc, lra = _rates(K)
    pop = _pop('step', 21, K)
    before = (pop.thetas, pop.w, pop._rng_step)
    with pytest.raises(ValueError):
        _train(pop, E, lrc, lra, evolve=_evolution(top=2, bottom=2))                           # no validate
    with pytest.raises(ValueError):
        _train(pop, E, lrc, lra, validate=_validation(pop), evolve=_evolution(top=3, bottom=3))   # counts exceed K
    with pytest.raises(TypeError):
        _train(pop, E, lrc, lra, validate=_validation(pop), evolve=dict(every=1))
    assert np.array_equal(pop.thetas, before[0]) and np.array_equal(pop.w, before[1]) and pop._rng_step == before[2]
    assert pop.evolution is None
    res = ActorCriticPopulation(np.linspace(8.2, 9.0, K), 0.16, 12000.0, 21, batch=12, pi0=np.random.RandomState(3).dirichlet(
        np.ones(21), size=9), update_every='step', device=DEV, episode_steps=T, resident=True)
    with pytest.raises(ValueError):
        _train(res, E, lrc, lra, validate=_validation(res), evolve=_evolution(top=2, bottom=2))
    assert res._rng_step == 0


def _evolve_block(dev, K, S_=4):
    i32 = lambda *s: torch.full(s, -1, dtype=torch.int32, device=dev)
    return dict(order=i32(K), active=i32(1), rank=i32(K, S_), parent=i32(K, S_),
                lr_log=torch.full((K, S_, 2), NAN, dtype=torch.float64, device=dev))


@pytest.mark.parametrize('mode', ['step', 'rollout'])
def test_irl_population_calls_refuse_a_bound_block(dev, mode):
    from discrete_mean_field_game_amd.irl_population import AC_IRLPopulation
    from discrete_mean_field_game_amd.networks import RewardNet
    K, d = 3, 15
    nets = []
    for j in range(K):
        torch.manual_seed(40 + d + j)
        nets.append(RewardNet(d=d, n_fc3=8, n_fc4=4, keep_prob=0.4).to(DEV))
    F = d * (d + 1) // 2 + d + 1
    pop = AC_IRLPopulation(np.linspace(8.2, 9.0, K), 0.05, 1e4, d, batch=B, reward_nets=nets, seeds=[11, 18, 25],
                           w0=np.random.RandomState(5).randn(K, F) * 0.1, pi0=np.random.RandomState(3).dirichlet(np.ones(d), size=9),
                           update_every=mode, precision='mixed', device=DEV)
    before = (pop.thetas, pop.w)
    rates = torch.full((K,), 0.1, dtype=torch.float64, device=dev)
    blk = _evolve_block(dev, K)
    pop._ctx.set_pop_evolve(rates, rates.clone(), n_top=1, n_bottom=1, **blk)
    try:
        _raises(EUNSUPPORTED, lambda: pop.train(2, GAMMA, False, 0.1, 0.001))
    finally:
        pop._ctx.set_pop_evolve()
    torch.cuda.synchronize()
    assert np.array_equal(pop.thetas, before[0]) and np.array_equal(pop.w, before[1])      # nothing was launched
    assert (blk['rank'] == -1).all() and (blk['active'] == -1).all()
    pop.train(1, GAMMA, False, 0.1, 0.001)                                                  # (cleared: the call runs)
    assert not np.array_equal(pop.thetas, before[0])


# --------------------------------------------------- the raw call: a population entry with both blocks set by hand
RAW_K, RAW_E = 3, 3


def _default_make(a):
    def make(kind, name, shape, dtype, fill):
        if kind == 'out':
            return a.out(name, shape, dtype, keep=fill)
        if kind == 'io':
            return a.io(name, fill)
        return a.ws(int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size(), dtype, shape)
    return make


def _raw_build(a, make=None, entry='mfg_train_rollouts_pop', control=False, validate=True, max_steps=RAW_E, K_block=RAW_K,
               other_rates=False, evolve=None, column=6, nan_emp64=False, bind_evolve=True):
    """A Bufs builder: one evolved population call of RAW_E episodes (d = 21, K = 3, batch 13, T = 3; a check of N = 2, L = 4,
    repeats = 3 and a step with n_top = n_bottom = 1 after every episode).  make(kind, name, shape, dtype, fill) allocates the
    arrays a step writes (default: in the Bufs)."""
    ops, Lb = S._ops(), S._L()
    make = make or _default_make(a)
    K, d = RAW_K, 21
    F = ops.num_features(d)
    sb = ops.pop_workspace_slice(B, d, T)
    mat = a.inp('mat_pi0', a.simplex((S.NUM_START, d), 30))
    th, sh, al, sd = a.policies(K)
    del a.inputs['thetas']
    th = make('io', 'thetas', (K,), S.F64, th)
    if 'thetas' not in a.inputs:
        a.inputs['thetas'] = th                      # (a guarded theta still is an input a producer writes)
        a.written.append('thetas')
    w = make('io', 'w', (K, F), S.F64, a.randn64((K, F), d).abs_() * 0.1)
    if 'w' not in a.inputs:
        a.inputs['w'] = w
        a.written.append('w')
    G = a.out('G', (K, F + 3), S.F64)
    acc = a.io('reward_acc', torch.zeros(K, RAW_E, dtype=S.F64, device=a.dev) + a.salt)
    lrc = make('io', 'lr_critic', (K,), S.F64, a.f64(*np.linspace(0.05, 0.15, K)))
    lra = make('io', 'lr_actor', (K,), S.F64, a.f64(*np.linspace(5e-4, 2e-3, K)))
    for n, t in (('lr_critic', lrc), ('lr_actor', lra)):
        if n not in a.inputs:
            a.inputs[n] = t
            a.written.append(n)
    ws = a.ws(K * sb, S.F64, (K, sb // 8))
    emp = a.simplex((N, LR, d), 31)
    emp32, emp64 = a.inp('emp32', emp), a.inp('emp64', emp.double() * (NAN if nan_emp64 else 1.0))
    i32 = lambda v: torch.full((K,), v, dtype=S.I32, device=a.dev)
    val = dict(curve=a.out('val_curve', (K, RAW_E, 10), S.F64), checks=a.io('val_checks', i32(0)),
               best_value=a.io('val_best_value', torch.full((K,), INF, dtype=S.F64, device=a.dev)),
               best_check=a.io('val_best_check', i32(-1)), since_best=a.io('val_since_best', i32(0)),
               best_theta=a.out('val_best_theta', (K,), S.F64), best_w=a.out('val_best_w', (K, F), S.F64))
    vws = a.ws(ops.pop_validate_workspace_bytes(N, LR, d, K, REP, False))
    evo = dict(order=make('ws', 'evo_order', (K_block,), S.I32, 0), active=make('ws', 'evo_active', (1,), S.I32, 0),
               rank=make('out', 'evo_rank', (K_block, max_steps), S.I32, -1),
               parent=make('out', 'evo_parent', (K_block, max_steps), S.I32, -1),
               lr_log=make('out', 'evo_lr_log', (K_block, max_steps, 2), S.F64, NAN))
    ev_lrc, ev_lra = (lrc.clone(), lra.clone()) if other_rates else (lrc, lra)
    if K_block != K:
        ev_lrc = ev_lra = torch.full((K_block,), 0.1, dtype=S.F64, device=a.dev)
    ctx = ops.Context(a.dev)
    a.keep.append(ctx)
    if entry == 'mfg_train_rollouts_pop':
        traj, last, r, delta, g = S._rollout_outs(a, B, d, T, (K,))
        args = (S.p(mat), S.NUM_START, B, K, d, T, RAW_E, 0, 0, S.p(th), S.p(sh), S.p(al), S.p(w), GAMMA, Lb.REWARD_MFG_AC2,
                S.p(sd), 100, 1000, 0, S.p(lrc), S.p(lra), S.p(traj), S.p(last), S.p(r), S.p(delta), S.p(g), S.p(G), S.p(acc),
                S.p(ws), sb)
    else:       # the step-mode entries (per-step and resident): the same argument list
        pi = a.out('pi_io', (K, B, d))
        scratch, r, delta, g = S._episode_bufs(a, B, d, (K,))
        args = (S.p(mat), S.NUM_START, S.p(pi), S.p(scratch), B, K, d, T, RAW_E, 0, 0, S.p(th), S.p(sh), S.p(al), S.p(w), GAMMA,
                Lb.REWARD_MFG_AC2, S.p(sd), 100, 1000, Lb.PRECISION_MIXED, S.p(lrc), S.p(lra), S.p(r), S.p(delta), S.p(g), S.p(G),
                S.p(acc), S.p(ws), sb)
    if control:
        ctl = (a.io('ctl_state', torch.zeros(K, dtype=S.I32, device=a.dev)), a.io('ctl_status', torch.zeros(K, dtype=S.I32, device=a.dev)),
               a.out('ctl_theta_prev', (K,), S.F64), a.io('ctl_episodes_run', torch.zeros(K, dtype=S.I32, device=a.dev)),
               a.inp('ctl_stop_criteria', a.f64(-1.0, -1.0, -1.0)))

    def issue():
        before = ctx.bind_scoped()
        try:
            if control:
                ctx.set_pop_control(*ctl)
            if validate:
                ctx.set_pop_validate(emp32, emp64, period=1, column=column, first_step=7, repeats=REP, workspace=vws, **val)
            if bind_evolve:
                ctx.set_pop_evolve(ev_lrc, ev_lra, **dict(dict(n_top=1, n_bottom=1, seed=SEED), **(evolve or {})), **evo)
            S.call(entry, *args)
        finally:
            ctx.set_pop_evolve()
            ctx.set_pop_validate()
            ctx.set_pop_control()
            ctx.restore(before)
    a.evo = evo
    return issue


@pytest.mark.parametrize('code,kw', [(EINVAL, dict(validate=False)), (EINVAL, dict(other_rates=True)), (EINVAL, dict(max_steps=2)),
                                     (EINVAL, dict(K_block=2)), (EINVAL, dict(evolve=dict(every=0))),
                                     (EINVAL, dict(evolve=dict(n_top=0))), (EINVAL, dict(evolve=dict(n_bottom=0))),
                                     (EINVAL, dict(evolve=dict(n_top=2, n_bottom=2))), (EINVAL, dict(evolve=dict(perturb=4))),
                                     (EINVAL, dict(evolve=dict(factors=(0.0, 1.25)))), (EINVAL, dict(evolve=dict(factors=(0.8, INF)))),
                                     (EINVAL, dict(evolve=dict(lr_critic_bounds=(0.2, 0.1)))),
                                     (EINVAL, dict(evolve=dict(lr_actor_bounds=(0.0, 0.1)))),
                                     (EUNSUPPORTED, dict(entry='mfg_train_episodes_pop_resident', validate=False))])
def test_refusals_leave_everything_alone(dev, code, kw):
    a = S.Bufs(dev, 0)
    issue = _raw_build(a, **kw)
    before = {n: t.clone() for n, t in a.compared().items()}
    torch.cuda.synchronize()
    _raises(code, issue)
    torch.cuda.synchronize()
    assert not S.differing({n: t for n, t in a.compared().items()}, before)      # theta, w, rates, every log: untouched
    assert S._ops().status() == 0


# --------------------------------------------------- 7. stream order and write bounds
ROW = S.Row('train_rollouts_pop-evolve', ('mfg_train_rollouts_pop',), _raw_build)
ROW_STEP = S.Row('train_episodes_pop-evolve-control', ('mfg_train_episodes_pop',),
                 lambda a: _raw_build(a, entry='mfg_train_episodes_pop', control=True))


@pytest.fixture(scope='module')
def M(dev):
    class _M:
        pass
    S._ops().init()
    m = _M()
    m.ref = {r.name: S.reference(r, dev) for r in (ROW, ROW_STEP)}
    m.delay_ms = max(20.0, 10.0 * 1e3 * max(x.enqueue_s for x in m.ref.values()))
    m.cycles = int(m.delay_ms * S.sleep_cycles_per_ms())
    m.side = S.independent_side_stream(dev, m.cycles)
    return m


@pytest.mark.parametrize('r', [ROW, ROW_STEP], ids=lambda r: r.name)
def test_evolved_call_runs_behind_a_delayed_producer(dev, M, r):
    want = M.ref[r.name].want
    assert (want['evo_rank'] >= 0).all() and (want['evo_parent'] != torch.arange(RAW_K, device=dev)[:, None]).any()
    assert torch.isfinite(want['evo_lr_log']).all() and not S.same(want['lr_critic'], M.ref[r.name].true['lr_critic'])
    pending, got = S.run_delayed(r, M.ref[r.name], dev, M.cycles, M.side)
    assert pending, 'inconclusive: the producer (%.1f ms) had finished when the call returned, or the call waited for it' % M.delay_ms
    bad = S.differing(got, want)
    assert not bad, '%s differ from the default-stream run: part of the call ran ahead of the stream it was given' % bad


@pytest.mark.parametrize('r', [ROW, ROW_STEP], ids=lambda r: r.name)
def test_evolved_call_is_capturable_and_replays(dev, M, r):
    found = S.run_captured(r, M.ref[r.name], dev, M.side)
    assert not found, found


@pytest.mark.parametrize('entry', ['mfg_train_rollouts_pop', 'mfg_train_episodes_pop'])
def test_step_arrays_between_guard_bands(dev, entry):
    guarded = {}

    def make(kind, name, shape, dtype, fill):
        g = GB.Guarded(shape, dtype, dev, fill=fill)
        guarded[name] = g
        return g.t
    a = S.Bufs(dev, 0)
    issue = _raw_build(a, make=make, entry=entry)
    torch.cuda.synchronize()
    issue()
    torch.cuda.synchronize()
    assert sorted(guarded) == ['evo_active', 'evo_lr_log', 'evo_order', 'evo_parent', 'evo_rank', 'lr_actor', 'lr_critic', 'thetas', 'w']
    GB.check_all(*guarded.items())
    rank, parent = guarded['evo_rank'].t.cpu().numpy(), guarded['evo_parent'].t.cpu().numpy()
    assert all(sorted(rank[:, s]) == [0, 1, 2] for s in range(RAW_E)) and int(guarded['evo_active'].t[0]) == RAW_K
    assert ((parent != np.arange(RAW_K)[:, None]).sum(0) == 1).all()
    assert sorted(guarded['evo_order'].t.cpu().numpy()) == [0, 1, 2] and torch.isfinite(guarded['evo_lr_log'].t).all()
    assert torch.isfinite(guarded['thetas'].t).all() and torch.isfinite(guarded['w'].t).all()
