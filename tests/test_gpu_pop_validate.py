"""-m gpu: held-out validation inside a population training call (mfg_ctx_set_pop_validate; train(..., validate=...)).

Everything is compared bit for bit (array_equal).  The reference of a validated call is the host loop it replaces: train
`period` episodes, snapshot theta / w, ops.evaluate_pop with the block's first_step (and ops.forecast_score on the members of
that very call), repeat.  The only arithmetic the feature adds is the hour mean of columns 8 / 9 -- sequential fp64 adds and
one division --, which a NumPy loop restates exactly.  Shapes: K = 3, batch 13 (no multiple of a tile), T = 3, N = 2 held-out
files of L = 4 rows, repeats = 3, E = 7 episodes with period 2 (three checks, the last episode has none); d = 21 for
ActorCriticPopulation, d = 15 (and the class's T = 15) for AC_IRLPopulation."""
import ctypes as C
import functools

import numpy as np
import pytest

torch = pytest.importorskip('torch')

import guard_bands as GB
import stream_order as S

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
K, B, T, N, LR, R, E, PERIOD = 3, 13, 3, 2, 4, 3, 7, 2
GAMMA = 0.9
EINVAL, EUNSUPPORTED, EWORKSPACE = -1, -3, -4
INF, NAN = float('inf'), float('nan')


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.fail('-m gpu tests need a GPU')
    return torch.device(DEV)


def _table(d, seed=3):
    return np.random.RandomState(seed).dirichlet(np.ones(d), size=9)


def _w0(d, seed=5):
    return np.random.RandomState(seed).randn(K, d * (d + 1) // 2 + d + 1) * 0.1


@functools.lru_cache(maxsize=None)
def _emp(d):
    return np.random.RandomState(17 + d).dirichlet(np.ones(d), size=(N, LR))


@functools.lru_cache(maxsize=None)
def _nets(d):
    from discrete_mean_field_game_amd.networks import RewardNet
    out = []
    for j in range(K):
        torch.manual_seed(40 + d + j)
        net = RewardNet(d=d, n_fc3=8, n_fc4=4, keep_prob=0.4).to(DEV)
        with torch.no_grad():
            for p in net.parameters():
                if p.dim() == 1:
                    p.uniform_(-0.2, 0.2)
        out.append(net)
    return out


def _pop(cls, mode, precision, reward='mfg_ac2', thetas=None, seeds=None, w0=None):
    thetas = np.linspace(8.2, 9.0, K) if thetas is None else thetas
    if cls == 'irl':
        from discrete_mean_field_game_amd.irl_population import AC_IRLPopulation
        return AC_IRLPopulation(thetas, 0.05, 1e4, 15, batch=B, reward_nets=_nets(15), seeds=[11 + 7 * k for k in range(K)],
                                w0=_w0(15), pi0=_table(15), update_every=mode, precision=precision, device=DEV)     # (its episodes have the class's 15 steps)
    from discrete_mean_field_game_amd import ActorCriticPopulation
    return ActorCriticPopulation(thetas, 0.16, 12000.0, 21, batch=B, seeds=seeds or [5 + 3 * k for k in range(K)],
                                 w0=_w0(21) if w0 is None else w0,
                                 pi0=_table(21), update_every=mode, precision=precision, reward=reward, device=DEV,
                                 episode_steps=T)


def _train(pop, n, first_episode=0, lr_critic=0.1, lr_actor=0.001, **kw):
    return pop.train(n, GAMMA, False, lr_critic, lr_actor, first_episode=first_episode, **kw)


def _validation(pop, **kw):
    from discrete_mean_field_game_amd.population import Validation
    kw.setdefault('period', PERIOD)
    return Validation(emp=_emp(pop.d), repeats=R, **kw)


def _hour_mean(summary, col):
    """Columns 8 / 9 restated: summary [K, L, 2]; the hours 1 .. L-1 added in order in fp64, divided by L - 1."""
    out = np.zeros(summary.shape[0])
    for k in range(summary.shape[0]):
        s = np.float64(0.0)
        for l in range(1, summary.shape[1]):
            s = s + summary[k, l, col]
        out[k] = s / np.float64(summary.shape[1] - 1)
    return out


def _check_rows(pop, first_step):
    """One check on the host: (row [K, 10] with the scores, the same with NaN scores)."""
    from discrete_mean_field_game_amd import ops
    emp = _emp(pop.d)
    emp64 = torch.as_tensor(emp, dtype=torch.float64, device=DEV)
    emp32 = torch.as_tensor(emp.astype(np.float32), device=DEV)
    metrics, traj = ops.evaluate_pop(emp32, emp64, pop._theta, pop._shifts_dev, pop._alphas_dev, pop._seeds_dev,
                                     first_step=first_step, repeats=R, precision=pop.precision, want_traj=True)
    summary = ops.forecast_score(traj, emp32, emp64, N, R, want_energy=True)['summary'].cpu().numpy()
    row = np.concatenate([metrics.cpu().numpy(), _hour_mean(summary, 0)[:, None], _hour_mean(summary, 1)[:, None]], axis=1)
    assert np.isfinite(row).all()
    return row


@functools.lru_cache(maxsize=None)
def _chunked(cls, mode, precision, reward, period=PERIOD, episodes=E):
    """The host loop a validated call replaces, from Philox step L - 1 on (the validated call's first training step): per
    check the row [K, 10] and the theta / w snapshots; then the remaining episodes.  Computed once per configuration."""
    pop = _pop(cls, mode, precision, reward)
    pop._rng_step = LR - 1
    rows, thetas, ws, acc = [], [], [], []
    for c in range(episodes // period):
        acc.append(_train(pop, period, first_episode=c * period))
        thetas.append(pop.thetas)
        ws.append(pop.w)
        rows.append(_check_rows(pop, 0))
    rest = episodes % period
    if rest:
        acc.append(_train(pop, rest, first_episode=episodes - rest))
    return dict(rows=np.stack(rows, 1), thetas=np.stack(thetas, 1), ws=np.stack(ws, 1), acc=np.concatenate(acc, 1),
                theta=pop.thetas, w=pop.w, G=pop._bufs['G'].cpu().numpy(), step=pop._rng_step)


def _first_argmin(col):
    """NumPy's first arg-min over the finite entries of col [K, C] (-1 / +inf when a learner has none)."""
    masked = np.where(np.isfinite(col), col, INF)
    idx = np.argmin(masked, axis=1)
    val = masked[np.arange(col.shape[0]), idx]
    return np.where(np.isfinite(val), idx, -1), val


CASES = [('ac', 'step', 'mixed', 'mfg_ac2', 'JSD_mean'), ('ac', 'rollout', 'mixed', 'synthetic', 'crps'),
         ('ac', 'rollout', 'f64', 'mfg_ac2', 'l1_final'), ('ac', 'step', 'f64', 'synthetic', 'crps'),
         ('irl', 'step', 'mixed', None, 'l1_final'), ('irl', 'rollout', 'mixed', None, 'crps'),
         ('irl', 'rollout', 'f64', None, 'JSD_mean')]


# --------------------------------------------------- 1-3. non-interference, the curve, the best iterate, restore_best
@pytest.mark.parametrize('cls,mode,precision,reward,metric', CASES)
def test_validated_call_equals_the_host_loop(dev, cls, mode, precision, reward, metric):
    from discrete_mean_field_game_amd.population import validation_column
    score = metric == 'crps'
    # 1. the same call without validate, from the Philox step the validated call trains from
    plain = _pop(cls, mode, precision, reward)
    plain._rng_step = LR - 1
    acc_plain = _train(plain, E)
    pop = _pop(cls, mode, precision, reward)
    acc = _train(pop, E, validate=_validation(pop, metric=metric, score=score))
    assert pop._rng_step == plain._rng_step == LR - 1 + E * pop.episode_steps
    assert np.array_equal(acc, acc_plain)
    assert np.array_equal(pop.thetas, plain.thetas) and np.array_equal(pop.w, plain.w)
    assert np.array_equal(pop._bufs['G'].cpu().numpy(), plain._bufs['G'].cpu().numpy())
    assert np.array_equal(pop.learner_state, plain.learner_state) and np.array_equal(pop.episodes_run, plain.episodes_run)
    assert pop.status() == 0
    # 2. the chunked host loop is a reference: it ends where the single call ends
    ref = _chunked(cls, mode, precision, reward)
    assert np.array_equal(ref['theta'], pop.thetas) and np.array_equal(ref['w'], pop.w) and np.array_equal(ref['acc'], acc)
    assert np.array_equal(ref['G'], pop._bufs['G'].cpu().numpy()) and ref['step'] == pop._rng_step
    v = pop.validation
    Cn = E // PERIOD
    assert v.curve.shape == (K, Cn, 10) and np.array_equal(v.checks, [Cn] * K)
    assert np.array_equal(v.episodes, [2, 4, 6])
    assert np.array_equal(v.curve[:, :, :8], ref['rows'][:, :, :8])
    if score:
        assert np.array_equal(v.curve[:, :, 8:], ref['rows'][:, :, 8:])
    else:
        assert np.isnan(v.curve[:, :, 8:]).all()
    # 3. the best iterate: NumPy's first arg-min of the chosen column, the loop's snapshots at that check
    col = validation_column(metric)
    idx, val = _first_argmin(ref['rows'][:, :, col])
    assert (idx >= 0).all()
    assert np.array_equal(v.best_check, idx) and np.array_equal(v.best_value, val)
    assert np.array_equal(v.best_episode, (idx + 1) * PERIOD)
    assert np.array_equal(v.best_theta, ref['thetas'][np.arange(K), idx])
    assert np.array_equal(v.best_w, ref['ws'][np.arange(K), idx])
    pop.restore_best()
    assert np.array_equal(pop.thetas, ref['thetas'][np.arange(K), idx]) and np.array_equal(pop.w, ref['ws'][np.arange(K), idx])


def test_restore_best_of_one_learner_and_without_a_best(dev):
    pop = _pop('ac', 'rollout', 'mixed')
    with pytest.raises(ValueError):
        pop.restore_best()
    _train(pop, 1, validate=_validation(pop))           # (period 2: no check falls into the call)
    assert pop.validation.curve.shape == (K, 0, 10) and np.array_equal(pop.validation.best_check, [-1] * K)
    assert pop._rng_step == LR - 1 + T
    before = pop.thetas
    pop.restore_best()                                  # (nobody has a best: nothing moves)
    assert np.array_equal(pop.thetas, before)
    with pytest.raises(ValueError):
        pop.restore_best(1)
    _train(pop, 4, validate=_validation(pop))
    after, w_after = pop.thetas, pop.w
    pop.restore_best(1)
    want, want_w = after.copy(), w_after.copy()
    want[1], want_w[1] = pop.validation.best_theta[1], pop.validation.best_w[1]
    assert np.array_equal(pop.thetas, want) and np.array_equal(pop.w, want_w)


# --------------------------------------------------- 4. common random numbers and patience
def _patience_expected(col, patience):
    """The stop rule on the host, per learner over its period-1 curve column: (checks taken, stopped)."""
    best, since = INF, 0
    for c, x in enumerate(col):
        if np.isfinite(x) and x < best:
            best, since = x, 0
        else:
            since += 1
            if since >= patience:
                return c + 1, True
    return len(col), False


@pytest.mark.parametrize('mode', ['step', 'rollout'])
def test_common_random_numbers_and_patience(dev, mode):
    from discrete_mean_field_game_amd.population import ACTIVE, STOPPED
    lrc, lra = np.array([0.1, 0.0, 0.1]), np.array([0.001, 0.0, 0.001])
    # Learners 0 and 2 are meant to keep improving, so that only learner 1 runs out of patience: both train under seed 11 and
    # from learner 2's critic weights, with
    # which theta falls at every episode from 9.0 as from 9.2, and the held-out JSD falls with theta in this range.  (Whether
    # they do is not assumed: the expected stops below come from the free run's curve, and the last line asserts it.)
    start, seeds = np.array([9.2, np.linspace(8.2, 9.0, K)[1], 9.0]), (11, 8, 11)
    w_start = _w0(21)[[2, 1, 2]]
    free = _pop('ac', mode, 'mixed', thetas=start, seeds=seeds, w0=w_start)
    _train(free, E, lr_critic=lrc, lr_actor=lra, validate=_validation(free, period=1))
    vf = free.validation
    assert np.array_equal(vf.checks, [E] * K) and free.thetas[1] == start[1]
    # learner 1 never moves and every check draws the same random numbers: one row, E times, the same bits
    assert np.array_equal(vf.curve[1, :, :8], np.repeat(vf.curve[1, :1, :8], E, axis=0)) and np.isnan(vf.curve[:, :, 8:]).all()
    assert vf.best_check[1] == 0
    pop = _pop('ac', mode, 'mixed', thetas=start, seeds=seeds, w0=w_start)
    theta0, w0 = pop.thetas, pop.w
    acc = _train(pop, E, lr_critic=lrc, lr_actor=lra, validate=_validation(pop, period=1, patience=2))
    v = pop.validation
    want = [_patience_expected(vf.curve[k, :, 6], 2) for k in range(K)]
    assert want[1] == (3, True)                          # best at check 0, no improvement at checks 1 and 2
    assert pop.episodes_run[1] == 3 and pop.learner_state[1] == STOPPED
    assert np.array_equal(pop.episodes_run, [n for n, _ in want])
    assert np.array_equal(pop.learner_state, [STOPPED if s else ACTIVE for _, s in want])
    assert np.array_equal(v.checks, [n for n, _ in want])
    assert pop.thetas[1] == theta0[1] and np.array_equal(pop.w[1], w0[1]) and not acc[1, 3:].any()
    for k in range(K):
        n = want[k][0]
        assert np.array_equal(v.curve[k, :n, :8], vf.curve[k, :n, :8]) and np.isnan(v.curve[k, n:]).all()
    # learner independence: a learner that ran all E episodes holds what it holds without learner 1's stop
    full = [k for k in (0, 2) if want[k][0] == E]
    for k in full:
        assert pop.thetas[k] == free.thetas[k] and np.array_equal(pop.w[k], free.w[k])
        assert v.best_check[k] == vf.best_check[k] and v.best_value[k] == vf.best_value[k]
    assert full == [0, 2], 'learners 0 and 2 are meant to run all %d episodes: %r' % (E, want)


# --------------------------------------------------- 5. retired learners
def test_a_failed_learner_takes_no_part_in_the_checks(dev):
    from discrete_mean_field_game_amd.population import FAILED
    healthy = _pop('ac', 'rollout', 'mixed')
    _train(healthy, E, validate=_validation(healthy, metric='crps', score=True), isolate=True)
    start = np.linspace(8.2, 9.0, K)
    start[0] = NAN
    pop = _pop('ac', 'rollout', 'mixed', thetas=start)
    _train(pop, E, validate=_validation(pop, metric='crps', score=True), isolate=True)
    v, vh = pop.validation, healthy.validation
    assert pop.learner_state[0] == FAILED and pop.episodes_run[0] == 0
    assert v.checks[0] == 0 and np.isnan(v.curve[0]).all()          # the sentinel fill: nothing of learner 0 was touched
    assert v.best_value[0] == INF and v.best_check[0] == -1 and np.isnan(v.best_theta[0]) and np.isnan(v.best_w[0]).all()
    assert np.array_equal(v.checks[1:], [3, 3])
    for name in ('curve', 'best_value', 'best_check', 'best_theta', 'best_w'):
        assert np.array_equal(getattr(v, name)[1:], getattr(vh, name)[1:]), name
    assert np.array_equal(pop.thetas[1:], healthy.thetas[1:]) and np.array_equal(pop.w[1:], healthy.w[1:])
    with pytest.raises(ValueError):
        pop.restore_best(0)
    pop.restore_best()
    assert np.isnan(pop.thetas[0]) and np.array_equal(pop.thetas[1:], v.best_theta[1:])


# --------------------------------------------------- the raw call: mfg_train_rollouts_pop with a block set by hand
RAW_E = 3


def _default_make(a):
    def make(kind, name, shape, dtype, fill):
        if kind == 'out':
            return a.out(name, shape, dtype)
        if kind == 'io':
            return a.io(name, fill)
        return a.ws(shape[0])
    return make


def _raw_build(a, max_checks=RAW_E, make=None, column=8, with_score=True, patience=0, period=1, ws_short=0, K_block=K,
               control=False, entry='mfg_train_rollouts_pop', first_step=7):
    """A Bufs builder: one validated population call of RAW_E episodes (d = 21, K = 3, batch 13, T = 3; checks of N = 2, L = 4,
    repeats = 3).  make(kind, name, shape, dtype, fill) allocates the block's arrays and workspace (default: in the Bufs)."""
    ops, Lb = S._ops(), S._L()
    make = make or _default_make(a)
    d = 21
    F = ops.num_features(d)
    sb = ops.pop_workspace_slice(B, d, T)
    mat = a.inp('mat_pi0', a.simplex((S.NUM_START, d), 30))
    th, sh, al, sd = a.policies(K)
    a.written.append('thetas')
    w, G = a.w(d, True, (K,)), a.out('G', (K, F + 3), S.F64)
    acc = a.io('reward_acc', torch.zeros(K, RAW_E, dtype=S.F64, device=a.dev) + a.salt)
    lrc, lra = a.inp('lr_critic', a.f64(*np.linspace(0.05, 0.15, K))), a.inp('lr_actor', a.f64(*np.linspace(5e-4, 2e-3, K)))
    ws = a.ws(K * sb, S.F64, (K, sb // 8))
    emp = a.simplex((N, LR, d), 31)
    emp32, emp64 = a.inp('emp32', emp), a.inp('emp64', emp.double())
    i32 = lambda v: torch.full((K_block,), v, dtype=S.I32, device=a.dev)
    blk = dict(curve=make('out', 'val_curve', (K_block, max_checks, 10), S.F64, NAN),
               checks=make('io', 'val_checks', (K_block,), S.I32, i32(5 * a.salt)),          # (decoy: a full curve, valid)
               best_value=make('io', 'val_best_value', (K_block,), S.F64,
                               torch.full((K_block,), 0.0 if a.salt else INF, dtype=S.F64, device=a.dev)),
               best_check=make('io', 'val_best_check', (K_block,), S.I32, i32(4 if a.salt else -1)),
               since_best=make('io', 'val_since_best', (K_block,), S.I32, i32(a.salt)),
               best_theta=make('out', 'val_best_theta', (K_block,), S.F64, NAN),
               best_w=make('out', 'val_best_w', (K_block, F), S.F64, NAN))
    nbytes = ops.pop_validate_workspace_bytes(N, LR, d, K_block, R, with_score)
    vws = make('ws', 'val_workspace', (nbytes,), S.U8, 0)
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
            ctx.set_pop_validate(emp32, emp64, period=period, column=column, with_score=with_score, patience=patience,
                                 first_step=first_step, repeats=R, workspace=vws, workspace_bytes=nbytes - ws_short, **blk)
            S.call(entry, *args)
        finally:
            ctx.set_pop_validate()
            ctx.set_pop_control()
            ctx.restore(before)
    a.blk = blk
    return issue


def _run_raw(dev, **kw):
    a = S.Bufs(dev, 0)
    issue = _raw_build(a, **kw)
    torch.cuda.synchronize()
    issue()
    torch.cuda.synchronize()
    return a


# --------------------------------------------------- 6. capacity
def test_curve_capacity(dev):
    full = _run_raw(dev)
    short = _run_raw(dev, max_checks=2)
    cf, cs = full.blk['curve'].cpu().numpy(), short.blk['curve'].cpu().numpy()
    assert np.isfinite(cf).all() and cf.shape == (K, 3, 10) and cs.shape == (K, 2, 10)
    assert np.array_equal(short.blk['checks'].cpu().numpy(), [3] * K)         # three checks ran,
    assert np.array_equal(cs, cf[:, :2])                                     # two rows were written,
    idx, val = _first_argmin(cf[:, :, 8])                                    # and the best tracking covers all three
    for name, want in (('best_check', idx), ('best_value', val)):
        assert np.array_equal(short.blk[name].cpu().numpy(), want), name
    for name in ('best_check', 'best_value', 'best_theta', 'best_w', 'since_best'):
        assert S.same(short.blk[name], full.blk[name]), name
    for name in ('thetas', 'w', 'reward_acc'):
        assert S.same(short.inputs[name], full.inputs[name]), name


# --------------------------------------------------- 7. refusals
def _raises(code, fn):
    from discrete_mean_field_game_amd._lib import MfgError
    with pytest.raises(MfgError) as e:
        fn()
    assert e.value.code == code, str(e.value)


@pytest.mark.parametrize('code,kw', [(EINVAL, dict(period=0)), (EINVAL, dict(max_checks=0)), (EINVAL, dict(patience=-1)),
                                     (EINVAL, dict(column=10)), (EINVAL, dict(column=-1)),
                                     (EINVAL, dict(column=8, with_score=False)), (EINVAL, dict(column=9, with_score=False)),
                                     (EINVAL, dict(first_step=0xFFFFFFFF - LR + 2)),
                                     # checked again before the call launches anything
                                     (EINVAL, dict(K_block=2)), (EINVAL, dict(patience=2)), (EWORKSPACE, dict(ws_short=8)),
                                     (EWORKSPACE, dict(ws_short=8, with_score=False, column=6)),
                                     (EUNSUPPORTED, dict(entry='mfg_train_episodes_pop_resident'))])
def test_refusals_leave_everything_alone(dev, code, kw):
    a = S.Bufs(dev, 0)
    issue = _raw_build(a, **kw)       # (max_checks = 0: a [K, 0, 10] curve has no address either -- MFG_EINVAL both ways)
    before = {n: t.clone() for n, t in a.compared().items()}
    torch.cuda.synchronize()
    _raises(code, issue)
    torch.cuda.synchronize()
    assert not S.differing({n: t for n, t in a.compared().items()}, before)      # theta, w, every output: untouched
    assert S._ops().status() == 0


def test_set_time_refusals_of_the_shape_and_of_null_pointers(dev):
    from discrete_mean_field_game_amd import _lib, ops
    ctx = ops.Context(dev)
    d, F = 21, ops.num_features(21)
    f64 = lambda *s: torch.zeros(*s, dtype=torch.float64, device=dev)
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32, device=dev)
    blk = dict(curve=f64(K, 3, 10), checks=i32(K), best_value=f64(K), best_check=i32(K), since_best=i32(K), best_theta=f64(K),
               best_w=f64(K, F), workspace=f64(1 << 16))

    def set_(n, l, **kw):
        emp = torch.full((n, l, d), 1.0 / d, dtype=torch.float32, device=dev)
        ctx.set_pop_validate(emp, emp.double(), **dict(blk, **kw))
    set_(N, LR)                                               # (the block itself is fine)
    _raises(EINVAL, lambda: set_(N, 1))                       # L < 2
    _raises(EINVAL, lambda: set_(0, LR))                      # N < 1
    _raises(EINVAL, lambda: set_(N, LR, repeats=0))
    _raises(EUNSUPPORTED, lambda: set_(N, LR, repeats=_lib.FORECAST_MAX_REPEATS + 1, with_score=True, column=8))
    set_(N, LR, repeats=_lib.FORECAST_MAX_REPEATS + 1)        # (without the scores the cap does not apply)
    # K outside [1, MFG_POP_MAX_K] and a null pointer: through the struct, ops would not build such a block
    emp = torch.full((N, LR, d), 1.0 / d, dtype=torch.float32, device=dev)
    e64 = emp.double()
    ptrs = [emp.data_ptr(), e64.data_ptr()] + [blk[n].data_ptr() for n in ('curve', 'checks', 'best_value', 'best_check',
                                                                            'since_best', 'best_theta', 'best_w', 'workspace')]
    tail = [1 << 19, N, LR, 1, 1, 6, 0, 0, 3]
    lib = _lib.lib()
    assert lib.mfg_ctx_set_pop_validate(ctx._ptr, C.byref(_lib.PopValidateStruct(*ptrs, *tail, K, 0))) == 0
    for bad_K in (0, _lib.POP_MAX_K + 1):
        assert lib.mfg_ctx_set_pop_validate(ctx._ptr, C.byref(_lib.PopValidateStruct(*ptrs, *tail, bad_K, 0))) == EINVAL
    for j in range(len(ptrs)):
        q = list(ptrs)
        q[j] = 0
        assert lib.mfg_ctx_set_pop_validate(ctx._ptr, C.byref(_lib.PopValidateStruct(*q, *tail, K, 0))) == EINVAL, j
    ctx.set_pop_validate()
    ctx.close()


# --------------------------------------------------- 8. stream order and write bounds
ROW = S.Row('train_rollouts_pop-validate', ('mfg_train_rollouts_pop',), _raw_build)
ROW_CTL = S.Row('train_rollouts_pop-validate-control', ('mfg_train_rollouts_pop',),
                lambda a: _raw_build(a, control=True, patience=2, column=6))


@pytest.fixture(scope='module')
def M(dev):
    class _M:
        pass
    S._ops().init()
    m = _M()
    m.ref = {r.name: S.reference(r, dev) for r in (ROW, ROW_CTL)}
    m.delay_ms = max(20.0, 10.0 * 1e3 * max(x.enqueue_s for x in m.ref.values()))
    m.cycles = int(m.delay_ms * S.sleep_cycles_per_ms())
    m.side = S.independent_side_stream(dev, m.cycles)
    return m


@pytest.mark.parametrize('r', [ROW, ROW_CTL], ids=lambda r: r.name)
def test_validated_call_runs_behind_a_delayed_producer(dev, M, r):
    want = M.ref[r.name].want
    assert torch.isfinite(want['val_curve']).all() and (want['val_checks'] == RAW_E).all()
    pending, got = S.run_delayed(r, M.ref[r.name], dev, M.cycles, M.side)
    assert pending, 'inconclusive: the producer (%.1f ms) had finished when the call returned, or the call waited for it' % M.delay_ms
    bad = S.differing(got, want)
    assert not bad, '%s differ from the default-stream run: part of the call ran ahead of the stream it was given' % bad


@pytest.mark.parametrize('r', [ROW, ROW_CTL], ids=lambda r: r.name)
def test_validated_call_is_capturable_and_replays(dev, M, r):
    found = S.run_captured(r, M.ref[r.name], dev, M.side)
    assert not found, found


@pytest.mark.parametrize('with_score', [True, False])
def test_block_arrays_and_workspace_between_guard_bands(dev, with_score):
    guarded = {}

    def make(kind, name, shape, dtype, fill):
        g = GB.Guarded(shape, dtype, dev, fill=fill if kind != 'ws' else 0)
        guarded[name] = g
        return g.t
    a = S.Bufs(dev, 0)
    issue = _raw_build(a, make=make, with_score=with_score, column=8 if with_score else 0)
    torch.cuda.synchronize()
    issue()
    torch.cuda.synchronize()
    assert len(guarded) == 8
    GB.check_all(*guarded.items())
    curve = guarded['val_curve'].t
    assert torch.isfinite(curve[:, :, :8]).all() and bool(torch.isfinite(curve[:, :, 8:]).all()) == with_score
    assert bool(torch.isnan(curve[:, :, 8:]).all()) != with_score
    assert (guarded['val_checks'].t == RAW_E).all() and (guarded['val_best_check'].t >= 0).all()
    for name in ('val_best_value', 'val_best_theta', 'val_best_w'):
        assert torch.isfinite(guarded[name].t).all(), name
