"""-m gpu: the backward-equation check of K policies (mfg_consistency_given / mfg_consistency_pop, ops.consistency_*,
population.consistency, ActorCriticPopulation.evaluate_synthetic(_JSD), mfg_synthetic.sweep).

The per-hour values and V match oracle.mfg_oracle.evaluate_synthetic_diffs on the same fp32 actions within the bounds the
project pins for this computation (test_backward_value_kernel_vs_reference_golden: V rtol 1e-12 / atol 1e-13, l1 rtol 1e-12,
jsd rtol 1e-10); the metrics match np.mean / np.std of the steps the same call returned; the rollout form's actions and states
are those of single ops.rollout calls; learner k's row does not depend on K; bad arguments are refused before anything is
launched; the classes give what population.consistency gives at their learners' parameters, seeds and Philox step.
"""
import ctypes as C
import functools
import os

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

EINVAL, EUNSUPPORTED, EWORKSPACE = -1, -3, -4
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.fail('-m gpu tests need a GPU')
    from discrete_mean_field_game_amd import ops
    ops.init()
    return torch.device('cuda', 0)


def _O():
    from oracle import mfg_oracle
    return mfg_oracle


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64 if a.dtype == np.float64 else np.int32)


def _freeze(res):
    for v in res.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return res


def _check_steps(steps, V, P, what):
    """steps [..., T, 2] and V [..., T+1, d] (or None) against the oracle on the same fp32 actions, with the pinned bounds."""
    Vo, l1o, jso = _O().evaluate_synthetic_diffs(P)
    checks = [('l1', steps[..., 0], l1o, 1e-12, 0.0), ('jsd', steps[..., 1], jso, 1e-10, 0.0)]
    if V is not None:
        checks.append(('V', V, Vo, 1e-12, 1e-13))
    for name, got, ref, rtol, atol in checks:
        assert got.shape == ref.shape, (what, name)
        assert not np.isnan(got).any(), (what, name)
        err = np.abs(got - ref)
        bound = atol + rtol * np.abs(ref)
        ratio = err / np.where(bound > 0, bound, 1.0)
        ratio = np.where((bound == 0) & (err == 0), 0.0, ratio)
        k = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
        print('%s %s: worst |got - ref| = %.3e at bound %.3e' % (what, name, err[k], bound[k]))
        assert np.allclose(got, ref, rtol=rtol, atol=atol), (what, name)


# ------------------------------------------------------------------------------------------------- 1. given actions
def _cap(dev):
    """Trajectories one pass of the backward kernel's capped grid covers: 8 blocks per CU of 4 waves (d <= 62)."""
    from discrete_mean_field_game_amd import _lib as L
    cu = C.c_int(0)
    L.check(L.lib().mfg_device_info(C.byref(cu), None, 0), 'mfg_device_info')
    assert cu.value > 0
    return 8 * cu.value * 4


@functools.lru_cache(maxsize=None)
def _given(d, T, K, M, conc):
    """One ops.consistency_given call with steps and V, as NumPy arrays (shared by the tests: computed once, never changed).
    Rows are Dirichlet(conc) (0.05: near one-hot, underflows to exact zeros in fp32); trajectory 0 and the last one have
    exact zeros planted in every row."""
    from discrete_mean_field_game_amd import ops
    dev = torch.device('cuda', 0)
    rs = np.random.RandomState(900 + 7 * d + T + K + M)
    P = rs.dirichlet(np.ones(d) * conc, size=(K * M, T, d)).astype(np.float32)
    if d > 1:
        for b in sorted({0, K * M - 1}):
            P[b, :, np.arange(d), (np.arange(d) + 1) % d] = 0.0
            P[b, 0, 0, 0] = 0.0
    P = P.reshape(K, M, T, d, d)
    Pd = torch.as_tensor(P, device=dev)
    out = ops.consistency_given(Pd)
    res = {k: v.cpu().numpy() for k, v in out.items()}
    res['P'] = P
    res['P_dev'] = Pd
    return _freeze(res)


GIVEN_CASES = [(d, T, conc) for d in (5, 15, 21, 33, 64) for T in (1, 3, 15) for conc in (1.0, 0.05)]


@pytest.mark.parametrize('d,T,conc', GIVEN_CASES)
def test_given_actions_against_oracle(dev, d, T, conc):
    from discrete_mean_field_game_amd import ops
    K, M = 3, 7
    g = _given(d, T, K, M, conc)
    assert g['steps'].shape == (K, M, T, 2) and g['V'].shape == (K, M, T + 1, d) and g['metrics'].shape == (K, 4)
    _check_steps(g['steps'], g['V'], g['P'], 'd=%d T=%d conc=%g' % (d, T, conc))
    assert not np.isnan(g['metrics']).any()
    assert np.array_equal(g['V'][:, :, T], np.zeros((K, M, d)))            # V^T = 0 is written too
    # without V, without steps, without both: the same metrics bits (and the same steps bits)
    for want_steps, want_V in ((True, False), (False, True), (False, False)):
        o = ops.consistency_given(g['P_dev'], want_steps=want_steps, want_V=want_V)
        assert (o['steps'] is None) == (not want_steps) and (o['V'] is None) == (not want_V)
        assert np.array_equal(_bits(o['metrics'].cpu().numpy()), _bits(g['metrics'])), (want_steps, want_V)
        if want_steps:
            assert np.array_equal(_bits(o['steps'].cpu().numpy()), _bits(g['steps']))
        if want_V:
            assert np.array_equal(_bits(o['V'].cpu().numpy()), _bits(g['V']))


def test_given_actions_past_the_grid_cap(dev):
    """K M = 2 cap + 3 (or a little more) trajectories: two full passes of the capped grid and a ragged third."""
    K, T, d = 3, 2, 5
    M = -(-(2 * _cap(dev) + 3) // K)
    g = _given(d, T, K, M, 1.0)
    _check_steps(g['steps'], g['V'], g['P'], 'past the cap, K M = %d' % (K * M))
    _check_metrics(g, 'past the cap')


# ---------------------------------------------------------------------------------------------------- 2. the reduction
def _check_metrics(g, what):
    """metrics against np.mean / np.std (ddof = 0) of the steps the same call returned.  Mean: rtol 1e-12 (n eps of up to a
    few ten thousand positive terms stays far below).  Std: |got - ref| <= 1e-9 ref + 1e-13 mean -- the spread is small
    against the mean (std / mean ~ 1e-4 in the reference regime), so a deviation carries a relative rounding error of about
    eps mean / std; a two-pass sum is insensitive to the error of the mean in first order."""
    K = g['steps'].shape[0]
    vals = g['steps'].reshape(K, -1, 2)
    for q, name in ((0, 'l1'), (1, 'jsd')):
        mean, std = np.mean(vals[:, :, q], axis=1), np.std(vals[:, :, q], axis=1)
        got_mean, got_std = g['metrics'][:, 2 * q], g['metrics'][:, 2 * q + 1]
        print('%s %s: max rel mean error %.3e, max std excess %.3e' % (
            what, name, np.max(np.abs(got_mean - mean) / np.abs(mean)), np.max(np.abs(got_std - std) - 1e-9 * std - 1e-13 * mean)))
        assert np.all(np.isfinite(g['metrics']))
        assert np.allclose(got_mean, mean, rtol=1e-12, atol=0.0), (what, name)
        assert np.all(np.abs(got_std - std) <= 1e-9 * std + 1e-13 * np.abs(mean)), (what, name)


@pytest.mark.parametrize('d,T,K,M,conc', [(21, 15, 3, 7, 1.0), (21, 15, 3, 7, 0.05), (15, 3, 3, 7, 1.0), (64, 15, 3, 7, 1.0),
                                          (21, 15, 2, 1, 1.0), (21, 15, 2, 26, 1.0), (5, 3, 2, 300, 1.0), (21, 3, 1, 5, 0.05)])
def test_metrics_are_mean_and_std_of_the_steps(dev, d, T, K, M, conc):
    _check_metrics(_given(d, T, K, M, conc), 'd=%d T=%d K=%d M=%d' % (d, T, K, M))


@pytest.mark.parametrize('d', [5, 21, 64])
def test_one_value_has_std_zero(dev, d):
    g = _given(d, 1, 3, 1, 1.0)                                            # M T = 1: the mean is the value, the std 0 exactly
    assert np.array_equal(g['metrics'][:, [0, 2]], g['steps'][:, 0, 0, :])
    assert np.array_equal(g['metrics'][:, [1, 3]], np.zeros((3, 2)))


def test_golden_anchor(dev):
    """The actions captured from the unmodified reference, each array one group: its returned mean and std within the bounds
    of test_backward_value_kernel_vs_reference_golden (1e-5 relative on the mean, 1e-4 relative + 1e-9 on the std)."""
    from discrete_mean_field_game_amd import ops
    z = np.load(os.path.join(G, 'backward_value_mfg_synthetic.npz'))
    for key, mean_k, std_k, col in (('actions_l1', 'l1_mean', 'l1_std', 0), ('actions_jsd', 'jsd_mean', 'jsd_std', 2)):
        acts = np.ascontiguousarray(z[key].astype(np.float32))[None]
        out = ops.consistency_given(torch.as_tensor(acts, device=dev))
        _check_steps(out['steps'].cpu().numpy(), out['V'].cpu().numpy(), acts, key)
        m = out['metrics'].cpu().numpy()[0]
        assert abs(m[col] - float(z[mean_k])) < 1e-5 * abs(float(z[mean_k]))
        assert abs(m[col + 1] - float(z[std_k])) < 1e-4 * abs(float(z[std_k])) + 1e-9


# ------------------------------------------------------------------------------------------------------ 3. rollout form
def _starts(d, N, seed):
    """N start rows as the files hold them ('%.3e' text), one exact zero included."""
    rs = np.random.RandomState(seed)
    m = np.array([[float('%.3e' % v) for v in row] for row in rs.dirichlet(np.ones(d), size=N)])
    m[0, d // 2] = 0.0
    return m


def _policies(K, seed):
    """The synthetic sweep's regime (theta in [1, 5], shift in [0, 0.02], alpha_scale 10 000); learners 0 and 1 identical in
    policy and seed."""
    rs = np.random.RandomState(seed)
    seeds = rs.randint(0, 2 ** 40, K).astype(np.int64)
    th, sh, al = rs.uniform(1.0, 5.0, K), rs.uniform(0.0, 0.02, K), np.full(K, 10000.0)
    if K > 1:
        seeds[1], th[1], sh[1] = seeds[0], th[0], sh[0]
    return th, sh, al, seeds


def _dev_args(dev, th, sh, al, sd):
    f = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=dev)
    return f(th), f(sh), f(al), torch.as_tensor(np.ascontiguousarray(sd, dtype=np.int64), device=dev)


@functools.lru_cache(maxsize=None)
def _rolled(d, precision, N, R, H, first_step, K=3):
    """One ops.consistency_pop call with everything it can return (shared by the tests: computed once, never changed)."""
    from discrete_mean_field_game_amd import ops
    dev = torch.device('cuda', 0)
    start = _starts(d, N, 40 + d + N)
    th, sh, al, sd = _policies(K, d + K)
    start32 = torch.as_tensor(start.astype(np.float32), device=dev)
    out = ops.consistency_pop(start32, *_dev_args(dev, th, sh, al, sd), H, first_step=first_step, repeats=R, precision=precision,
                              want_steps=True, want_V=True, want_actions=True, want_traj=True)
    res = {k: v.cpu().numpy() for k, v in out.items()}
    res.update(start=start, start32=start32, policies=(th, sh, al, sd), actions_dev=out['actions'], traj_dev=out['traj'])
    return _freeze(res)


ROLL_CASES = [(d, p, N, R, H, fs) for d in (21, 15, 5) for p in ('mixed', 'f64') for N, R in ((3, 2), (5, 5)) for H in (2, 16)
              for fs in (0, 37)]


@pytest.mark.parametrize('d,precision,N,R,H,first_step', ROLL_CASES)
def test_rollout_form(dev, d, precision, N, R, H, first_step):
    from discrete_mean_field_game_amd import ops
    K, T = 3, H - 1
    ops.clear_status()
    r = _rolled(d, precision, N, R, H, first_step)
    assert ops.status(synchronize=True) == 0
    th, sh, al, sd = r['policies']
    assert r['actions'].shape == (K, N * R, T, d, d) and r['traj'].shape == (K, N * R, H, d)
    assert r['steps'].shape == (K, N * R, T, 2) and r['V'].shape == (K, N * R, H, d) and r['metrics'].shape == (K, 4)
    # actions and states: single rollouts over the R-fold tiled start rows, per learner
    tiled = torch.as_tensor(np.tile(r['start'], (R, 1)).astype(np.float32), device=dev)
    for k in range(K):
        ref = ops.rollout(tiled, T, torch.tensor([th[k]], dtype=torch.float64, device=dev), float(sh[k]), float(al[k]),
                          seed=int(sd[k]), first_step=first_step, td=False, write_P=True, reward_kind=1, precision=precision)
        assert torch.equal(r['actions_dev'][k], ref['P']), 'actions of learner %d' % k
        assert torch.equal(r['traj_dev'][k], ref['pi_traj']), 'states of learner %d' % k
    # the check itself, on the returned actions
    _check_steps(r['steps'], r['V'], r['actions'], 'd=%d %s N=%d R=%d H=%d' % (d, precision, N, R, H))
    _check_metrics(r, 'rollout form')
    # the same policy on the same seed; another policy
    for key in ('metrics', 'steps', 'V', 'actions', 'traj'):
        assert np.array_equal(_bits(r[key][0]), _bits(r[key][1])), key
    assert not np.array_equal(r['actions'][0], r['actions'][2])
    # learner k alone (K = 1) and the whole call again: equal bits; nothing asked for beyond the metrics: the same metrics
    for k in (0, 2):
        alone = ops.consistency_pop(r['start32'], *_dev_args(dev, th[k:k + 1], sh[k:k + 1], al[k:k + 1], sd[k:k + 1]), H,
                                    first_step=first_step, repeats=R, precision=precision, want_steps=True)
        assert alone['V'] is None and alone['actions'] is None and alone['traj'] is None
        assert np.array_equal(_bits(alone['metrics'].cpu().numpy()[0]), _bits(r['metrics'][k])), k
        assert np.array_equal(_bits(alone['steps'].cpu().numpy()[0]), _bits(r['steps'][k])), k
    again = ops.consistency_pop(r['start32'], *_dev_args(dev, th, sh, al, sd), H, first_step=first_step, repeats=R,
                                precision=precision)
    assert again['steps'] is None
    assert np.array_equal(_bits(again['metrics'].cpu().numpy()), _bits(r['metrics']))
    assert ops.status(synchronize=True) == 0


def test_mixed_range_raises_on_its_own_context(dev):
    from discrete_mean_field_game_amd import _lib, ops, population
    ops.clear_status()
    pi0 = _starts(21, 2, 3)
    args = ([2.0, 150.0], 0.5, 1e4, pi0)             # 150 (1 + 0.5) > 86: beyond mixed precision's fp32 range
    with pytest.raises(_lib.MfgError):
        population.consistency(*args, d=21, hours=4, repeats=3)
    assert ops.status(synchronize=True) == 0         # the caller's status word is left alone
    res = population.consistency(*args, d=21, hours=4, repeats=3, precision='f64', want_steps=True)
    assert res.steps.shape == (2, 6, 3, 2) and np.all(np.isfinite(res.metrics)) and res.jsd_mean.shape == (2,)


def test_population_consistency_chunks_and_common_random_numbers(dev, monkeypatch):
    from discrete_mean_field_game_amd import ops, population
    pi0 = _starts(21, 3, 9)
    th = [1.0, 2.5, 2.5, 4.5, 0.0]
    kw = dict(d=21, seed=12345, hours=5, repeats=2, want_steps=True)
    whole = population.consistency(th, 0.01, 1e4, pi0, **kw)
    assert whole.steps.shape == (5, 6, 4, 2) and whole.l1_mean.shape == (5,)
    assert np.array_equal(whole.metrics[1], whole.metrics[2]) and not np.array_equal(whole.metrics[1], whole.metrics[3])
    per = ops.consistency_pop_workspace_bytes(3, 5, 21, 1, 2, True)
    monkeypatch.setattr(population, 'CONSISTENCY_BUDGET', 2 * per + 1)
    assert population.consistency_chunks(5, per, population.CONSISTENCY_BUDGET) == [(0, 2), (2, 2), (4, 1)]
    parts = population.consistency(th, 0.01, 1e4, pi0, **kw)
    assert np.array_equal(_bits(parts.metrics), _bits(whole.metrics)) and np.array_equal(_bits(parts.steps), _bits(whole.steps))
    monkeypatch.setattr(population, 'CONSISTENCY_BUDGET', per - 1)
    with pytest.raises(ValueError):
        population.consistency(th, 0.01, 1e4, pi0, **kw)


# ----------------------------------------------------------------------------------------------------------- 4. refusals
def _raw(dev, entry, **kw):
    """One of the two entries through the binding with real device buffers that hold NaN; returns (code, outputs)."""
    from discrete_mean_field_game_amd import _lib, ops
    d, K, N, R, H = 21, 2, 3, 2, 4
    a = dict(d=d, K=K, N=N, R=R, H=H, first_step=0, null=None, short=0, precision=1)
    a.update(kw)
    T, NR = H - 1, N * R
    nan = lambda shape, dt=torch.float64: torch.full(shape, float('nan'), dtype=dt, device=dev)
    bufs = {'metrics': nan((K, 4)), 'steps': nan((K, NR, T, 2)), 'V': nan((K, NR, H, d))}
    ptr = lambda name, t: None if a['null'] == name else t.data_ptr()
    h = _lib.lib()
    if entry == 'given':
        P = torch.as_tensor(np.random.RandomState(1).dirichlet(np.ones(d), size=(K, NR, T, d)).astype(np.float32), device=dev)
        ws = torch.empty(max(h.mfg_consistency_given_workspace_bytes(K, NR, T, 0) // 8, 1), dtype=torch.float64, device=dev)
        steps = None if a.get('no_steps') else bufs['steps'].data_ptr()
        rc = h.mfg_consistency_given(ptr('P', P), a['K'], a['N'] * a['R'], a['H'] - 1, a['d'], ptr('metrics', bufs['metrics']), steps,
                                     bufs['V'].data_ptr(), ptr('ws', ws), ws.numel() * 8 - a['short'], None)
    else:
        bufs['actions'] = nan((K, NR, T, d, d), torch.float32)
        bufs['traj'] = nan((K, NR, H, d), torch.float32)
        th, sh, al, sd = _dev_args(dev, *_policies(K, 7))
        start32 = torch.as_tensor(_starts(d, N, 5).astype(np.float32), device=dev)
        ws = torch.empty(ops.consistency_pop_workspace_bytes(N, H, d, K, R, True, True, True) // 8, dtype=torch.float64, device=dev)
        rc = h.mfg_consistency_pop(ptr('start', start32), a['N'], a['H'], a['d'], a['K'], ptr('theta', th), ptr('shift', sh),
                                   ptr('alpha', al), ptr('seed', sd), a['first_step'], a['R'], a['precision'],
                                   ptr('metrics', bufs['metrics']), bufs['steps'].data_ptr(), bufs['V'].data_ptr(),
                                   bufs['actions'].data_ptr(), bufs['traj'].data_ptr(), ptr('ws', ws),
                                   ws.numel() * 8 - a['short'], None)
    torch.cuda.synchronize()
    return rc, bufs


REFUSALS = [(dict(K=0), EINVAL), (dict(K=65536), EINVAL), (dict(H=1), EINVAL), (dict(N=0), EINVAL), (dict(R=0), EINVAL),
            (dict(d=65), EUNSUPPORTED), (dict(null='metrics'), EINVAL), (dict(null='ws'), EINVAL), (dict(short=8), EWORKSPACE)]


@pytest.mark.parametrize('entry,kw,code', [('pop', kw, code) for kw, code in REFUSALS]
                         + [('pop', dict(null=n), EINVAL) for n in ('start', 'theta', 'shift', 'alpha', 'seed')]
                         + [('pop', dict(first_step=0xFFFFFFFF - 2), EINVAL), ('pop', dict(precision=7), EINVAL)]
                         + [('given', dict(kw, no_steps=True), code) for kw, code in REFUSALS]
                         + [('given', dict(null='P'), EINVAL)])
def test_refusals_launch_nothing(dev, entry, kw, code):
    from discrete_mean_field_game_amd import _lib
    rc, bufs = _raw(dev, entry, **kw)
    assert rc == code
    assert _lib.lib().mfg_last_error()
    for name, t in bufs.items():
        assert bool(torch.isnan(t).all()), name
    rc, bufs = _raw(dev, entry)                      # the same buffers' shapes, good arguments: everything is written
    assert rc == 0
    for name, t in bufs.items():
        assert not bool(torch.isnan(t).any()), name


# ------------------------------------------------------------------------------------------------------------ 5. classes
def _population(dev, K=3, d=21, B=16, rows=6):
    from discrete_mean_field_game_amd.population import ActorCriticPopulation
    th, sh, al, sd = _policies(K, 6)
    rs = np.random.RandomState(7)
    pop = ActorCriticPopulation(th, sh, al, d, batch=B, seeds=sd, w0=rs.rand(K, d * (d + 1) // 2 + d + 1) * 0.1,
                                pi0=_starts(d, rows, 11), update_every='step', reward='synthetic')
    pop.train(1, constant=1)
    return pop


@pytest.mark.parametrize('method,cols', [('evaluate_synthetic_JSD', ('jsd_mean', 'jsd_std')),
                                         ('evaluate_synthetic', ('l1_mean', 'l1_std'))])
def test_population_evaluate_synthetic(dev, method, cols):
    from discrete_mean_field_game_amd import population
    from discrete_mean_field_game_amd.mfg_synthetic import actor_critic as SAC
    pop = _population(dev)
    K, d = pop.K, pop.d
    step0 = pop._rng_step
    assert step0 > 0
    mean, std = getattr(pop, method)(1, 4)
    assert pop._rng_step == step0 + 15
    assert mean.shape == std.shape == (K,) and np.all(np.isfinite(mean)) and np.all(std >= 0)
    want = population.consistency(pop.thetas, pop.shifts, pop.alpha_scales, pop.mat_pi0[0:4], d=d, seed=pop.seeds,
                                  precision=pop.precision, first_step=step0)
    assert np.array_equal(_bits(mean), _bits(getattr(want, cols[0]))) and np.array_equal(_bits(std), _bits(getattr(want, cols[1])))
    # each learner's own call from the same Philox step: the same actions, another summation order
    for k in range(K):
        state = np.random.get_state()
        ac = SAC(float(pop.thetas[k]), float(pop.shifts[k]), float(pop.alpha_scales[k]), d, pi0=pop.mat_pi0, batch=pop.batch,
                 seed=int(pop.seeds[k]), precision=pop.precision, device=pop.device, verbose=0)
        np.random.set_state(state)
        ac._rng_step = step0
        m, s = getattr(ac, method)(1, 4)
        assert ac._rng_step == step0 + 15
        print('learner %d: class %.17g %.17g, population %.17g %.17g' % (k, m, s, mean[k], std[k]))
        assert np.allclose([mean[k], std[k]], [m, s], rtol=1e-9, atol=0.0), k
    # repeats = 2 rolls twice the members; a failed learner is not launched: NaN, the others unchanged
    pop._rng_step = step0
    m2, s2 = getattr(pop, method)(1, 4, repeats=2)
    assert np.all(np.isfinite(m2)) and not np.array_equal(m2, mean)
    pop._rng_step = step0
    pop._act.state[1] = population.FAILED
    m3, s3 = getattr(pop, method)(1, 4)
    assert pop._rng_step == step0 + 15
    assert np.isnan(m3[1]) and np.isnan(s3[1])
    for k in (0, 2):
        assert m3[k] == mean[k] and s3[k] == std[k]
    pop.clear_status(1)
    # a range outside the table: refused, the Philox step stays
    step = pop._rng_step
    with pytest.raises(ValueError):
        getattr(pop, method)(1, 26)
    assert pop._rng_step == step


def test_population_of_another_reward_is_refused(dev):
    from discrete_mean_field_game_amd.population import ActorCriticPopulation
    pop = ActorCriticPopulation([8.0, 9.0], 0.16, 12000, 21, batch=16, pi0=_starts(21, 6, 2))
    for method in (pop.evaluate_synthetic, pop.evaluate_synthetic_JSD):
        with pytest.raises(ValueError):
            method(1, 4)
    assert pop._rng_step == 0


@pytest.mark.parametrize('metric', ['jsd', 'l1'])
def test_sweep(dev, tmp_path, metric):
    from discrete_mean_field_game_amd import mfg_synthetic as S
    from discrete_mean_field_game_amd import population
    shifts, thetas = np.arange(0, 0.04, 0.02), np.array([0.0, 1.5, 3.0])
    pi0 = _starts(21, 4, 21)
    out = str(tmp_path / 'synthetic.csv')
    kw = dict(batch=16, num_episodes=3, d=21, pi0=pi0, day_first=1, day_last=4, seed=5, eval_seed=77)
    np.random.seed(3)                                                      # (the critic weights come from np.random, as actor_critic's)
    table = S.sweep(shifts, thetas, outfile=out, metric=metric, **kw)
    assert table.shape == (6, 5)
    assert np.array_equal(table[:, 0], np.repeat(shifts, 3)) and np.array_equal(table[:, 1], np.tile(thetas, 2))   # shift-major
    lines = open(out).read().split('\n')
    assert lines[0] == 'Shift,theta_initial,theta_final,diff_mean,diff_std' and lines[7] == '' and len(lines) == 8
    assert lines[1:7] == ['%.3f,%.3f,%.3f,%.3f,%.3f' % tuple(row) for row in table]
    # theta_final: the population's, trained the same way from the same critic weights
    np.random.seed(3)
    pop = population.ActorCriticPopulation(table[:, 1], table[:, 0], 10000, 21, batch=16, seeds=5 + np.arange(6), pi0=pi0,
                                           update_every='step', reward='synthetic')
    pop.train(3, gamma=1, constant=1, lr_critic=0.1, lr_actor=0.001, isolate=True)
    assert np.all(pop.learner_state != population.FAILED)
    assert np.array_equal(_bits(pop.thetas), _bits(table[:, 2]))
    assert not np.array_equal(table[:, 2], table[:, 1])                    # (it trained)
    # diff_*: one consistency call at the final thetas and eval_seed
    want = population.consistency(table[:, 2], table[:, 0], 10000, pi0, d=21, seed=77)
    mean, std = (want.jsd_mean, want.jsd_std) if metric == 'jsd' else (want.l1_mean, want.l1_std)
    assert np.array_equal(_bits(table[:, 3]), _bits(mean)) and np.array_equal(_bits(table[:, 4]), _bits(std))
