"""GPU checks of the finite-population members (mfg_agents_step_pop, mfg_forecast_agents_pop and what is built on them).  The
step's whole state is integer, so the kernel is compared with the NumPy restatement (tests/agents_ref.py) by array_equal; the
forecast is taken apart step by step: its actions are the sampler's on its own histogram rows, its counts the restatement's step
from them, its reductions the mean-field forecast's on its rows."""
import ctypes as C

import numpy as np
import pytest
import torch

import agents_ref as ref
from guard_bands import Guarded, check_all

pytestmark = pytest.mark.gpu

F32, F64, I32, I64, U8 = torch.float32, torch.float64, torch.int32, torch.int64, torch.uint8


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.fail('-m gpu tests need a GPU')
    from discrete_mean_field_game_amd import ops
    ops.init()
    return torch.device('cuda', 0)


def _members(rs, K, B, d, agents, zeros=True):
    """counts [K, B, d] int32 and actions [K, B, d, d] fp32: member 0 of a group has all its agents in one topic (topic 0, the
    last topic in the next group), member 1 keeps every other topic empty, odd members have exact zeros in their rows."""
    counts = np.zeros((K, B, d), dtype=np.int32)
    P = rs.dirichlet(np.ones(d), size=(K, B, d))
    for k in range(K):
        for b in range(B):
            w = rs.dirichlet(np.ones(d) * 0.3)
            if b == 1:
                w[1::2] = 0.0
                w[0] += 1e-3
            counts[k, b] = rs.multinomial(agents, w / w.sum())
            if b == 0:
                counts[k, b] = 0
                counts[k, b, 0 if k % 2 == 0 else d - 1] = agents
            if zeros and b % 2 == 1:
                P[k, b][rs.rand(d, d) < 0.3] = 0.0
                P[k, b][np.arange(d), rs.randint(d, size=d)] += 0.05
                P[k, b] /= P[k, b].sum(axis=1, keepdims=True)
    return counts, P.astype(np.float32)


def _step(dev, counts, P, agents, seeds, step, traj_offset=0, **kw):
    from discrete_mean_field_game_amd import ops
    out = ops.agents_step_pop(torch.as_tensor(counts, device=dev), torch.as_tensor(P, device=dev), agents,
                              torch.as_tensor(np.asarray(seeds, dtype=np.uint64).view(np.int64), device=dev), step, traj_offset,
                              want_moves=True, **kw)
    return [None if t is None else t.cpu().numpy() for t in out]


def _same_as_ref(got, counts, P, agents, seeds, step, traj_offset=0):
    want = ref.step_pop(counts, P, agents, seeds, step, traj_offset)
    assert np.array_equal(got[0], want[0]), 'counts_next'
    assert np.array_equal(got[2], want[1]), 'moves'
    assert np.array_equal(got[1].view(np.int32), want[2].view(np.int32)), 'pi_next'
    ok = want[0][..., 0] >= 0
    assert np.array_equal(got[0][ok].sum(axis=-1), counts[ok].sum(axis=-1))      # every agent lands somewhere


D_ALL, A_ALL, B_ALL = (1, 2, 15, 21, 64), (1, 3, 4, 5, 255, 256, 257, 1000, 65537), (1, 5, 67)
# PAIRWISE, not the 135-case product: every (d, A), every (d, B) and every (A, B) pair occurs in these 45 cases, B going round
# over the A values
STEP_CASES = [(d, A, B_ALL[(i + j) % 3]) for i, d in enumerate(D_ALL) for j, A in enumerate(A_ALL)]


def test_step_cases_are_pairwise_complete():
    assert {(d, B) for d, _, B in STEP_CASES} == {(d, B) for d in D_ALL for B in B_ALL}
    assert {(A, B) for _, A, B in STEP_CASES} == {(A, B) for A in A_ALL for B in B_ALL}
    assert {(d, A) for d, A, _ in STEP_CASES} == {(d, A) for d in D_ALL for A in A_ALL}


@pytest.mark.parametrize('d,agents,B', STEP_CASES)
def test_step_equals_the_restatement(dev, d, agents, B):
    from discrete_mean_field_game_amd import _lib
    rs = np.random.RandomState(1000 * d + agents % 997 + B)
    K = 2
    counts, P = _members(rs, K, B, d, agents)
    seeds = [(7 << 32) | 12345, 99]
    got = _step(dev, counts, P, agents, seeds, 41)
    _same_as_ref(got, counts, P, agents, seeds, 41)
    # in place (counts_next = counts, as the header allows), without the optional outputs: the same counts
    c, Pd = torch.as_tensor(counts, device=dev), torch.as_tensor(P, device=dev)
    sd = torch.as_tensor(np.asarray(seeds, dtype=np.uint64).view(np.int64), device=dev)
    _lib.check(_lib.lib().mfg_agents_step_pop(c.data_ptr(), Pd.data_ptr(), B, d, K, agents, sd.data_ptr(), 41, 0, c.data_ptr(), None,
                                              None, torch.cuda.current_stream().cuda_stream), 'mfg_agents_step_pop')
    assert np.array_equal(c.cpu().numpy(), got[0])


def test_step_member_ids_above_2_32_and_full_seed(dev):
    d, agents, B = 21, 1000, 5
    counts, P = _members(np.random.RandomState(3), 1, B, d, agents)
    seeds = [0xFEDCBA9876543210]
    off = (3 << 32) + 0xFFFFFFFE                                     # the ids cross a multiple of 2^32 inside the launch
    got = _step(dev, counts, P, agents, seeds, 0xFFFFFFFF, off)
    _same_as_ref(got, counts, P, agents, seeds, 0xFFFFFFFF, off)
    low = _step(dev, counts, P, agents, seeds, 0xFFFFFFFF, off & 0xFFFFFFFF)
    assert not np.array_equal(low[0], got[0])                        # the high id bits are keyed


def test_step_groups_are_independent(dev):
    d, agents, B, K = 15, 257, 5, 3
    counts, P = _members(np.random.RandomState(4), K, B, d, agents)
    seeds = [5, 5, 1 << 40]
    whole = _step(dev, counts, P, agents, seeds, 9, 2)
    for k in range(K):
        one = _step(dev, counts[k:k + 1], P[k:k + 1], agents, seeds[k:k + 1], 9, 2)
        for a, b in zip(whole, one):
            assert np.array_equal(a[k:k + 1].view(np.int32), b.view(np.int32)), k
    again = _step(dev, counts, P, agents, seeds, 9, 2)
    assert all(np.array_equal(a.view(np.int32), b.view(np.int32)) for a, b in zip(whole, again))
    bare = _step(dev, counts, P, agents, seeds, 9, 2, want_pi=False)
    assert bare[1] is None and np.array_equal(bare[0], whole[0])


def test_step_thresholds_that_do_not_ascend(dev):
    """Negative entries (no policy draws them; the given-P entry takes what it is given) make a row's thresholds go down and up:
    an agent still moves to the FIRST column with w < t, and thresholds clamp to [0, 2^32]."""
    d, agents, B = 15, 257, 5
    counts, P = _members(np.random.RandomState(6), 2, B, d, agents, zeros=False)
    P[:, :, :, 3] = -0.5 * P[:, :, :, 2]                             # t_3 < t_2
    P[:, 2, :, 0] = -1e-3                                            # t_0 < 0
    P[:, 3, :, 5] += 2.0
    P[:, 3, :, 9] = -1.5                                             # t_5 .. t_8 > 2^32
    t = np.array([ref.thresholds(P[0, b])[0] for b in range(B)])
    assert (np.diff(t, axis=-1) < 0).any() and (t == 0).any() and (t[:, :, :-1] == 1 << 32).any()
    seeds = [21, 22]
    _same_as_ref(_step(dev, counts, P, agents, seeds, 2), counts, P, agents, seeds, 2)


def test_step_a_bad_row_fails_its_member_alone(dev):
    d, agents, B, K = 21, 1000, 5, 2
    counts, P = _members(np.random.RandomState(5), K, B, d, agents, zeros=False)
    seeds = [11, 12]
    clean = _step(dev, counts, P, agents, seeds, 1)
    Q = P.copy()
    Q[0, 2, np.flatnonzero(counts[0, 2])[0], 3] = np.nan             # a row with agents
    Q[1, 3, np.flatnonzero(counts[1, 3])[-1], :] = 0.0               # a row that sums to 0
    Q[1, 1, np.flatnonzero(counts[1, 1] == 0)[0], 0] = np.inf        # an empty topic's row: harmless
    c2 = counts.copy()
    c2[0, 4, np.argmax(counts[0, 4])] -= 1                           # (a sum below `agents` is not checked)
    c2[1, 4, 5] = -1                                                 # a negative count
    got = _step(dev, c2, Q, agents, seeds, 1)
    _same_as_ref(got, c2, Q, agents, seeds, 1)
    failed = np.zeros((K, B), dtype=bool)
    failed[0, 2] = failed[1, 3] = failed[1, 4] = True
    assert np.all(got[0][failed] == -1) and np.all(got[2][failed] == -1) and np.isnan(got[1][failed]).all()
    untouched = ~failed
    untouched[0, 4] = False
    for a, b in zip(got, clean):
        assert np.array_equal(a[untouched].view(np.int32), b[untouched].view(np.int32))


# ------------------------------------------------------------------------------------------------------------ the forecast
H, FIRST = 3, 37


def _policies(K, seed):
    rs = np.random.RandomState(seed)
    seeds = rs.randint(0, 2 ** 40, K).astype(np.int64)
    return rs.uniform(6.0, 10.0, K), rs.uniform(0.1, 0.5, K), rs.uniform(8000.0, 14000.0, K), seeds


def _dev_args(dev, th, sh, al, sd):
    f = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=dev)
    return f(th), f(sh), f(al), torch.as_tensor(np.ascontiguousarray(sd, dtype=np.int64), device=dev)


def _np_curves(emp, traj):
    """The per-step L1 and JSD terms of mfg_ac2.py:631-666 on given members [N R, H, d], mean and std over the members: [H, 4]
    (as tests/test_gpu_forecast_pop.py forms them)."""
    from oracle import mfg_oracle as O
    e32 = emp.astype(np.float32).astype(np.float64)
    N, Hh = emp.shape[0], emp.shape[1]
    l1, jsd = np.zeros((traj.shape[0], Hh)), np.zeros((traj.shape[0], Hh))
    for j in range(traj.shape[0]):
        mt = traj[j].astype(np.float64)
        for l in range(Hh):
            l1[j, l] = np.linalg.norm(mt[l] - emp[j % N, l], ord=1)
            jsd[j, l] = O.JSD(e32[j % N, l].copy(), mt[l].copy())
    return np.stack([l1.mean(0), l1.std(0), jsd.mean(0), jsd.std(0)], axis=1)


def _check_taken_apart(dev, out, emp, counts0, agents, policies, ranks, R, precision, first=FIRST):
    """A finite-population forecast with its members, counts and actions (the dict of ops.forecast_agents_pop), taken apart:
    every action is sample_dirichlet's on the member's state, every step the restatement's (tests/agents_ref.py), the members
    the rounded quotients of the counts, the reductions those of the mean-field forecast on these members."""
    from discrete_mean_field_game_amd import ops
    th, sh, al, sd = policies
    K, N, d = len(th), emp.shape[0], emp.shape[2]
    traj, counts, actions = out['traj'].cpu().numpy(), out['counts'].cpu().numpy(), out['actions'].cpu().numpy()
    assert traj.shape == (K, N * R, H, d) and counts.shape == traj.shape and actions.shape == (K, N * R, H - 1, d, d)
    assert np.array_equal(counts[:, :, 0], np.broadcast_to(np.tile(counts0, (R, 1)), (K, N * R, d)))
    assert np.all(counts.sum(axis=-1) == agents) and counts.min() >= 0
    assert np.array_equal(traj, (counts.astype(np.float64) / float(agents)).astype(np.float32))       # the rounded quotient
    for k in range(K):
        theta = torch.tensor([th[k]], dtype=F64, device=dev)
        for t in range(H - 1):
            P = ops.sample_dirichlet(out['traj'][k, :, t].contiguous(), theta, float(sh[k]), float(al[k]), int(sd[k]),
                                     step=first + t, traj_offset=0, precision=precision)
            assert torch.equal(out['actions'][k, :, t], P), (k, t)
            want = ref.step_pop(counts[k:k + 1, :, t], actions[k:k + 1, :, t], agents, [int(sd[k])], first + t)[0]
            assert np.array_equal(counts[k:k + 1, :, t + 1], want), (k, t)
    # the reductions: those of the mean-field forecast, on these members (tolerances of tests/test_gpu_forecast_pop.py)
    tol = 2.0 * R * 2.0 ** -53
    mean, std, quant, curves = (out[key].cpu().numpy() for key in ('mean', 'std', 'quant', 'curves'))
    for k in range(K):
        m = traj[k].reshape(R, N, H, d).transpose(1, 0, 2, 3)        # member r of start state n is trajectory r N + n
        assert np.array_equal(quant[k], np.sort(m, axis=1)[:, list(ranks)].transpose(0, 2, 1, 3)), k
        m64 = m.astype(np.float64)
        err_mean = np.max(np.abs(mean[k] - m64.mean(axis=1)))
        err_std = np.max(np.abs(std[k] - m64.std(axis=1)) - tol * np.abs(m64.std(axis=1)))
        print('learner %d: mean error %.3e (tol %.3e), std excess %.3e (abs tol %.3e)' % (k, err_mean, tol, err_std, 2.0 ** -60))
        assert err_mean <= tol and err_std <= 2.0 ** -60, k
        assert np.array_equal(mean[k][:, 0], traj[k, :N, 0].astype(np.float64)) and not std[k][:, 0].any()
        np.testing.assert_allclose(curves[k], _np_curves(emp, traj[k]), rtol=1e-12, atol=1e-15, err_msg='learner %d' % k)


@pytest.mark.parametrize('precision', ['mixed', 'f64'])
@pytest.mark.parametrize('agents', [1, 5, 1000])
@pytest.mark.parametrize('d', [15, 21, 4])
def test_forecast_taken_apart(dev, d, agents, precision):
    from discrete_mean_field_game_amd import ops, population
    K, N, R = 2, 2, 3
    rs = np.random.RandomState(d + agents)
    emp = np.array([[[float('%.3e' % v) for v in row] for row in rs.dirichlet(np.ones(d), size=H)] for _ in range(N)])
    th, sh, al, sd = _policies(K, d + K)
    counts0 = population.apportion(emp[:, 0], agents)
    ranks = (0, R - 1, R // 2)
    out = ops.forecast_agents_pop(torch.as_tensor(counts0, device=dev), agents, *_dev_args(dev, th, sh, al, sd), H, first_step=FIRST,
                                  repeats=R, ranks=ranks, precision=precision,
                                  emp32=torch.as_tensor(emp.astype(np.float32), device=dev), emp64=torch.as_tensor(emp.copy(), device=dev),
                                  want_traj=True, want_counts=True, want_actions=True)
    _check_taken_apart(dev, out, emp, counts0, agents, (th, sh, al, sd), ranks, R, precision)
    mean, std = out['mean'].cpu().numpy(), out['std'].cpu().numpy()
    # nothing but the moments asked for: the same moments
    bare = ops.forecast_agents_pop(torch.as_tensor(counts0, device=dev), agents, *_dev_args(dev, th, sh, al, sd), H, first_step=FIRST,
                                   repeats=R, precision=precision)
    assert all(bare[key] is None for key in ('quant', 'curves', 'traj', 'counts', 'actions'))
    assert np.array_equal(bare['mean'].cpu().numpy(), mean) and np.array_equal(bare['std'].cpu().numpy(), std)


def test_forecast_mixed_range_policy_fails_alone_and_the_call_completes(dev):
    """One policy of K beyond mixed precision's fp32 range (|theta| (1 + |shift|) > 86): as mfg_forecast_pop, the call itself
    returns -- all its launches, however many steps and whenever the host sees the device's report -- the healthy policies'
    outputs are complete and equal their own call's, the bad policy's members fail (NaN rows and -1 counts after row 0),
    and the NEXT mixed-precision call on the context is refused.  H = 16: fifteen sampling launches behind the report."""
    from discrete_mean_field_game_amd import _lib, ops, population
    d, N, R, agents, Hh = 21, 2, 3, 100, 16
    start = np.random.RandomState(12).dirichlet(np.ones(d), size=N)
    counts0 = torch.as_tensor(population.apportion(start, agents), device=dev)
    th, sh, al, sd = np.array([8.0, 150.0, 9.0]), np.full(3, 0.5), np.full(3, 1e4), np.array([5, 6, 7], dtype=np.int64)
    ops.clear_status()
    ctx = ops.Context(dev)
    prev = ctx.bind_scoped()
    try:
        out = ops.forecast_agents_pop(counts0, agents, *_dev_args(dev, th, sh, al, sd), Hh, first_step=FIRST, repeats=R, ranks=(0, 2),
                                      want_traj=True, want_counts=True)                 # returns: no MfgError
        assert ctx.status(synchronize=True) & _lib.STATUS_MIXED_RANGE
        with pytest.raises(_lib.MfgError) as refused:
            ops.forecast_agents_pop(counts0, agents, *_dev_args(dev, th, sh, al, sd), Hh, repeats=R)
        assert refused.value.code != 0
        ctx.clear_status()
        host = {k: v.cpu().numpy() for k, v in out.items() if v is not None}
        for k in (0, 2):
            one = ops.forecast_agents_pop(counts0, agents, *_dev_args(dev, th[k:k + 1], sh[k:k + 1], al[k:k + 1], sd[k:k + 1]), Hh,
                                          first_step=FIRST, repeats=R, ranks=(0, 2), want_traj=True, want_counts=True)
            for key, a in host.items():
                assert np.array_equal(a[k], one[key][0].cpu().numpy()), (key, k)
            assert np.all(np.isfinite(host['mean'][k])) and np.all(host['counts'][k].sum(axis=-1) == agents)
        assert ctx.status(synchronize=True) == 0
    finally:
        ctx.restore(prev)
        ctx.close()
    # the bad policy: row 0 stands; its actions are unspecified (csrc/mfg_device.h: NaN only where a product overflowed), so
    # every later row of a member is either a failed one (-1, NaN) or still a histogram of all its agents -- nothing else
    c, x = host['counts'][1], host['traj'][1]
    assert np.array_equal(c[:, 0], host['counts'][0][:, 0]) and np.array_equal(x[:, 0], host['traj'][0][:, 0])
    failed = (c == -1).all(axis=-1)
    whole = (c >= 0).all(axis=-1) & (c.sum(axis=-1) == agents)
    assert np.all(failed | whole) and not failed[:, 0].any()
    assert np.all(failed[:, 1:] >= failed[:, :-1])                   # a failed member stays failed
    assert np.isnan(x[failed]).all() and np.array_equal(x[whole], (c[whole].astype(np.float64) / agents).astype(np.float32))
    assert ops.status(synchronize=True) == 0                         # the default context's word was never involved
    # the module function: raises on a context of its own, leaves the caller's word alone; strict precision has no such range
    with pytest.raises(_lib.MfgError):
        population.forecast_agents(th, 0.5, 1e4, start, Hh, d=d, agents=agents, repeats=R)
    assert ops.status(synchronize=True) == 0
    fc = population.forecast_agents(th, 0.5, 1e4, start, Hh, d=d, agents=agents, repeats=R, precision='f64', want_counts=True)
    assert np.all(np.isfinite(fc.mean)) and np.all(fc.counts.sum(axis=-1) == agents)


# ------------------------------------------------------------------------------------------------- module and class layers
def test_population_chunks_and_scores(dev, monkeypatch):
    from discrete_mean_field_game_amd import ops, population
    d, N, R, agents, Hh = 21, 3, 5, 300, 4
    emp = np.random.RandomState(10).dirichlet(np.ones(d), size=(N, Hh))
    th = [7.0, 8.5, 8.5, 9.5, 6.5]
    kw = dict(d=d, agents=agents, seed=12345, repeats=R)
    whole = population.forecast_agents(th, 0.3, 1e4, None, Hh, emp=emp, probs=(0.0, 0.5, 1.0), want_traj=True, want_counts=True, **kw)
    assert whole.counts.shape == (5, N * R, Hh, d) and np.all(whole.counts.sum(axis=-1) == agents)
    assert np.array_equal(whole.traj[1], whole.traj[2]) and not np.array_equal(whole.traj[0], whole.traj[1])   # common random numbers
    assert np.array_equal(whole.counts[:, :N, 0], np.broadcast_to(population.apportion(emp[:, 0], agents), (5, N, d)))
    score = population.forecast_agents_score(th, 0.3, 1e4, emp, horizon=Hh, **kw)
    e64 = torch.as_tensor(emp.copy(), device=dev)
    want = ops.forecast_score(torch.as_tensor(whole.traj, device=dev), e64.float(), e64, N, R)
    for key in ('crps', 'less', 'equal', 'energy', 'summary'):
        assert np.array_equal(getattr(score, key), want[key].cpu().numpy()), key
    per = population.forecast_agents_score_bytes(N, Hh, d, R)
    chunked = population.forecast_agents_score(th, 0.3, 1e4, emp, horizon=Hh, budget=2 * per, **kw)          # chunks of 2, 2, 1
    for key in ('crps', 'less', 'equal', 'energy', 'summary'):
        assert np.array_equal(getattr(chunked, key), getattr(score, key)), key
    monkeypatch.setattr(population, 'FORECAST_CHUNK', 2)
    parts = population.forecast_agents(th, 0.3, 1e4, None, Hh, emp=emp, probs=(0.0, 0.5, 1.0), want_traj=True, want_counts=True, **kw)
    for key in ('mean', 'std', 'quantiles', 'curves', 'traj', 'counts'):
        assert np.array_equal(getattr(parts, key), getattr(whole, key)), key


def _same(a, b, keys):
    for key in keys:
        x, y = getattr(a, key), getattr(b, key)
        assert (x is None) == (y is None), key
        if x is not None:
            assert np.array_equal(x, y), key


FC_KEYS = ('mean', 'std', 'quantiles', 'curves', 'traj', 'counts')
SC_KEYS = ('crps', 'less', 'equal', 'energy', 'summary')


def test_class_methods_equal_the_module_functions(dev):
    from discrete_mean_field_game_amd import population
    from discrete_mean_field_game_amd.population import ActorCriticPopulation
    d, K, R, agents, Hh = 21, 3, 4, 500, 4
    th, sh, al, sd = _policies(K, 6)
    rs = np.random.RandomState(7)
    emp = rs.dirichlet(np.ones(d), size=(2, Hh))
    pop = ActorCriticPopulation(th, sh, al, d, batch=64, seeds=sd, w0=rs.rand(K, d * (d + 1) // 2 + d + 1) * 0.1,
                                pi0=rs.dirichlet(np.ones(d), size=16), update_every='step')
    pop.train(1)
    learners = [pop.learner(k) for k in range(K)]
    step0 = pop._rng_step
    assert step0 > 0
    fc = pop.forecast_agents(emp[:, 0], horizon=Hh, repeats=R, agents=agents, want_traj=True, want_counts=True)
    assert pop._rng_step == step0 + Hh - 1
    args = (pop.thetas, pop.shifts, pop.alpha_scales)
    kw = dict(d=d, agents=agents, seed=pop.seeds, repeats=R, precision=pop.precision)
    _same(fc, population.forecast_agents(*args, emp[:, 0], Hh, first_step=step0, want_traj=True, want_counts=True, **kw), FC_KEYS)
    sc = pop.forecast_agents_score(horizon=Hh, repeats=R, agents=agents, emp=emp)
    assert pop._rng_step == step0 + 2 * (Hh - 1)
    _same(sc, population.forecast_agents_score(*args, emp, horizon=Hh, first_step=step0 + Hh - 1, **kw), SC_KEYS)
    for k, lk in enumerate(learners):
        own = lk.forecast_agents(emp[:, 0], Hh, R, agents=agents, want_traj=True, want_counts=True)
        assert lk._rng_step == step0 + Hh - 1 and own.mean.shape == (2, Hh, d) and own.counts.dtype == np.int32
        _same(own, fc.learner(k), FC_KEYS)
        _same(lk.forecast_agents_score(None, Hh, R, agents=agents, emp=emp), sc.learner(k), SC_KEYS)
    with pytest.raises(ValueError):
        pop.forecast_agents(emp[:, 0], horizon=Hh, repeats=R, agents=0)
    assert pop._rng_step == step0 + 2 * (Hh - 1)                     # refused ahead of the step


# ------------------------------------------------------------------------------------------------------------ guard bands
def _call(name, *args):
    from discrete_mean_field_game_amd import _lib
    _lib.check(getattr(_lib.lib(), name)(*args, torch.cuda.current_stream().cuda_stream), name)


@pytest.mark.parametrize('offset', [0, 4], ids=['aligned', 'offset4'])
@pytest.mark.parametrize('d,agents,B', [(21, 1000, 5), (64, 257, 3), (1, 4, 67)])
def test_step_writes_inside_its_outputs(dev, d, agents, B, offset):
    K = 2
    counts, P = _members(np.random.RandomState(d), K, B, d, agents)
    seeds = [3, (1 << 35) + 1]
    want = _step(dev, counts, P, agents, seeds, 5)
    g = {'counts': Guarded((K, B, d), I32, dev, offset=offset, fill=torch.as_tensor(counts)),
         'P': Guarded((K, B, d, d), F32, dev, offset=offset, fill=torch.as_tensor(P)),
         'seeds': Guarded((K,), I64, dev, fill=torch.as_tensor(np.asarray(seeds, dtype=np.int64))),
         'counts_next': Guarded((K, B, d), I32, dev, offset=offset), 'pi_next': Guarded((K, B, d), F32, dev, offset=offset),
         'moves': Guarded((K, B, d, d), I32, dev, offset=offset)}
    _call('mfg_agents_step_pop', g['counts'].ptr(), g['P'].ptr(), B, d, K, agents, g['seeds'].ptr(), 5, 0, g['counts_next'].ptr(),
          g['pi_next'].ptr(), g['moves'].ptr())
    torch.cuda.synchronize()
    check_all(*g.items())
    assert np.array_equal(g['counts_next'].t.cpu().numpy(), want[0]) and np.array_equal(g['moves'].t.cpu().numpy(), want[2])
    assert np.array_equal(g['pi_next'].t.cpu().numpy().view(np.int32), want[1].view(np.int32))
    assert np.array_equal(g['counts'].t.cpu().numpy(), counts) and np.array_equal(g['P'].t.cpu().numpy(), P)     # inputs untouched


@pytest.mark.parametrize('offset', [0, 4], ids=['aligned', 'offset4'])
@pytest.mark.parametrize('given', [True, False], ids=['all_outputs', 'in_workspace'])
def test_forecast_writes_inside_its_outputs_and_workspace(dev, given, offset):
    """Every fp32 / int32 buffer at offset 0 and 4 (the fp64 outputs and the workspace, which holds fp64 parts, stay 8-byte
    aligned, as the header asks); the workspace is exactly the advertised bytes."""
    from discrete_mean_field_game_amd import _lib, ops, population
    d, K, N, R, Hh, agents = 21, 2, 2, 3, 4, 77
    rs = np.random.RandomState(11)
    emp = rs.dirichlet(np.ones(d), size=(N, Hh))
    counts0 = population.apportion(emp[:, 0], agents)
    th, sh, al, sd = _policies(K, 12)
    ranks = (0, R - 1, R // 2)
    e32, e64 = torch.as_tensor(emp.astype(np.float32), device=dev), torch.as_tensor(emp.copy(), device=dev)
    want = ops.forecast_agents_pop(torch.as_tensor(counts0, device=dev), agents, *_dev_args(dev, th, sh, al, sd), Hh, first_step=FIRST,
                                   repeats=R, ranks=ranks, emp32=e32, emp64=e64, want_traj=True, want_counts=True, want_actions=True)
    nbytes = int(_lib.lib().mfg_forecast_agents_pop_workspace_bytes(N, Hh, d, K, R, int(given), int(given)))
    assert nbytes % 8 == 0
    NR = N * R
    g = {'counts0': Guarded((N, d), I32, dev, offset=offset, fill=torch.as_tensor(counts0)),
         'emp32': Guarded((N, Hh, d), F32, dev, offset=offset, fill=e32.cpu()), 'emp64': Guarded((N, Hh, d), F64, dev, fill=e64.cpu()),
         'mean': Guarded((K, N, Hh, d), F64, dev), 'std': Guarded((K, N, Hh, d), F64, dev),
         'quant': Guarded((K, N, Hh, len(ranks), d), F32, dev, offset=offset), 'curves': Guarded((K, Hh, 4), F64, dev),
         'ws': Guarded((nbytes,), U8, dev)}
    if given:
        g.update(traj=Guarded((K, NR, Hh, d), F32, dev, offset=offset), counts=Guarded((K, NR, Hh, d), I32, dev, offset=offset),
                 actions=Guarded((K, NR, Hh - 1, d, d), F32, dev, offset=offset))
    p = lambda name: g[name].ptr() if name in g else None
    pol = _dev_args(dev, th, sh, al, sd)
    _call('mfg_forecast_agents_pop', p('counts0'), N, Hh, d, K, agents, *[t.data_ptr() for t in pol], FIRST, R, _lib.PRECISIONS['mixed'],
          (C.c_int32 * len(ranks))(*ranks), len(ranks), p('emp32'), p('emp64'), p('mean'), p('std'), p('quant'), p('curves'),
          p('traj'), p('counts'), p('actions'), p('ws'), nbytes)
    torch.cuda.synchronize()
    check_all(*g.items())
    names = {'mean': 'mean', 'std': 'std', 'quant': 'quant', 'curves': 'curves'}
    if given:
        names.update(traj='traj', counts='counts', actions='actions')
    for name, key in names.items():
        a, b = g[name].t.cpu().numpy(), want[key].cpu().numpy()
        assert np.array_equal(a.view(np.int32 if a.itemsize == 4 else np.int64), b.view(np.int32 if b.itemsize == 4 else np.int64)), name
