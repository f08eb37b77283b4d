"""-m gpu: the VAR population call (mfg_var_fit_pop, ops.var_fit_pop, var.fit_population) against the NumPy restatement of its
definitions (tests/var_ref.py).  u = 2^-53.

A call has ONE d, so "all the cases in one call" is one mixed call per d: every case of that d with both ridges and both
origins, in shuffled order, each case on day rows of its own.  The module fixture runs the four mixed calls once; the tests
read them.

Bounds (none of them measured on the code under test):
  1. backward error of the solve: eta = ||G B - C||_F / (||G||_F ||B||_F + ||C||_F) <= 4 m (m + n) u, G and C formed by NumPy,
     eta evaluated in longdouble.  The worst-case Cholesky-solve bound (Higham, Accuracy and Stability, Thm 10.4:
     gamma_(3m+1) m) plus the gamma_n of the two Gram accumulations.  A wrong pivot, tile or index gives eta >~ 1e-3.
  2. forward error at lambda = 1e-2: <= 2 kappa_2(G) 4 m (m + n) u.
  3. downstream, on the device's own coefficients (conditioning cannot leak in): a fitted element within
     delta = 4 m u |z|'|B|, sse / insample within what delta does to them plus their gamma_n; `future` within 64 x the
     restatement's own fp64-against-longdouble gap on the case plus delta; per_day / metrics recomputed from the device's
     future to 1e-12.
"""
import numpy as np
import pytest

torch = pytest.importorskip('torch')

import var_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
U = R.U


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.fail('-m gpu tests need a GPU: the HIP path has no CPU fallback')
    return torch.device('cuda:0')


def run(dev, days, specs, **kw):
    """specs: (lag, ridge, train list, test list, origin) per model -> ops.var_fit_pop's outputs as NumPy."""
    from discrete_mean_field_game_amd import ops
    K = len(specs)
    ntr, nte = [len(s[2]) for s in specs], [len(s[3]) for s in specs]
    tr, te = np.zeros((K, max(ntr)), np.int32), np.zeros((K, max(max(nte), 1)), np.int32)
    for k, s in enumerate(specs):
        tr[k, :ntr[k]], te[k, :nte[k]] = s[2], s[3]
    res = ops.var_fit_pop(torch.as_tensor(np.ascontiguousarray(days), device=dev), [s[0] for s in specs], [s[1] for s in specs],
                          torch.as_tensor(tr, device=dev), ntr, torch.as_tensor(te, device=dev) if max(nte) else None, nte,
                          [s[4] for s in specs], **kw)
    torch.cuda.synchronize()
    return {n: (None if t is None else t.cpu().numpy()) for n, t in res.items()}


class Mixed:
    """One mixed call: days, specs, the case of each model, the outputs."""


@pytest.fixture(scope='module')
def mixed(dev):
    out = {}
    for d in sorted({c[0] for c in R.CASES}):
        g = Mixed()
        tables, g.specs, g.cases, at = [], [], [], 0
        for c in [c for c in R.CASES if c[0] == d]:
            days, tr, te = R.case_days(c)
            tables.append(days)
            for lam in R.RIDGES:
                for origin in (0, 1):
                    g.specs.append((c[1], lam, [at + i for i in tr], [at + i for i in te], origin))
                    g.cases.append(c)
            at += days.shape[0]
        order = np.random.RandomState(d).permutation(len(g.specs))
        g.specs, g.cases = [g.specs[i] for i in order], [g.cases[i] for i in order]
        g.days = np.concatenate(tables)
        g.out = run(dev, g.days, g.specs)
        out[d] = g
    return out


def models_of(mixed, case, lam=None, origin=None):
    g = mixed[case[0]]
    return [(g, k) for k, (s, c) in enumerate(zip(g.specs, g.cases))
            if c == case and (lam is None or s[1] == lam) and (origin is None or s[4] == origin)]


def test_every_model_of_the_mixed_calls_is_healthy(mixed):
    for g in mixed.values():
        assert not g.out['status'].any()
        assert all(np.isfinite(g.out[n]).all() for n in ('coef', 'sse', 'insample', 'future', 'per_day', 'metrics'))


def backward_error(days, train, p, lam, B, n):
    """(eta, bound): the normwise backward error of the coefficients B [m, d] of a model of lag p, ridge lam fitted on n rows of
    the training days `train`, in longdouble, and its bound 4 m (m + n) u."""
    m = B.shape[0]
    G, C = R.gram(R.series(days, train), p, lam)
    B, G, C = B.astype(np.longdouble), G.astype(np.longdouble), C.astype(np.longdouble)
    fro = lambda a: np.sqrt(np.sum(a * a))
    return float(fro(G @ B - C) / (fro(G) * fro(B) + fro(C))), 4 * m * (m + n) * U


@pytest.mark.parametrize('lam', R.RIDGES)
@pytest.mark.parametrize('case', R.CASES, ids=R.case_id)
def test_solve_backward_error(mixed, case, lam):
    d, p, n_train = case
    m, n = 1 + p * d, n_train * R.HD - p
    g, k = models_of(mixed, case, lam, 0)[0]
    eta, bound = backward_error(g.days, g.specs[k][2], p, lam, g.out['coef'][k, :m], n)
    print('eta %s lambda=%g: %.3e (bound %.3e)' % (R.case_id(case), lam, eta, bound))
    assert eta <= bound


@pytest.mark.parametrize('case', R.CASES, ids=R.case_id)
def test_solve_forward_error_at_the_larger_ridge(mixed, case):
    d, p, n_train = case
    m, n = 1 + p * d, n_train * R.HD - p
    g, k = models_of(mixed, case, 1e-2, 0)[0]
    Y = R.series(g.days, g.specs[k][2])
    G, _ = R.gram(Y, p, 1e-2)
    ref = R.ridge_fit(Y, p, 1e-2)
    err = np.linalg.norm(g.out['coef'][k, :m] - ref) / np.linalg.norm(ref)
    bound = 2 * np.linalg.cond(G, 2) * 4 * m * (m + n) * U
    print('forward %s: %.3e (bound %.3e)' % (R.case_id(case), err, bound))
    assert err <= bound


@pytest.mark.parametrize('case', R.CASES, ids=R.case_id)
def test_downstream_of_the_device_coefficients(mixed, case):
    d, p, n_train = case
    m, n = 1 + p * d, n_train * R.HD - p
    for g, k in models_of(mixed, case):
        lag, lam, tr, te, origin = g.specs[k]
        B = g.out['coef'][k, :m]
        ref = R.model(g.days, tr, te, p, lam, origin, B=B)
        Y, X = R.series(g.days, tr), R.series(g.days, te)
        # the fitted rows: element (t, j) within delta
        Z, T_ = R.design(Y, p)
        delta = 4 * m * U * (np.abs(Z) @ np.abs(B))
        E = np.abs(T_ - Z @ B)
        sse_tol = np.sum(2 * E * delta + delta ** 2, axis=0) + 4 * n * U * ref['sse']
        assert np.all(np.abs(g.out['sse'][k] - ref['sse']) <= sse_tol), (lam, origin)
        l1_tol = delta.sum(axis=1).mean() + 4 * (n + d) * U * ref['insample'][0]
        assert abs(g.out['insample'][k, 0] - ref['insample'][0]) <= l1_tol
        # JSD: |d JSD / d q_j| = |log(q_j' / m_j')| / (2 sum q) < 1 for rows within a factor e^2 of each other, as fitted rows are
        jsd_tol = delta.sum(axis=1).mean() + 4 * (n + d) * U * ref['insample'][1] + 16 * d * U
        assert abs(g.out['insample'][k, 1] - ref['insample'][1]) <= jsd_tol
        # the forecast: 64 x the restatement's own rounding over the path, plus delta of each step's regressors
        S = len(te) * R.HD
        fut = g.out['future'][k, :S]
        floor = np.zeros((S, d))
        true, own = np.concatenate([Y, X]), np.concatenate([Y, ref['future']])
        for s in range(S):
            s0 = s - s % R.HD                        # (origin 1: rows up to the day's hour 0 are observed, later ones forecast)
            if origin == 1 and s == s0:
                continue                             # the observed row itself: exact
            rows = [(own if origin == 0 or s - l > s0 else true)[len(Y) + s - l] for l in range(1, p + 1)]
            floor[s] = 4 * m * U * (np.abs(np.concatenate([[1.0]] + rows)) @ np.abs(B))
        gap = R.longdouble_gap(case, lam, origin)
        err = np.abs(fut - ref['future'])
        print('future %s lambda=%g origin=%d: max err %.3e, 64 gap %.3e, max floor %.3e' % (R.case_id(case), lam, origin, err.max(),
                                                                                          64 * gap, floor.max()))
        assert np.all(err <= 64 * gap + floor), (lam, origin)
        # the per-day values and their summary, from the device's own forecast
        per_day, met = R.metrics(fut, X, R.HD)
        assert np.max(np.abs(g.out['per_day'][k, :len(te)] - per_day)) <= 1e-12
        assert np.max(np.abs(g.out['metrics'][k] - met)) <= 1e-12


def test_padding_rows_are_zero_and_the_rolling_origin_starts_from_the_observed_row(mixed, dev):
    for g in mixed.values():
        M = g.out['coef'].shape[1]
        for k, s in enumerate(g.specs):
            m = 1 + s[0] * g.days.shape[2]
            assert m == M or not g.out['coef'][k, m:].any()
            if s[4] == 1:
                X = R.series(g.days, s[3])
                assert np.array_equal(g.out['future'][k, ::R.HD].view(np.int64), X[::R.HD].view(np.int64))
    # a model with one test day beside one with three: its forecast rows >= 16 and per-day rows >= 1 are zero
    days, tr, te = R.case_days((15, 2, 8))
    out = run(dev, days, [(2, 1e-2, tr, te, 0), (2, 1e-2, tr, te[:1], 1), (1, 1e-2, tr[:3], [], 0)])
    assert out['future'].shape == (3, 48, 15) and not out['future'][1, 16:].any() and out['future'][1, :16].all()
    assert not out['per_day'][1, 1:].any() and out['per_day'][0].all()
    assert not out['future'][2].any() and np.isnan(out['metrics'][2]).all() and np.isfinite(out['insample'][2]).all()
    assert not out['coef'][2, 16:].any() and not out['status'].any()


def test_an_all_zero_topic_stays_exactly_zero(dev):
    days, tr, te = R.case_days((15, 2, 8))
    days = days.copy()
    days[:, :, 4] = 0.0
    out = run(dev, days, [(2, 1e-8, tr, te, 0), (2, 1e-2, tr, te, 1)])
    assert not out['status'].any()
    for k in range(2):
        coef = out['coef'][k]
        assert np.all(coef[[1 + 4, 1 + 15 + 4]] == 0.0) and np.all(coef[:, 4] == 0.0) and np.all(out['future'][k][:, 4] == 0.0)


def bits(a):
    return a.view(np.int64) if a.dtype == np.float64 else a


def test_a_model_does_not_depend_on_its_neighbours(mixed, dev):
    for g in mixed.values():
        K = len(g.specs)
        S = 3 * R.HD
        back = run(dev, g.days, g.specs[::-1])
        for k, s in enumerate(g.specs):
            alone = run(dev, g.days, [s])
            m = 1 + s[0] * g.days.shape[2]
            for name in ('coef', 'sse', 'insample', 'future', 'per_day', 'metrics', 'status'):
                crop = (lambda a: a[:m]) if name == 'coef' else (lambda a: a)
                want = bits(crop(g.out[name][k]))
                assert np.array_equal(bits(crop(alone[name][0])), want), (name, k, 'alone')
                assert np.array_equal(bits(crop(back[name][K - 1 - k])), want), (name, k, 'reversed')
            assert alone['future'].shape[1] == S


def test_failures_stay_with_their_model(dev):
    base = R.synthetic_days(11, R.HD, 15, 77)
    specs = [(2, 1e-2, [0, 1, 2, 3], [8, 9], 0), (3, 1e-2, [4, 5, 6, 7], [8, 9], 1), (2, 1e-8, [0, 1, 2, 3], [9, 8], 1)]
    clean = run(dev, base, specs)
    assert not clean['status'].any()
    floats = ('coef', 'sse', 'insample', 'future', 'per_day', 'metrics')
    # a NaN in a training day of model 1 alone
    days = base.copy()
    days[5, 7, 3] = np.nan
    out = run(dev, days, specs)
    assert out['status'].tolist() == [0, 1, 0]
    for name in floats:
        assert np.isnan(out[name][1]).all(), name
        assert np.array_equal(bits(out[name][[0, 2]]), bits(clean[name][[0, 2]])), name
    # a NaN in a day that no model reads
    days = base.copy()
    days[10, 0, 0] = np.nan
    out = run(dev, days, specs)
    assert all(np.array_equal(bits(out[n]), bits(clean[n])) for n in floats + ('status',))
    # an infinity in a test day: the model reads it
    days = base.copy()
    days[9, 15, 14] = np.inf
    assert run(dev, days, specs[:1])['status'].tolist() == [1]
    # finite rows whose squares overflow: a pivot is not finite
    days = base.copy()
    days[4:8] *= 1e160
    out = run(dev, days, specs)
    assert out['status'].tolist() == [0, 2, 0]
    assert all(np.isnan(out[n][1]).all() for n in floats)
    assert all(np.array_equal(bits(out[n][[0, 2]]), bits(clean[n][[0, 2]])) for n in floats)


def test_a_refused_call_launches_nothing(dev):
    from discrete_mean_field_game_amd import ops
    days = torch.as_tensor(R.synthetic_days(4, R.HD, 15, 3), device=dev)
    tr = torch.tensor([[0, 1, 2]], dtype=torch.int32, device=dev)
    te = torch.tensor([[3]], dtype=torch.int32, device=dev)
    shapes = ops.var_fit_shapes(1, 15, 31, 16, 1)
    out = {n: torch.full(s, 7, dtype=t, device=dev) for n, (s, t) in shapes.items()}
    for bad in (dict(lags=[0]), dict(lags=[35]), dict(lags=[48]), dict(ridges=[0.0]), dict(ridges=[float('inf')]),
                dict(ridges=[float('nan')]), dict(origins=[2]), dict(train_n=[0]), dict(train_n=[4]), dict(test_n=[2])):
        a = dict(lags=[2], ridges=[1e-2], train_n=[3], test_n=[1], origins=[0])
        a.update(bad)
        with pytest.raises(ValueError):
            ops.var_fit_pop(days, a['lags'], a['ridges'], tr, a['train_n'], te, a['test_n'], a['origins'], out=out)
    with pytest.raises(ValueError):
        ops.var_fit_pop(days.float(), [2], [1e-2], tr, [3], te, [1], [0], out=out)
    with pytest.raises(ValueError):
        ops.var_fit_pop(days, [49], [1e-2], tr, [3], te, [1], [1], out=out)           # rolling origin: lag > T + 1
    torch.cuda.synchronize()
    assert all(bool((t == 7).all()) for t in out.values())


def test_chunking_changes_no_bit(mixed):
    from discrete_mean_field_game_amd import var as V
    g = mixed[15]
    names = {0: 'train_end', 1: 'rolling'}
    args = (g.days, [s[0] for s in g.specs], [s[1] for s in g.specs], [s[2] for s in g.specs], [s[3] for s in g.specs],
            [names[s[4]] for s in g.specs])
    whole = V.fit_population(*args)
    K, M = len(g.specs), g.out['coef'].shape[1]
    per = V.model_bytes(M, 48, 3, 15)
    parts = V.fit_population(*args, budget=per * ((K + 2) // 3))
    from discrete_mean_field_game_amd.population import consistency_chunks
    assert len(consistency_chunks(K, per, per * ((K + 2) // 3))) == 3
    for name in ('coef', 'sse', 'insample', 'future', 'per_day', 'metrics', 'status'):
        assert np.array_equal(bits(getattr(whole, name)), bits(g.out[name])), name
        assert np.array_equal(bits(getattr(parts, name)), bits(g.out[name])), name
    m = whole.model(0)
    p = g.specs[0][0]
    assert m['lag'] == p and m['A'].shape == (p, 15, 15) and np.array_equal(m['A'][0][2], whole.coef[0, 1:16, 2])


def test_the_forecast_scorer_takes_the_rolling_forecast(mixed, dev):
    """ops.forecast_score on VarFits.traj with one member per day: CRPS = |forecast - observation| in every cell."""
    from discrete_mean_field_game_amd import ops, var as V
    g = mixed[15]
    k = next(k for k, s in enumerate(g.specs) if s[4] == 1)
    s = g.specs[k]
    fits = V.fit_population(g.days, [s[0]], s[1], s[2], s[3], 'rolling')
    with pytest.raises(ValueError):
        V.fit_population(g.days, [s[0]], s[1], s[2], s[3]).traj(0)
    traj = torch.as_tensor(fits.traj(0)[None], device=dev)
    assert traj.shape == (1, 3, 16, 15) and traj.dtype == torch.float32
    emp32 = torch.as_tensor(R.series(g.days, s[3]).reshape(3, 16, 15).astype(np.float32), device=dev)
    sc = ops.forecast_score(traj, emp32, emp32.double(), 3, 1)
    want = (traj[0].double() - emp32.double()).abs()
    assert torch.equal(sc['crps'][0], want) and bool((sc['crps'][0][:, 0] == 0).all()) and bool((want[:, 1:] > 0).any())
