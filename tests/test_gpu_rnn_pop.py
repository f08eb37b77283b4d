"""-m gpu: mfg_rnn_fit_pop against the NumPy restatement tests/rnn_ref.py (itself pinned to torch.autograd and torch.optim.Adam in
tests/test_rnn_host.py).  As in the VAR tests there is one mixed call per d, the models in shuffled order, read by all tests.

Tolerances are not fixed figures: each is 64 x the restatement's own float64-against-longdouble gap on that case (the maximum over
elements) plus a floor of 16 u x the largest magnitude in the case, u = 2^-53 (rnn_ref.bound).  The margin is the form and the
factor of bound 3 of tests/test_gpu_var_pop.py: it covers a different but equally long fp64 summation order on the device, and it
is measured on the restatement, never on the code under test.  Adam turns a gradient error delta into a weight error of up to
lr delta / eps where |g| is below eps; the longdouble gap contains that amplification.  Every test prints the measured error next
to its bound.

The status-2 half of the failure test is not here: with lr = 1e6 the restatement's loss stays finite over 8 epochs at these shapes
(Adam moves a weight by at most lr per epoch: 1.4e6 .. 4.6e7; gradient descent with wd = 1e-3 reaches 1.7e43), so there is no
overflow to compare, and a failure that only the device shows is not constructed."""
import numpy as np
import pytest

torch = pytest.importorskip('torch')

import rnn_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
EPOCHS = 8
# per case two models: plain, and weight decay with an active clip
VARIANTS = [dict(lr=1e-2, wd=0.0, clip=0.0), dict(lr=3e-3, wd=1e-3, clip=0.02)]


class _Group:
    """The cases of one d: a day table, per model (case, variant, lists, w0), a shuffled order."""

    def __init__(self, d, cases, seed):
        rs = np.random.RandomState(seed)
        self.d, self.Hd = d, cases[0][3]
        self.D = max(c[2] for c in cases) + R.N_VAL + R.N_TEST
        self.days = R.dirichlet_days(self.D, self.Hd, d, 3000 + seed)
        self.models = []
        for case in cases:
            for v, var in enumerate(VARIANTS):
                pick = rs.permutation(self.D)[:case[2] + R.N_VAL + R.N_TEST].tolist()
                n = case[2]
                self.models.append(dict(case=case, var=var, H=case[1], tr=pick[:n], va=pick[n:n + R.N_VAL], te=pick[n + R.N_VAL:],
                                        w0=R.init_weights(case[1], d, [seed, len(self.models)])))
        self.order = rs.permutation(len(self.models)).tolist()


def _call(g, ids, dev, optimizer='adam', epochs=EPOCHS, lrs=None, val=True, days=None, override=None):
    """One ops.rnn_fit_pop call over the models `ids` of group g, in that order; NumPy out.  override: {position: entries of the
    model's record to replace}."""
    from discrete_mean_field_game_amd import ops
    from discrete_mean_field_game_amd.var import _table
    ms = [dict(g.models[i]) for i in ids]
    for pos, entries in (override or {}).items():
        ms[pos].update(entries)
    W_max = max(R.weight_count(m['H'], g.d) for m in g.models)
    w0 = np.zeros((len(ms), W_max))
    for k, m in enumerate(ms):
        w0[k, :m['w0'].size] = m['w0']
    tab = lambda key: torch.as_tensor(_table([np.asarray(m[key]) for m in ms], max(len(m[key]) for m in g.models)), device=dev)
    res = ops.rnn_fit_pop(torch.as_tensor(g.days if days is None else days, device=dev), torch.as_tensor(w0, device=dev),
                          [m['H'] for m in ms], [epochs] * len(ms), [m['var']['lr'] for m in ms] if lrs is None else lrs,
                          [m['var']['wd'] for m in ms], [m['var']['clip'] for m in ms], tab('tr'), [len(m['tr']) for m in ms],
                          tab('va') if val else None, [len(m['va']) if val else 0 for m in ms], tab('te'), [len(m['te']) for m in ms],
                          optimizer=optimizer, E_max=EPOCHS, C_max=EPOCHS if val else None)
    torch.cuda.synchronize()
    return {n: t.cpu().numpy() for n, t in res.items()}


class _Module:
    pass


@pytest.fixture(scope='module')
def M():
    if not torch.cuda.is_available():
        pytest.fail('-m gpu tests need a GPU: the HIP path has no CPU fallback')
    m = _Module()
    m.dev = torch.device('cuda:0')
    by_d = {}
    for case in R.CASES:
        by_d.setdefault((case[0], case[3]), []).append(case)
    m.groups = [_Group(d, cases, 10 + i) for i, ((d, _), cases) in enumerate(sorted(by_d.items()))]
    m.adam = [_call(g, g.order, m.dev) for g in m.groups]
    m.sgd = [_call(g, g.order, m.dev, optimizer='sgd', epochs=1, lrs=[1.0] * len(g.order), val=False) for g in m.groups]
    m.ref = {}
    return m


def _models(M):
    """(group index, position in the mixed call, model index) of every model."""
    return [(gi, pos, i) for gi, g in enumerate(M.groups) for pos, i in enumerate(g.order)]


def _ref(M, gi, i, dtype):
    """The restatement's 8 Adam epochs of model i of group gi, cached: computed once, shared, left unchanged."""
    key = (gi, i, dtype)
    if key not in M.ref:
        g = M.groups[gi]
        m = g.models[i]
        M.ref[key] = R.model(g.days, m['tr'], m['va'], m['te'], m['H'], m['w0'], EPOCHS, dtype=dtype, **m['var'])
    return M.ref[key]


def _name(M, gi, i):
    m = M.groups[gi].models[i]
    return '%s%s' % (R.case_id(m['case']), '-wd-clip' if m['var']['wd'] else '')


def _report(what, name, err, bound):
    print('%-10s %-28s err %.3e  bound %.3e  ratio %.3f' % (what, name, err, bound, err / bound))
    return err / bound


def test_the_mixed_calls_cover_every_case_twice_in_shuffled_order(M):
    seen = sorted((m['case'], bool(m['var']['wd'])) for g in M.groups for m in g.models)
    assert seen == sorted((c, w) for c in R.CASES for w in (False, True))
    assert any(g.order != sorted(g.order) for g in M.groups)
    for out in M.adam + M.sgd:
        assert not out['status'].any()


def test_gradient_of_one_sgd_epoch(M):
    """optimizer = 'sgd', one epoch, lr = 1 (the division is exact): g = (w0 - w1) / lr element by element.  The floor's magnitude
    is the larger of max |g| and max |w0|: w1 is rounded at the magnitude of the weights, both on the device and in the
    restatement, whatever the gradient's size."""
    for gi, pos, i in _models(M):
        g, m = M.groups[gi], M.groups[gi].models[i]
        W = m['w0'].size
        g_dev = m['w0'] - M.sgd[gi]['weights'][pos, :W]
        Y = g.days[m['tr']]
        l64, g64 = R.loss_and_grad(m['w0'], m['H'], g.d, Y, m['var']['wd'])
        lld, gld = R.loss_and_grad(m['w0'], m['H'], g.d, Y, m['var']['wd'], np.longdouble)
        gn = float(np.sqrt((g64 * g64).sum()))
        if m['var']['clip'] > 0 and gn > m['var']['clip']:
            g64, gld = g64 * (m['var']['clip'] / gn), gld * (np.longdouble(m['var']['clip']) / np.sqrt((gld * gld).sum()))
        bound = R.bound(g64, gld, max(np.abs(g64).max(), np.abs(m['w0']).max()))
        _report('gradient', _name(M, gi, i), float(np.abs(g_dev - g64).max()), bound)
        assert np.abs(g_dev - g64).max() <= bound
        assert abs(M.sgd[gi]['loss'][pos, 0] - l64) <= R.bound(l64, lld) and np.isnan(M.sgd[gi]['loss'][pos, 1:]).all()
        assert M.sgd[gi]['best_epoch'][pos] == 1 and np.all(M.sgd[gi]['weights'][pos, W:] == 0)


def test_an_active_clip_is_in_the_cases(M):
    for gi, pos, i in _models(M):
        g, m = M.groups[gi], M.groups[gi].models[i]
        if m['var']['clip'] > 0:
            _, g64 = R.loss_and_grad(m['w0'], m['H'], g.d, g.days[m['tr']], m['var']['wd'])
            assert np.sqrt((g64 * g64).sum()) > m['var']['clip'], 'the clip of %s never acts' % _name(M, gi, i)


def test_eight_adam_epochs(M):
    """Weights (the selected iterate), loss, val and best_epoch."""
    for gi, pos, i in _models(M):
        m = M.groups[gi].models[i]
        W = m['w0'].size
        a, b, out = _ref(M, gi, i, np.float64), _ref(M, gi, i, np.longdouble), M.adam[gi]
        assert out['best_epoch'][pos] == a['best_epoch'] == b['best_epoch']
        for what, dev, r64, rld in (('weights', out['weights'][pos, :W], a['weights'], b['weights']),
                                    ('loss', out['loss'][pos], a['loss'], b['loss']), ('val', out['val'][pos], a['val'], b['val'])):
            bound = R.bound(r64, rld)
            err = float(np.abs(dev - r64).max())
            _report(what, _name(M, gi, i), err, bound)
            assert err <= bound, '%s of %s: %.3e > %.3e' % (what, _name(M, gi, i), err, bound)
        assert np.all(out['weights'][pos, W:] == 0)


def test_downstream_of_the_devices_own_weights(M):
    """future recomputed by the restatement from the RETURNED weights; per_day and metrics recomputed from the device's own
    future to 1e-12 (the VAR tests' figure)."""
    for gi, pos, i in _models(M):
        g, m, out = M.groups[gi], M.groups[gi].models[i], M.adam[gi]
        w = out['weights'][pos, :m['w0'].size]
        Y = g.days[m['te']]
        f64, fld = R.forecast(w, m['H'], g.d, Y), R.forecast(w.astype(np.longdouble), m['H'], g.d, Y)
        fut = out['future'][pos, :len(m['te'])]
        bound = R.bound(f64, fld)
        err = float(np.abs(fut - f64).max())
        _report('future', _name(M, gi, i), err, bound)
        assert err <= bound and np.array_equal(fut[:, 0], Y[:, 0])
        per_day, met = R.metrics(fut, Y)
        assert np.abs(out['per_day'][pos, :len(m['te'])] - per_day).max() <= 1e-12 and np.abs(out['metrics'][pos] - met).max() <= 1e-12


def test_a_model_is_the_same_bits_alone_elsewhere_and_in_chunks(M, monkeypatch):
    from discrete_mean_field_game_amd import ops, rnn
    for gi, g in enumerate(M.groups):
        mixed = M.adam[gi]
        rev = _call(g, g.order[::-1], M.dev)
        for pos, i in enumerate(g.order):
            alone = _call(g, [i], M.dev)
            for name in ops.RNN_OUTPUTS:
                assert np.array_equal(alone[name][0], mixed[name][pos], equal_nan=True), '%s of %s alone' % (name, _name(M, gi, i))
                assert np.array_equal(rev[name][len(g.order) - 1 - pos], mixed[name][pos], equal_nan=True), name
        # through rnn.fit_population with a budget that leaves one model to a chunk
        ms = [g.models[i] for i in g.order]
        counts = [[len(m[k]) for m in ms] for k in ('tr', 'va', 'te')]
        budget = rnn.model_bytes([m['H'] for m in ms], [EPOCHS] * len(ms), *counts, g.d, g.Hd)
        calls = []
        real = ops.rnn_fit_pop
        monkeypatch.setattr(ops, 'rnn_fit_pop', lambda *a, **kw: calls.append(len(a[2])) or real(*a, **kw))
        fits = rnn.fit_population(g.days, [m['H'] for m in ms], [m['var']['lr'] for m in ms], EPOCHS, [m['tr'] for m in ms],
                                  [m['va'] for m in ms], [m['te'] for m in ms], wd=[m['var']['wd'] for m in ms],
                                  clip=[m['var']['clip'] for m in ms], w0=[m['w0'] for m in ms], budget=budget, device=M.dev)
        monkeypatch.setattr(ops, 'rnn_fit_pop', real)
        assert calls == [1] * len(ms)
        for name in ops.RNN_OUTPUTS:
            assert np.array_equal(getattr(fits, name), mixed[name], equal_nan=True), '%s in chunks' % name


@pytest.mark.parametrize('case,lr,inside', [((3, 4, 2, 16), 0.2, 3), ((5, 8, 3, 5), 0.02, 4)], ids=['d3-H4', 'd5-H8'])
def test_selection_returns_the_best_held_out_iterate(M, case, lr, inside):
    """12 epochs whose validation curve (from the restatement) has its minimum strictly inside: that epoch and those weights come
    back.  Without validation days the last iterate comes back."""
    from discrete_mean_field_game_amd import rnn
    d, H, n, Hd = case
    days, tr, va, te = R.case_days(case)
    w0 = R.init_weights(H, d, 21)
    a = R.model(days, tr, va, te, H, w0, 12, lr)
    b = R.model(days, tr, va, te, H, w0, 12, lr, dtype=np.longdouble)
    assert a['best_epoch'] == b['best_epoch'] == inside == int(np.argmin(a['val'])) + 1 and 1 < inside < 12
    assert np.sort(a['val'])[1] - a['val'].min() > 1e-6            # (no tie that rounding could turn)
    fits = rnn.fit_population(days, [H], lr, 12, tr, va, te, w0=[w0], device=M.dev)
    assert fits.status[0] == 0 and fits.best_epoch[0] == inside
    for what, dev, r64, rld in (('weights', fits.weights[0], a['weights'], b['weights']), ('val', fits.val[0], a['val'], b['val'])):
        bound = R.bound(r64, rld)
        _report(what, 'selection ' + R.case_id(case), float(np.abs(dev - r64).max()), bound)
        assert np.abs(dev - r64).max() <= bound
    assert np.abs(fits.weights[0] - a['last']).max() > 1e-4        # (and it is not the last iterate)
    last = rnn.fit_population(days, [H], lr, 12, tr, None, te, w0=[w0], device=M.dev)
    assert last.best_epoch[0] == 12 and last.val.shape == (1, 0)
    bound = R.bound(a['last'], b['last'])
    assert np.abs(last.weights[0] - a['last']).max() <= bound
    # eval_every = 5: checks after epochs 5, 10 and the last
    every = rnn.fit_population(days, [H], lr, 12, tr, va, te, w0=[w0], eval_every=5, device=M.dev)
    want = a['val'][[4, 9, 11]]
    assert every.val.shape == (1, 3) and np.abs(every.val[0] - want).max() <= R.bound(want, b['val'][[4, 9, 11]])
    assert every.best_epoch[0] == (5, 10, 12)[int(np.argmin(want))]


def test_a_nan_day_fails_its_model_alone(M):
    from discrete_mean_field_game_amd import ops
    gi = next(i for i, g in enumerate(M.groups) if len(g.models) > 2)
    g = M.groups[gi]
    clean = M.adam[gi]
    # the victim reads a copy of one of its training days, appended to the table, with a NaN planted in it: no other model reads it
    victim = 1
    tr = list(g.models[g.order[victim]]['tr'])
    days = np.concatenate([g.days, g.days[tr[1]:tr[1] + 1]])
    days[g.D, 3, 1] = np.nan
    tr[1] = g.D
    out = _call(g, g.order, M.dev, days=days, override={victim: dict(tr=tr)})
    assert out['status'][victim] == 1 and out['best_epoch'][victim] == 0
    for name in ('weights', 'loss', 'val', 'future', 'per_day', 'metrics'):
        assert np.isnan(out[name][victim]).all(), name
    others = [p for p in range(len(g.order)) if p != victim]
    assert not out['status'][others].any()
    for name in ops.RNN_OUTPUTS:
        assert np.array_equal(out[name][others], clean[name][others], equal_nan=True), name
    # a day index outside the table is the same failure, and nothing outside the table is read
    from discrete_mean_field_game_amd.var import _table
    m = g.models[g.order[0]]
    W = m['w0'].size
    tr = torch.as_tensor(_table([np.asarray(m['tr'][:-1] + [g.D + 5])], len(m['tr'])), device=M.dev)
    res = ops.rnn_fit_pop(torch.as_tensor(g.days, device=M.dev), torch.as_tensor(m['w0'][None].copy(), device=M.dev), [m['H']], [2],
                          [1e-2], [0.0], [0.0], tr, [len(m['tr'])])
    assert int(res['status'][0]) == 1 and bool(torch.isnan(res['weights'][0, :W]).all())


def _markov_days(D, Hd, d, seed):
    """Days from a fixed random row-stochastic P: pi' = pi P with 2 % multiplicative noise, renormalised."""
    rs = np.random.RandomState(seed)
    P = rs.dirichlet(np.ones(d), d)
    days = np.empty((D, Hd, d))
    for i in range(D):
        y = rs.dirichlet(np.ones(d))
        for h in range(Hd):
            if h:
                y = np.abs((y @ P) * (1 + 0.02 * rs.randn(d)))
                y /= y.sum()
            days[i, h] = y
    return days


def test_it_learns(M):
    """The test that a plausible-looking but wrong backward pass fails: d = 5, H = 8, 6 training and 2 test days of a noisy Markov
    chain, 300 Adam epochs at lr 1e-2.  Conditions, not measurements: the excess of the training loss over the data's entropy
    floor falls to at most 10 % of its start, and the test JSD_mean is at most 1/10 of the persistence forecast's.  (The
    restatement reaches 0.9 % and 1/260 here.)  The weights are not compared after 300 epochs."""
    from discrete_mean_field_game_amd import rnn
    days = _markov_days(8, 16, 5, 7)
    fits = rnn.fit_population(days, [8], 1e-2, 300, list(range(6)), None, [6, 7], device=M.dev)
    assert fits.status[0] == 0 and fits.best_epoch[0] == 300
    Y = days[:6]
    floor = float(-(Y[:, 1:] * np.log(Y[:, 1:])).sum(axis=2).mean())
    excess = fits.loss[0] - floor
    persistence = R.metrics(np.repeat(days[6:8, :1], 16, axis=1), days[6:8])[1][6]
    print('excess %.4f -> %.5f (%.2f %%), JSD_mean %.2e against persistence %.3f (1/%.0f)'
          % (excess[0], excess[-1], 100 * excess[-1] / excess[0], fits.metrics[0, 6], persistence, persistence / fits.metrics[0, 6]))
    assert excess[0] > 0 and excess[-1] <= 0.1 * excess[0]
    assert fits.metrics[0, 6] <= persistence / 10


def test_cross_validation_puts_every_model_in_one_call(M, monkeypatch):
    from discrete_mean_field_game_amd import ops, rnn
    days = _markov_days(8, 16, 5, 7)
    calls = []
    real = ops.rnn_fit_pop
    monkeypatch.setattr(ops, 'rnn_fit_pop', lambda *a, **kw: calls.append(len(a[2])) or real(*a, **kw))
    cv = rnn.cross_validation(days, [4, 8], [1e-2, 1e-3], validation_size=2, repetitions=3, epochs=20, split_seed=3, device=M.dev)
    assert calls == [12] and cv['mean'].shape == (2, 2) and np.isfinite(cv['mean']).all() and (cv['std'] >= 0).all()
    fits = cv['fits']
    assert np.allclose(cv['mean'][1, 0], fits.metrics[6:9, 6].mean()) and cv['best'] in [(h, l) for h in (4, 8) for l in (1e-2, 1e-3)]
    # the forecast goes to the proper scores unchanged
    t = fits.traj(0)
    assert t.shape == (2, 16, 5) and t.dtype == np.float32
