"""The VAR baseline of the paper's comparison (the reference's var.py), fitted as ONE population on the device.

fit_population() fits, forecasts and scores K independent vector autoregressions -- each with its own lag, ridge and days -- in
the three launches of one ops.var_fit_pop call per chunk; `var` is a drop-in for the reference's class on top of it, whose
cross_validation puts all len(lag_range) x repetitions models into one such call.

Two deliberate deviations from the reference ("The VAR baseline"):
  * The fit is RIDGE regression, B = (Z'Z + ridge I)^-1 Z'Y, not statsmodels' minimum-norm lstsq.  The rows are histograms that
    sum to 1, so the constant column equals the sum of every lag block and Z'Z is singular for every shape; with ridge > 0 the
    problem is well posed and factors by Cholesky, and B tends to the minimum-norm solution as ridge -> 0.
  * No information criterion: the reference's train() hands `ic='aic'` to statsmodels, which takes the logarithm of the
    determinant of a residual covariance that is exactly singular here (residuals sum to 0 over topics).  train(max_lag) fits
    order max_lag; the order is chosen by held-out error, which is what cross_validation does.
Parity with statsmodels is unpinned: it is no dependency of this project and the reference's var.py needs pandas calls that no
longer exist, so the yardstick of the tests is a NumPy restatement of the definitions in include/mfg_hip.h (tests/var_ref.py).
Not built: check_stationarity (adfuller) and plot (a figure).
"""
from __future__ import annotations

import numpy as np

from . import _lib as L

ORIGINS = {'train_end': 0, 'rolling': 1, 0: 0, 1: 1}
METRIC_NAMES = ('l1_final', 'l1_mean', 'JSD_final', 'JSD_mean')


def _per_model(name, value, K, dtype):
    a = np.asarray(value, dtype=dtype).reshape(-1)
    if a.shape[0] == 1:
        a = np.repeat(a, K)
    if a.shape[0] != K:
        raise ValueError('%s: one value or one per model (%d), got %d' % (name, K, a.shape[0]))
    return a


def _day_lists(name, lists, K, D, allow_empty):
    """K lists of day indices from one list (shared by every model) or K lists; each index inside [0, D)."""
    if lists is None:
        lists = [[] for _ in range(K)]
    lists = list(lists)
    if len(lists) and not hasattr(lists[0], '__len__'):
        lists = [lists] * K
    if len(lists) != K:
        raise ValueError('%s: one list of days or one per model (%d), got %d' % (name, K, len(lists)))
    out = []
    for k, days in enumerate(lists):
        idx = np.asarray(list(days), dtype=np.int64).reshape(-1)
        if idx.size == 0 and not allow_empty:
            raise ValueError('%s: model %d has no day' % (name, k))
        if idx.size and (idx.min() < 0 or idx.max() >= D):
            raise ValueError('%s: model %d names a day outside [0, %d)' % (name, k, D))
        out.append(idx)
    return out


def _table(lists, width):
    t = np.zeros((len(lists), max(width, 1)), dtype=np.int32)
    for k, idx in enumerate(lists):
        t[k, :idx.size] = idx
    return t


def model_bytes(M, S_max, n_test, d):
    """An upper bound of the device bytes one model of a fit_population chunk needs: its workspace slice and its outputs."""
    return (64 + (M + d) * M * 8 + 255) // 256 * 256 + 8 * (M * d + d + 2 + S_max * d + 4 * n_test + 8) + 4


def check_population_args(days, lags, ridges, train_days, test_days, origin):
    """The argument rules of fit_population, without a GPU (ValueError).  Returns (days, lags, ridges, train lists, test lists,
    origins, (K, D, Hd, d, M, S_max))."""
    from . import ops
    days = np.ascontiguousarray(days, dtype=np.float64)
    lags = np.asarray(lags, dtype=np.int64).reshape(-1)
    K = lags.shape[0]
    if K < 1:
        raise ValueError('no models')
    if days.ndim != 3:
        raise ValueError('days: expected [D, Hd, d], got %s' % (days.shape,))
    ridges = _per_model('ridges', ridges, K, np.float64)
    orgs = [origin] * K if isinstance(origin, (str, int)) else list(origin)
    if len(orgs) != K or any(o not in ORIGINS for o in orgs):
        raise ValueError("origin: 'train_end' or 'rolling', one or one per model")
    orgs = np.array([ORIGINS[o] for o in orgs], dtype=np.int32)
    tr = _day_lists('train_days', train_days, K, days.shape[0], False)
    te = _day_lists('test_days', test_days, K, days.shape[0], True)
    n_tr, n_te = [t.size for t in tr], [t.size for t in te]
    M = S_max = 0
    for c0 in range(0, K, L.POP_MAX_K):      # (per-model rules and the limit of one call; fit_population's chunks are never larger)
        s = slice(c0, c0 + L.POP_MAX_K)
        _, D, Hd, d, Mc, Sc = ops.check_var_fit_args(days.shape, lags[s], ridges[s], n_tr[s], n_te[s], orgs[s])
        M, S_max = max(M, Mc), max(S_max, Sc)
    return days, lags, ridges, tr, te, orgs, (K, D, Hd, d, M, S_max)


class VarFits:
    """The result of fit_population (NumPy): coef [K, M, d] (rows >= 1 + lag d zero), sse [K, d], insample [K, 2] (mean L1,
    mean JSD over the fitted rows), future [K, S_max, d], per_day [K, Nt_max, 4] (l1_final, l1_mean, JSD_final, JSD_mean per test
    day), metrics [K, 8] (mean, std over the test days of each), status [K] (bit 0: non-finite input, bit 1: Cholesky pivot;
    a model with status != 0 is NaN everywhere)."""

    def __init__(self, out, lags, ridges, origins, n_test, hours, d):
        for name in ('coef', 'sse', 'insample', 'future', 'per_day', 'metrics', 'status'):
            setattr(self, name, out[name])
        self.lags, self.ridges, self.origins, self.n_test, self.hours, self.d = lags, ridges, origins, n_test, int(hours), int(d)

    def __len__(self):
        return int(self.status.shape[0])

    def model(self, k):
        """Model k alone: intercept [d], lag matrices A [lag, d, d] with y_t = intercept + sum_l A[l-1] y_{t-l} (A[l-1][i, j] the
        weight of topic j at lag l on topic i), and its cropped outputs."""
        p, d = int(self.lags[k]), self.d
        B = self.coef[k, :1 + p * d]
        S = int(self.n_test[k]) * self.hours
        return {'lag': p, 'ridge': float(self.ridges[k]), 'origin': int(self.origins[k]), 'status': int(self.status[k]),
                'intercept': B[0].copy(), 'A': B[1:].reshape(p, d, d).transpose(0, 2, 1).copy(), 'sse': self.sse[k].copy(),
                'insample': self.insample[k].copy(), 'future': self.future[k, :S].copy(),
                'per_day': self.per_day[k, :int(self.n_test[k])].copy(), 'metrics': self.metrics[k].copy()}

    def traj(self, k):
        """Model k's rolling-origin forecast as [N, Hd, d] fp32 -- N test days, hour 0 the observed row --, the member layout of
        ops.forecast_score: with repeats = 1 that scorer takes traj(k)[None] unchanged."""
        if int(self.origins[k]) != 1:
            raise ValueError("model %d was forecast from the end of its training series: traj() is the origin='rolling' forecast" % k)
        N = int(self.n_test[k])
        return self.future[k, :N * self.hours].reshape(N, self.hours, self.d).astype(np.float32)


def fit_population(days, lags, ridges, train_days, test_days=None, origin='train_end', *, budget=None, device=None):
    """Fit, forecast and score K VAR models on the device.  days [D, Hd, d]: a table of day matrices; lags [K]; ridges: one
    value or [K], each > 0; train_days / test_days: one list of day indices for every model or K lists (test_days None: no
    forecast); origin 'train_end' (one path of n_test Hd steps from the end of the training series, as the reference's
    forecast / validation) or 'rolling' (every test day forecast from its observed hour 0, its history the training series and
    the test days before it -- what population.forecast is given), one or K.  NumPy in, a VarFits out.  Models go in chunks
    whose workspaces and outputs stay within `budget` bytes (population.consistency_chunks; None: its default); chunking
    changes no bit.  Runs on a context of its own."""
    import torch
    from . import ops
    from .population import consistency_chunks
    days, lags, ridges, tr, te, orgs, (K, D, Hd, d, M, S_max) = check_population_args(days, lags, ridges, train_days, test_days, origin)
    n_tr, n_te = np.array([t.size for t in tr]), np.array([t.size for t in te])
    chunks = consistency_chunks(K, model_bytes(M, S_max, int(n_te.max()), d), budget)
    if not torch.cuda.is_available():
        raise L.MfgError('fit_population needs a ROCm GPU: the HIP hot path has no CPU fallback')
    dev = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
    tr_tab, te_tab = _table(tr, int(n_tr.max())), _table(te, int(n_te.max()))
    ctx = ops.Context(dev)
    prev = ctx.bind_scoped()
    try:
        with torch.cuda.device(dev):
            days_dev = torch.as_tensor(days, device=dev)
            parts = []
            for c0, n in chunks:
                s = slice(c0, c0 + n)
                res = ops.var_fit_pop(days_dev, lags[s], ridges[s], torch.as_tensor(tr_tab[s].copy(), device=dev), n_tr[s],
                                      torch.as_tensor(te_tab[s].copy(), device=dev) if n_te.max() else None, n_te[s], orgs[s],
                                      M=M, S_max=S_max)
                parts.append({name: t.cpu().numpy() for name, t in res.items()})
    finally:
        ctx.restore(prev)
        ctx.close()
    out = {name: np.concatenate([p[name] for p in parts]) for name in parts[0]}
    return VarFits(out, lags, ridges, orgs, n_te, Hd, d)


def _hours(*lengths):
    """Rows per day for series of these lengths: the largest common divisor <= 64 that leaves each at most 64 days (the summation
    orders do not depend on it: lags run across day boundaries)."""
    for h in range(min(64, *lengths), 0, -1):
        if all(n % h == 0 and n // h <= 64 for n in lengths):
            return h
    raise ValueError('series of %s rows do not split into at most 64 days of one length <= 64' % (lengths,))


class VarResults:
    """What train() keeps of a fit: k_ar (the order), intercept [d], coefs [k_ar, d, d], params [1 + k_ar d, d], sse, insample."""

    def __init__(self, fits):
        m = fits.model(0)
        self.k_ar, self.intercept, self.coefs = m['lag'], m['intercept'], m['A']
        self.params = fits.coef[0, :1 + m['lag'] * fits.d].copy()
        self.sse, self.insample, self.status = m['sse'], m['insample'], m['status']

    def fitted(self, series, t):
        """The fitted row t >= k_ar of `series` [T, d] (host arithmetic, for the few rows evaluate_train's part 1 looks at)."""
        z = np.concatenate([[1.0]] + [series[t - l] for l in range(1, self.k_ar + 1)])
        return z @ self.params


class var:
    """Drop-in for the reference's var class (var.py:15-416) on the device population call.  The fit is ridge regression of
    order max_lag (the module docstring says why); check_stationarity and plot are not built."""

    hours = 16        # rows per day file (var.py hard-codes 16)

    def __init__(self, d=15, device=None):
        self.d = d
        self.device = device
        self.ridge = 1e-8

    def read_data(self, train='train_normalized_round2', train_start=1, train_end=18, test='test_normalized_round2', test_start=19,
                  test_end=24, old_format=False):
        """var.py:26-75: the day files of two directories as two DataFrames indexed by consecutive days."""
        import pandas as pd
        name = 'trend_distribution_day%d_reordered.csv' if old_format else 'trend_distribution_day%d.csv'
        idx = 0
        frames = {}
        for key, folder, first, last in (('train', train, train_start, train_end), ('test', test, test_start, test_end)):
            print('Reading %s files' % key)
            parts = []
            for num_day in range(first, last + 1):
                df = pd.read_csv(folder + '/' + name % num_day, sep=' ', header=None, names=range(self.d), usecols=range(self.d),
                                 dtype=np.float64)
                df.index = np.arange(idx, idx + self.hours)
                parts.append(df)
                idx += self.hours
            df = pd.concat(parts) if parts else pd.DataFrame()
            df.index = pd.to_datetime(df.index, unit='D')
            frames[key] = df
        self.df_train, self.df_test = frames['train'], frames['test']
        return self.df_train, self.df_test

    @staticmethod
    def _values(df):
        return np.ascontiguousarray(getattr(df, 'values', df), dtype=np.float64)

    def _day_rows(self, *lengths):
        """Rows per day of series of these lengths: the files' 16 when that splits them, else _hours' choice."""
        if all(n % self.hours == 0 and n // self.hours <= 64 for n in lengths):
            return self.hours
        return _hours(*lengths)

    def _fit(self, lag, train, test=None, origin='train_end'):
        train = self._values(train)
        if train.ndim != 2:
            raise ValueError('a training series is [T, d], got %s' % (train.shape,))
        d = train.shape[1]
        if test is None or len(test) == 0:
            h = self._day_rows(train.shape[0])
            return fit_population(train.reshape(-1, h, d), [lag], self.ridge, list(range(train.shape[0] // h)), device=self.device)
        test = self._values(test)
        h = self._day_rows(train.shape[0], test.shape[0])
        n_tr, n_te = train.shape[0] // h, test.shape[0] // h
        days = np.concatenate([train, test]).reshape(-1, h, d)
        return fit_population(days, [lag], self.ridge, list(range(n_tr)), list(range(n_tr, n_tr + n_te)), origin, device=self.device)

    def train(self, max_lag, df_train, *, ridge=1e-8):
        """Fit the VAR of order max_lag on df_train (a DataFrame or an array [T, d]) by ridge regression.  Unlike var.py:102-106
        no information criterion picks a smaller order."""
        if not (ridge > 0.0 and np.isfinite(ridge)):
            raise ValueError('ridge=%r must be finite and > 0' % (ridge,))
        self.ridge = float(ridge)
        self._train = self._values(df_train).copy()
        self.results = VarResults(self._fit(int(max_lag), self._train))
        return self.results

    def JSD(self, P, Q):
        """var.py:175-192 without its side effect on the arguments: entries <= 0 become 1e-100, then 1/2 (KL(P||M) + KL(Q||M)) with
        M = (P + Q) / 2, every argument renormalised as scipy.stats.entropy does."""
        P, Q = np.array(P, dtype=np.float64), np.array(Q, dtype=np.float64)
        P[P <= 0] = 1e-100
        Q[Q <= 0] = 1e-100
        M = 0.5 * (P + Q)
        kl = lambda a, b: float(np.sum(a / a.sum() * np.log((a / a.sum()) / (b / b.sum()))))
        return 0.5 * (kl(P, M) + kl(Q, M))

    def evaluate_train(self):
        """var.py:195-255: L1 and JSD between the training rows and the fitted rows -- at each day's final hour (part 1) and as the
        means over every fitted row (part 2, from the device).  Returns (mean_l1_final, mean_JSD_final, mean_l1, mean_JSD)."""
        lag, series, H = self.results.k_ar, self._train, self.hours
        finals = [t for t in range(H - 1, series.shape[0], H) if t >= lag]
        l1 = np.array([np.abs(series[t] - self.results.fitted(series, t)).sum() for t in finals])
        jsd = np.array([self.JSD(series[t], self.results.fitted(series, t)) for t in finals])
        out = (float(l1.mean()), float(jsd.mean()), float(self.results.insample[0]), float(self.results.insample[1]))
        print(l1)
        print(jsd)
        for x in out:
            print(x)
        return out

    def validation(self, steps, df_selected, df_validation):
        """var.py:258-291: the mean over the validation days of the mean JSD over the hours of a `steps`-row forecast from the end
        of df_selected (the order is that of the last train())."""
        val = self._values(df_validation)
        if int(steps) != val.shape[0]:
            raise ValueError('steps=%d, the validation set has %d rows' % (steps, val.shape[0]))
        fits = self._fit(self.results.k_ar, df_selected, val)
        return float(fits.metrics[0, 6])

    def forecast(self, num_prior=416, steps=176, topic=0, plot=1, show_plot=1):
        """var.py:294-327: `steps` rows from the end of the training series (num_prior >= the order rows feed it, as statsmodels
        uses the last k_ar of them).  Returns and keeps df_future; with a test set of `steps` rows the device also scores it
        (evaluate_test)."""
        import pandas as pd
        lag, T = self.results.k_ar, self._train.shape[0]
        if num_prior < lag:
            raise ValueError('num_prior=%d rows cannot feed a VAR of order %d' % (num_prior, lag))
        test = self._values(self.df_test) if getattr(self, 'df_test', None) is not None and len(self.df_test) == steps else None
        scored = test is not None
        if not scored:
            test = np.zeros((int(steps), self._train.shape[1]))
        self._fits = self._fit(lag, self._train, test)
        self._scored = scored
        self.df_future = pd.DataFrame(self._fits.future[0, :steps].copy())
        self.df_future.index = pd.to_datetime(np.arange(T, T + steps), unit='D')
        if plot == 1:
            import matplotlib.pylab as plt
            x_train, x_test = np.arange(T), np.arange(T, T + steps)
            fitted = np.array([self.results.fitted(self._train, t)[topic] for t in range(lag, T)])
            plt.plot(x_train, self._train[:, topic], color='r', linestyle='-', label='train data')
            plt.plot(x_train[lag:], fitted, color='b', linestyle='--', label='time series (train)')
            if scored:
                plt.plot(x_test, test[:, topic], color='k', linestyle='-', label='test data')
            plt.plot(x_test, self.df_future[topic], color='g', linestyle='--', label='time series (test)')
            plt.ylabel('Topic %d popularity' % topic)
            plt.xlabel('Time steps (hrs)')
            plt.legend(loc='best')
            plt.title('Topic %d data and fitted time series' % topic)
            if show_plot == 1:
                plt.show()
        return self.df_future

    def evaluate_test(self, outfile='eval_var_round2/test.csv'):
        """var.py:330-416: the per-day arrays of the last forecast() against df_test, their means and standard deviations, in the
        reference's sixteen np.savetxt lines."""
        if not getattr(self, '_scored', False):
            print('Lengths of test set and generated future differ!')
            return None
        n = int(self._fits.n_test[0])
        if self._fits.hours != self.hours:      # (per-day values need the day length of the files)
            raise ValueError('the forecast was split into days of %d rows, the files have %d' % (self._fits.hours, self.hours))
        per_day = self._fits.per_day[0, :n]
        arrays = {name: per_day[:, q].copy() for q, name in enumerate(METRIC_NAMES)}
        print('Mean L1 final', np.mean(arrays['l1_final']))
        print('Mean JSD final', np.mean(arrays['JSD_final']))
        print('Mean L1 mean', np.mean(arrays['l1_mean']))
        print('Mean JSD mean', np.mean(arrays['JSD_mean']))
        with open(outfile, 'ab') as f:
            for name in METRIC_NAMES:
                a = arrays[name]
                np.savetxt(f, np.array(['array_' + name]), fmt='%s')
                np.savetxt(f, np.array([np.mean(a)]), fmt='%.3e')
                np.savetxt(f, np.array([np.std(a)]), fmt='%.3e')
                np.savetxt(f, a.reshape(1, n), delimiter=',', fmt='%.3e')
        return arrays

    @staticmethod
    def splits(num_days, validation_size, n, rng=None):
        """The n random splits of var.py:126-127 in order: (selected, the_rest) per split, drawn with np.random.choice on the
        global state (rng None) or on a RandomState."""
        choice = np.random.choice if rng is None else rng.choice
        choices = range(num_days)
        out = []
        for _ in range(n):
            selected = choice(choices, num_days - validation_size, replace=False)
            out.append((selected, [x for x in choices if x not in selected]))
        return out

    def cross_validation(self, lag_range=range(1, 21), validation_size=5, repetitions=5, *, ridge=1e-8, seed=None,
                         outfile='eval_var_round2/var_cross_validation.csv'):
        """var.py:109-162: for every lag, `repetitions` random splits of the training days into a fitted and a held-out part,
        scored by the mean JSD of the forecast of the held-out days.  The splits are the reference's draws (seed None: the
        global NumPy state; else RandomState(seed)); all len(lag_range) x repetitions models run in ONE fit_population call.
        Appends the reference's two CSV lines to outfile and returns (best_lag, list_error)."""
        lag_range = list(lag_range)
        series = self._values(self.df_train)
        H, d = self.hours, series.shape[1]
        num_days = series.shape[0] // H
        if not 1 <= validation_size < num_days:
            raise ValueError('validation_size=%d of %d training days' % (validation_size, num_days))
        if not lag_range or repetitions < 1:
            raise ValueError('no lag or no repetition')
        rng = None if seed is None else np.random.RandomState(seed)
        splits = self.splits(num_days, validation_size, len(lag_range) * repetitions, rng)
        lags = np.repeat(lag_range, repetitions)
        fits = fit_population(series[:num_days * H].reshape(num_days, H, d), lags, ridge, [s for s, _ in splits],
                              [r for _, r in splits], device=self.device)
        list_error = []
        for i, lag in enumerate(lag_range):
            print('Lag %d' % lag)
            avg_error = 0
            for rep in range(repetitions):
                avg_error += fits.metrics[i * repetitions + rep, 6]
            avg_error = avg_error / repetitions
            print('Lag %d. avg_error' % lag, avg_error)
            list_error.append(avg_error)
        best = lag_range[int(np.argmin(list_error))]
        print('Min error is', np.min(list_error))
        print('Best lag value is', best)
        with open(outfile, 'a') as f:
            f.write(','.join(map(str, lag_range)) + '\n')
            f.write(','.join(map(str, list_error)) + '\n')
        self.cv_fits = fits
        return best, list_error
