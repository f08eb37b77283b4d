"""The VAR population call restated in NumPy from the definitions of include/mfg_hip.h (mfg_var_fit_pop): the yardstick of
tests/test_gpu_var_pop.py, test_gpu_var_class.py and test_var_host.py.  Every function takes a dtype, so that it also runs in
np.longdouble (the restatement's own rounding error is measured as fp64 against longdouble).  statsmodels is not a yardstick
here: the project does not depend on it, and the reference's var.py cannot run on a current pandas (.ix, pd.rolling_mean)."""
import numpy as np

U = 2.0 ** -53

# (d, lag, training days); Hd = 16 and 3 test days everywhere
CASES = [(3, 1, 2),        # m = 4: the smallest
         (3, 5, 6),        # m = 16: exactly one tile
         (15, 2, 8),       # m = 31: a ragged tile
         (15, 9, 8),       # m = 136 > n = 119: underdetermined, nine panels
         (21, 5, 6),       # m = 106 > n = 91: underdetermined
         (15, 20, 13),     # m = 301: the largest lag of the reference's range
         (64, 7, 4)]       # m = 449: near the cap, d at its limit
HD, N_TEST = 16, 3
RIDGES = (1e-8, 1e-2)


def case_id(c):
    return 'd%d-p%d-n%d' % c


def synthetic_days(D, Hd, d, seed):
    """[D, Hd, d] fp64: rows on the simplex drifting toward an hour-dependent target around a Zipf profile,
    y <- 0.8 y + 0.2 target_h + 0.02 Dirichlet noise, renormalised; each day starts from Dirichlet(200 q)."""
    rs = np.random.RandomState(seed)
    q = 1.0 / np.arange(1, d + 1)
    q /= q.sum()
    targets = np.stack([q * (1.0 + 0.5 * np.sin(2 * np.pi * (h / Hd + np.arange(d) / d))) for h in range(Hd)])
    targets /= targets.sum(axis=1, keepdims=True)
    days = np.empty((D, Hd, d))
    for i in range(D):
        y = rs.dirichlet(200.0 * q)
        for h in range(Hd):
            if h:
                y = 0.8 * y + 0.2 * targets[h] + 0.02 * rs.dirichlet(np.ones(d))
                y = y / y.sum()
            days[i, h] = y
    return days


def series(days, idx, dtype=np.float64):
    """The days `idx` of the table concatenated in list order: [len(idx) Hd, d]."""
    days = np.asarray(days)
    return days[np.asarray(idx, dtype=np.int64)].reshape(-1, days.shape[2]).astype(dtype)


def design(Y, p, dtype=np.float64):
    """(Z [n, 1 + p d], targets [n, d]) of the series Y [T, d]: row t - p of Z is [1, y_{t-1}, ..., y_{t-p}], t = p .. T-1."""
    Y = np.asarray(Y, dtype=dtype)
    T = Y.shape[0]
    Z = np.concatenate([np.ones((T - p, 1), dtype=dtype)] + [Y[p - l:T - l] for l in range(1, p + 1)], axis=1)
    return Z, Y[p:]


def gram(Y, p, lam, dtype=np.float64):
    Z, X = design(Y, p, dtype)
    return Z.T @ Z + dtype(lam) * np.eye(Z.shape[1], dtype=dtype), Z.T @ X


def ridge_fit(Y, p, lam, dtype=np.float64):
    """B [1 + p d, d] = (Z'Z + lam I)^-1 Z'Y.  np.linalg.solve has no longdouble form: there the fp64 solution is refined in
    longdouble until its residual is at the longdouble level."""
    G, C = gram(Y, p, lam, dtype)
    if dtype is not np.longdouble:
        return np.linalg.solve(G, C)
    G64 = G.astype(np.float64)
    B = np.linalg.solve(G64, C.astype(np.float64)).astype(np.longdouble)
    for _ in range(6):
        B = B + np.linalg.solve(G64, (C - G @ B).astype(np.float64)).astype(np.longdouble)
    return B


def fitted(Y, p, B, dtype=np.float64):
    Z, X = design(Y, p, dtype)
    return Z @ np.asarray(B, dtype=dtype), X


def jsd(P, Q, dtype=np.float64):
    """var.py:175-192 on the last axis; the inputs are not modified."""
    P, Q = np.array(P, dtype=dtype), np.array(Q, dtype=dtype)
    P[P <= 0] = dtype(1e-100)
    Q[Q <= 0] = dtype(1e-100)
    M = dtype(0.5) * (P + Q)
    n = lambda a: a / a.sum(axis=-1, keepdims=True)
    kl = lambda a, b: np.sum(n(a) * np.log(n(a) / n(b)), axis=-1)
    return dtype(0.5) * (kl(P, M) + kl(Q, M))


def insample(Y, p, B, dtype=np.float64):
    """(sse [d], [mean L1, mean JSD]) of the fitted rows."""
    F, X = fitted(Y, p, B, dtype)
    return np.sum((X - F) ** 2, axis=0), np.array([np.abs(X - F).sum(axis=1).mean(), jsd(X, F, dtype).mean()], dtype=dtype)


def forecast(train, test, p, B, origin, Hd, dtype=np.float64):
    """[S, d]: origin 0 -- one path from the last p training rows, fed by its own outputs; origin 1 -- per test day the history
    is [train | test days before | hour 0 of the day], hour 0 of the output is the observed row."""
    train, test, B = np.asarray(train, dtype=dtype), np.asarray(test, dtype=dtype), np.asarray(B, dtype=dtype)
    S, d = test.shape
    out = np.empty((S, d), dtype=dtype)
    step = lambda h: np.concatenate([np.ones(1, dtype=dtype)] + [h[-l] for l in range(1, p + 1)]) @ B
    if origin == 0:
        hist = [r for r in train[-p:]]
        for s in range(S):
            out[s] = step(hist)
            hist = hist[1:] + [out[s]]
        return out
    ext = np.concatenate([train, test])
    T = train.shape[0]
    for j in range(S // Hd):
        s0 = j * Hd
        out[s0] = test[s0]
        hist = [r for r in ext[T + s0 + 1 - p:T + s0 + 1]]
        for h in range(1, Hd):
            out[s0 + h] = step(hist)
            hist = hist[1:] + [out[s0 + h]]
    return out


def metrics(future, test, Hd, dtype=np.float64):
    """(per_day [N, 4] = l1_final, l1_mean, JSD_final, JSD_mean; metrics [8] = mean, np.std of each over the days)."""
    future, test = np.asarray(future, dtype=dtype), np.asarray(test, dtype=dtype)
    N = test.shape[0] // Hd
    l1 = np.abs(test - future).sum(axis=1).reshape(N, Hd)
    js = jsd(test, future, dtype).reshape(N, Hd)
    per_day = np.stack([l1[:, -1], l1.mean(axis=1), js[:, -1], js.mean(axis=1)], axis=1)
    return per_day, np.stack([per_day.mean(axis=0), per_day.std(axis=0)], axis=1).reshape(-1)


def model(days, train_idx, test_idx, p, lam, origin, dtype=np.float64, B=None):
    """Everything mfg_var_fit_pop returns for one model, as a dict; B given: everything downstream of those coefficients."""
    Hd = np.asarray(days).shape[1]
    Y, X = series(days, train_idx, dtype), series(days, test_idx, dtype)
    B = ridge_fit(Y, p, lam, dtype) if B is None else np.asarray(B, dtype=dtype)
    sse, ins = insample(Y, p, B, dtype)
    out = {'coef': B, 'sse': sse, 'insample': ins}
    if len(test_idx):
        out['future'] = forecast(Y, X, p, B, origin, Hd, dtype)
        out['per_day'], out['metrics'] = metrics(out['future'], X, Hd, dtype)
    return out


def case_days(case, seed=None):
    """The day table of a case and its lists: (days [n_train + 3, 16, d], train_idx, test_idx)."""
    d, p, n_train = case
    days = synthetic_days(n_train + N_TEST, HD, d, 1000 + 7 * d + p if seed is None else seed)
    return days, list(range(n_train)), list(range(n_train, n_train + N_TEST))


_GAP = {}


def longdouble_gap(case, lam, origin):
    """max |forecast in fp64 - forecast in longdouble| of the restatement, both from the SAME coefficients (the fp64 fit): its
    own rounding error over the S steps.  Cached."""
    key = (case, lam, origin)
    if key not in _GAP:
        days, tr, te = case_days(case)
        p = case[1]
        Y, X = series(days, tr), series(days, te)
        B = ridge_fit(Y, p, lam)
        a = forecast(Y, X, p, B, origin, HD)
        b = forecast(Y, X, p, B, origin, HD, np.longdouble)
        _GAP[key] = float(np.max(np.abs(a - b)))
    return _GAP[key]


def forecast_tolerance(Y, X, p, lam, origin, Hd, B_dev):
    """[S, d]: what a forecast from the coefficients B_dev may differ by from forecast(Y, X, p, B_dev, ...): 64 x the
    restatement's own fp64-against-longdouble gap on this problem (measured on its own fit, never on the code under test; the
    margin covers fused multiply-add and another summation tree) plus the dot-product floor 4 m u |z|'|B_dev| of each step."""
    B = ridge_fit(Y, p, lam)
    gap = float(np.max(np.abs(forecast(Y, X, p, B, origin, Hd) - forecast(Y, X, p, B, origin, Hd, np.longdouble))))
    ref = forecast(Y, X, p, B_dev, origin, Hd)
    S, d = X.shape
    m = 1 + p * d
    floor = np.zeros((S, d))
    true, own = np.concatenate([Y, X]), np.concatenate([Y, ref])
    for s in range(S):
        s0 = s - s % Hd                              # (origin 1: rows up to the day's hour 0 are observed, later ones forecast)
        if origin == 1 and s == s0:
            continue                                 # the observed row itself: exact
        rows = [(own if origin == 0 or s - l > s0 else true)[len(Y) + s - l] for l in range(1, p + 1)]
        floor[s] = 4 * m * U * (np.abs(np.concatenate([[1.0]] + rows)) @ np.abs(B_dev))
    return 64 * gap + floor
