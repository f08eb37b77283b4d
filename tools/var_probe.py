#!/usr/bin/env python3
"""GPU: the VAR cross-validation as one population call, against the two ways to do without it.  The shape is the reference's
cross_validation (var.py:109-162): d = 15, 18 training days of 16 hours, 5 random splits into 13 fitted and 5 held-out days for
each lag 1 .. 20 -- 100 models, each fitted, forecast over 80 rows and scored.
  call   one var.fit_population call (uploads, three launches, read-back), host clock around it; and the device part alone,
         ops.var_fit_pop on resident buffers, event-timed
  (a)    the same 100 models one after another on the host: np.linalg.lstsq on the ridge-augmented system [Z; sqrt(lambda) I],
         the forecast recursion and the JSD in NumPy
  (b)    the FIT stage alone with torch on the same device, batched per lag (5 models): Z gathered on the device, Z'Z + lambda I
         and Z'Y by bmm, torch.linalg.cholesky + torch.cholesky_solve -- to be held against the call's k_var_gram + k_var_solve
         (the kernel table: rocprofv3 --kernel-trace --stats -- python tools/var_probe.py --kernels-only)
Alternating rounds, medians.  Then the backward error eta of the call's coefficients on the cases of tests/var_ref.py.
python tools/var_probe.py [--rounds 7] [--out profiles/var_pop.txt] [--kernels-only]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from discrete_mean_field_game_amd import ops, var as V  # noqa: E402
import var_ref as R  # noqa: E402

D_TOPICS, HD, DAYS, HELD, REPS, LAGS, RIDGE = 15, 16, 18, 5, 5, list(range(1, 21)), 1e-8


def event_ms(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e)


def host_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def host_models(days, lags, splits):
    """(a): every model on the host; returns the per-model mean JSD (the number cross_validation averages)."""
    out = []
    for p, (sel, rest) in zip(lags, splits):
        Y, X = R.series(days, sel), R.series(days, rest)
        Z, T = R.design(Y, p)
        m = Z.shape[1]
        B = np.linalg.lstsq(np.concatenate([Z, np.sqrt(RIDGE) * np.eye(m)]), np.concatenate([T, np.zeros((m, T.shape[1]))]),
                            rcond=None)[0]
        out.append(R.metrics(R.forecast(Y, X, p, B, 0, HD), X, HD)[1][6])
    return np.array(out)


def torch_fit(days_dev, lags, splits, dev):
    """(b): the coefficients alone, batched per lag."""
    out = []
    for i in range(0, len(lags), REPS):
        p = int(lags[i])
        idx = torch.as_tensor(np.stack([s for s, _ in splits[i:i + REPS]]), device=dev)
        Y = days_dev[idx].reshape(REPS, -1, D_TOPICS)                                      # [5, T, d]
        T = Y.shape[1]
        Z = torch.cat([torch.ones(REPS, T - p, 1, dtype=torch.float64, device=dev)] + [Y[:, p - l:T - l] for l in range(1, p + 1)], 2)
        G = Z.transpose(1, 2) @ Z + RIDGE * torch.eye(Z.shape[2], dtype=torch.float64, device=dev)
        out.append(torch.cholesky_solve(Z.transpose(1, 2) @ Y[:, p:], torch.linalg.cholesky(G)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--out', default=None)
    ap.add_argument('--kernels-only', action='store_true', help='three device calls and nothing else: the run to put under rocprofv3')
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    days = R.synthetic_days(DAYS, HD, D_TOPICS, 2024)
    lags = np.repeat(LAGS, REPS)
    splits = V.var.splits(DAYS, HELD, len(lags), np.random.RandomState(0))
    K = len(lags)
    # the device part alone, on resident buffers
    days_dev = torch.as_tensor(days, device=dev)
    ntr, nte = [DAYS - HELD] * K, [HELD] * K
    table, nbytes = ops.var_models(lags, [RIDGE] * K, ntr, nte, [0] * K, D_TOPICS)
    models = (table, ops.var_models_device(table, dev), nbytes)
    tr = torch.as_tensor(np.stack([s for s, _ in splits]).astype(np.int32), device=dev)
    te = torch.as_tensor(np.array([r for _, r in splits], dtype=np.int32), device=dev)
    shapes = ops.var_fit_shapes(K, D_TOPICS, 1 + 20 * D_TOPICS, HELD * HD, HELD)
    bufs = {n: torch.empty(s, dtype=t, device=dev) for n, (s, t) in shapes.items()}
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
    device_call = lambda: ops.var_fit_pop(days_dev, lags, [RIDGE] * K, tr, ntr, te, nte, [0] * K, out=bufs, workspace=ws, models=models)
    for _ in range(3):
        device_call()
    torch.cuda.synchronize()
    if a.kernels_only:
        return
    whole_call = lambda: V.fit_population(days, lags, RIDGE, [s for s, _ in splits], [r for _, r in splits])
    fits = whole_call()
    torch_fit(days_dev, lags, splits, dev)
    ref = host_models(days, lags, splits)
    t = {'call': [], 'device': [], 'a': [], 'b': []}
    for _ in range(a.rounds):
        t['call'].append(host_ms(whole_call))
        t['device'].append(event_ms(device_call))
        t['b'].append(event_ms(lambda: torch_fit(days_dev, lags, splits, dev)))
        t['a'].append(host_ms(lambda: host_models(days, lags, splits)))
    med = {k: float(np.median(v)) for k, v in t.items()}
    fmt = lambda v: ' '.join('%.2f' % x for x in v)
    lines = ['var_probe: %s, d=%d, %d days x %d hours, %d models = lags 1..20 x %d splits (%d fitted / %d held-out days), ridge %g, '
             '%d alternating rounds, ms (medians; all rounds in brackets)' % (torch.cuda.get_device_name(0), D_TOPICS, DAYS, HD, K, REPS,
                                                                              DAYS - HELD, HELD, RIDGE, a.rounds),
             'call    one fit_population call, host clock, uploads and read-back included   %8.2f [%s]' % (med['call'], fmt(t['call'])),
             '        its device part alone (ops.var_fit_pop, three launches, events)        %8.2f [%s]' % (med['device'], fmt(t['device'])),
             '(a)     the %d models one after another on the host (lstsq, NumPy)             %8.2f [%s]' % (K, med['a'], fmt(t['a'])),
             '(b)     the FIT stage alone by torch (bmm, cholesky, cholesky_solve per lag)   %8.2f [%s]' % (med['b'], fmt(t['b'])),
             '        (a) / call = %.1f;  (b) covers the coefficients only, the call also forecasts and scores' % (med['a'] / med['call']),
             '        cross-validation error per model, call against (a): max |difference| %.2e (lstsq on the augmented system and '
             'Cholesky on the normal equations differ by conditioning)' % float(np.abs(fits.metrics[:, 6] - ref).max()),
             'backward error eta = ||G B - C||_F / (||G||_F ||B||_F + ||C||_F) of the call\'s coefficients, longdouble, and its bound 4 m (m + n) u:']
    fro = lambda x: np.sqrt(np.sum(x * x))
    for case in R.CASES:
        d, p, n_train = case
        cd, ctr, cte = R.case_days(case)
        m, n = 1 + p * d, n_train * HD - p
        for lam in R.RIDGES:
            f = V.fit_population(cd, [p], lam, ctr, cte)
            G, C = R.gram(R.series(cd, ctr), p, lam, np.longdouble)
            B = f.coef[0, :m].astype(np.longdouble)
            lines.append('        %-14s m=%-3d n=%-3d lambda=%-5g eta %.2e  bound %.2e' % (R.case_id(case), m, n, lam,
                                                                                        float(fro(G @ B - C) / (fro(G) * fro(B) + fro(C))),
                                                                                        4 * m * (m + n) * R.U))
    text = '\n'.join(lines)
    print(text)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
