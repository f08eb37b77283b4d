#!/usr/bin/env python3
"""GPU: the RNN cross-validation as one population call, against doing without it.  The shape is the VAR section's
cross-validation shape: d = 15, 18 days of 16 hours, 5 random splits into 13 fitted and 5 held-out days, here for each of
H in {8, 16, 32, 64} x 5 learning rates -- 100 models, 200 Adam epochs each, then forecast over the held-out days and scored.
  call   one rnn.fit_population call (uploads, two launches, read-back), host clock around it; and the device part alone,
         ops.rnn_fit_pop on resident buffers, event-timed
  (a)    the same models one after another through torch.nn.LSTM + torch.nn.Linear + torch.optim.Adam in fp64 on the same
         device (training only: 200 full-batch epochs; no forecast, no scores)
  (b)    the same on the host CPU
         (a) and (b) run --baseline-models models per round, one per hidden size first (default 4: H = 8, 16, 32, 64 at the first
         learning rate and split), and are scaled to the 100; the per-model times are printed so that the scaling can be checked
Both sides warmed up, alternating rounds, medians.  Then the worst error-to-bound ratio of the cases of tests/rnn_ref.py
(the comparisons of tests/test_gpu_rnn_pop.py).  Kernel table: rocprofv3 --kernel-trace --stats -- python tools/rnn_probe.py
--kernels-only.
python tools/rnn_probe.py [--rounds 5] [--baseline-models 4] [--out profiles/rnn_pop.txt] [--kernels-only]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from discrete_mean_field_game_amd import ops, rnn, var as V  # noqa: E402
import rnn_ref as R  # noqa: E402

D_TOPICS, HD, DAYS, HELD, REPS, EPOCHS = 15, 16, 18, 5, 5, 200
HIDDEN, LRS = [8, 16, 32, 64], [3e-3, 1e-2, 3e-2, 1e-3, 1e-1]


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


def torch_model(days_t, H, lr, sel, w0, dev):
    """One model through torch.nn.LSTM + Linear + Adam, fp64, the whole training set one batch; returns the last loss."""
    d = days_t.shape[2]
    lstm, head = torch.nn.LSTM(d, H, batch_first=True).double().to(dev), torch.nn.Linear(H, d).double().to(dev)
    p = rnn.unpack(w0, H, d)
    with torch.no_grad():
        lstm.weight_ih_l0.copy_(torch.as_tensor(p['Wx'])), lstm.weight_hh_l0.copy_(torch.as_tensor(p['Wh']))
        lstm.bias_ih_l0.copy_(torch.as_tensor(p['b'])), lstm.bias_hh_l0.zero_()
        head.weight.copy_(torch.as_tensor(p['Wo'])), head.bias.copy_(torch.as_tensor(p['bo']))
    lstm.bias_hh_l0.requires_grad_(False)                  # (one gate bias, as in the call)
    opt = torch.optim.Adam([q for q in list(lstm.parameters()) + list(head.parameters()) if q.requires_grad], lr=lr)
    Y = days_t[torch.as_tensor(np.asarray(sel), device=dev)]
    loss = None
    for _ in range(EPOCHS):
        opt.zero_grad()
        out, _ = lstm(Y[:, :-1])
        loss = -(Y[:, 1:] * torch.log_softmax(head(out), dim=2)).sum(dim=2).mean()
        loss.backward()
        opt.step()
    return float(loss.detach())


def case_ratios():
    """Per case of tests/rnn_ref.py, the worst error / bound of the comparisons of tests/test_gpu_rnn_pop.py (plain variant)."""
    lines = []
    for case in R.CASES:
        d, H, n, Hd = case
        days, tr, va, te = R.case_days(case)
        w0 = R.init_weights(H, d, 12)
        a, b = (R.model(days, tr, va, te, H, w0, 8, 1e-2, dtype=t) for t in (np.float64, np.longdouble))
        f = rnn.fit_population(days, [H], 1e-2, 8, tr, va, te, w0=[w0])
        s = rnn.fit_population(days, [H], 1.0, 1, tr, None, None, optimizer='sgd', w0=[w0])
        ratio = {}
        for what, dev, r64, rld in (('weights', f.weights[0], a['weights'], b['weights']), ('loss', f.loss[0], a['loss'], b['loss']),
                                    ('val', f.val[0], a['val'], b['val'])):
            ratio[what] = float(np.abs(dev - r64).max()) / R.bound(r64, rld)
        g64, gld = a['grads'][0], b['grads'][0]
        ratio['gradient'] = float(np.abs((w0 - s.weights[0]) - g64).max()) / R.bound(g64, gld, max(np.abs(g64).max(), np.abs(w0).max()))
        w = f.weights[0]
        f64, fld = R.forecast(w, H, d, days[te]), R.forecast(w.astype(np.longdouble), H, d, days[te])
        ratio['future'] = float(np.abs(f.future[0] - f64).max()) / R.bound(f64, fld)
        lines.append('        %-20s ' % R.case_id(case) + '  '.join('%s %.3f' % kv for kv in sorted(ratio.items()))
                     + '   (weights bound %.2e, best_epoch %d = %d)' % (R.bound(a['weights'], b['weights']), f.best_epoch[0], a['best_epoch']))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--baseline-models', type=int, default=4)
    ap.add_argument('--out', default=None)
    ap.add_argument('--kernels-only', action='store_true', help='three device calls and nothing else: the run to put under rocprofv3')
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    days = R.dirichlet_days(DAYS, HD, D_TOPICS, 2024)
    hidden = np.repeat(HIDDEN, len(LRS) * REPS)
    lrs = np.tile(np.repeat(LRS, REPS), len(HIDDEN))
    K = len(hidden)
    splits = V.var.splits(DAYS, HELD, K, np.random.RandomState(0))
    sel, rest = [s for s, _ in splits], [r for _, r in splits]
    w0 = [rnn.init_weights(int(H), D_TOPICS, [0, k]) for k, H in enumerate(hidden)]
    # the device part alone, on resident buffers
    days_dev = torch.as_tensor(days, device=dev)
    ntr, nva, nte = [DAYS - HELD] * K, [0] * K, [HELD] * K
    cols = (hidden, [EPOCHS] * K, lrs, [0.0] * K, [0.0] * K)
    table, nbytes = ops.rnn_models(*cols, ntr, nva, nte, D_TOPICS, HD)
    models = (table, ops.rnn_models_device(table, dev), nbytes)
    W_max = ops.rnn_weight_count(max(HIDDEN), D_TOPICS)
    w_tab = np.zeros((K, W_max))
    for k, w in enumerate(w0):
        w_tab[k, :w.size] = w
    w_dev = torch.as_tensor(w_tab, device=dev)
    tr = torch.as_tensor(np.stack(sel).astype(np.int32), device=dev)
    te = torch.as_tensor(np.array(rest, dtype=np.int32), device=dev)
    bufs = {n: torch.empty(s, dtype=t, device=dev) for n, (s, t) in ops.rnn_fit_shapes(K, HD, D_TOPICS, W_max, EPOCHS, 0, HELD).items()}
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
    device_call = lambda: ops.rnn_fit_pop(days_dev, w_dev, *cols, tr, ntr, None, nva, te, nte, out=bufs, workspace=ws, models=models)
    for _ in range(3):
        device_call()
    torch.cuda.synchronize()
    if a.kernels_only:
        return
    whole_call = lambda: rnn.fit_population(days, hidden, lrs, EPOCHS, sel, None, rest, w0=w0)
    fits = whole_call()
    # the baselines' models: one per hidden size first
    step = len(LRS) * REPS
    ids = ([q * step for q in range(len(HIDDEN))] + [k for k in range(K) if k % step])[:a.baseline_models]
    days_cpu = torch.as_tensor(days)
    base = lambda t, device: [torch_model(t, int(hidden[k]), float(lrs[k]), sel[k], w0[k], device) for k in ids]
    last = base(days_dev, dev)
    base(days_cpu, torch.device('cpu'))
    t = {'call': [], 'device': [], 'a': [], 'b': []}
    for _ in range(a.rounds):
        t['call'].append(host_ms(whole_call))
        t['device'].append(event_ms(device_call))
        t['a'].append(host_ms(lambda: base(days_dev, dev)))
        t['b'].append(host_ms(lambda: base(days_cpu, torch.device('cpu'))))
    per_H = [[host_ms(lambda: torch_model(t_, int(H), LRS[0], sel[0], rnn.init_weights(int(H), D_TOPICS, 0), dv)) for H in HIDDEN]
             for t_, dv in ((days_dev, dev), (days_cpu, torch.device('cpu')))]
    med = {k: float(np.median(v)) for k, v in t.items()}
    scale = K / len(ids)
    fmt = lambda v: ' '.join('%.2f' % x for x in v)
    lines = ['rnn_probe: %s, d=%d, %d days x %d hours, %d models = H %s x %d learning rates x %d splits (%d fitted / %d held-out days), '
             '%d Adam epochs, %d alternating rounds, ms (medians; all rounds in brackets)'
             % (torch.cuda.get_device_name(0), D_TOPICS, DAYS, HD, K, HIDDEN, len(LRS), REPS, DAYS - HELD, HELD, EPOCHS, a.rounds),
             'call    one fit_population call, host clock, uploads and read-back included   %9.2f [%s]' % (med['call'], fmt(t['call'])),
             '        its device part alone (ops.rnn_fit_pop, two launches, events)          %9.2f [%s]' % (med['device'], fmt(t['device'])),
             '(a)     %d of the models through torch LSTM + Adam, fp64, same device          %9.2f [%s]   x %.0f = %.0f for the %d'
             % (len(ids), med['a'], fmt(t['a']), scale, med['a'] * scale, K),
             '(b)     the same on the host CPU                                               %9.2f [%s]   x %.0f = %.0f for the %d'
             % (med['b'], fmt(t['b']), scale, med['b'] * scale, K),
             '        one model of H = %s alone, ms: device %s; CPU %s' % (HIDDEN, fmt(per_H[0]), fmt(per_H[1])),
             '        (a) / call = %.0f, (b) / call = %.0f (scaled); the baselines train only, the call also forecasts and scores'
             % (med['a'] * scale / med['call'], med['b'] * scale / med['call']),
             '        last training loss of the baseline models, call against (a): max |difference| %.2e'
             % float(np.abs(np.array([fits.loss[k, -1] for k in ids]) - np.array(last)).max()),
             '        status of the %d models: %d ok; held-out JSD_mean %.4f .. %.4f' % (K, int((fits.status == 0).sum()),
                                                                                         float(np.nanmin(fits.metrics[:, 6])), float(np.nanmax(fits.metrics[:, 6]))),
             'worst error / bound per case (8 Adam epochs at lr 1e-2, one gradient-descent epoch; bound = 64 x the restatement\'s '
             'fp64-against-longdouble gap + 16 u x the largest magnitude):'] + case_ratios()
    text = '\n'.join(lines)
    print(text)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
