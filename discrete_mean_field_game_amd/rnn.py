"""The RNN baseline of the paper's comparison, trained as ONE population on the device.

The reference holds this arm as text files only: process.py:4-22 writes the network's training file, read_rnn
(mfg_ac2.py:757-761, ac_irl.py:1657-1661) reads its predictions back for a figure, and plots.py:29-30 hard-codes its scores.  The
network itself is not in the reference, so the model is this project's definition (include/mfg_hip.h, mfg_rnn_fit_pop; DESIGN.md,
"The RNN baseline"): one LSTM layer and a softmax head, trained teacher forced on whole days by full-batch Adam or gradient
descent, selected on held-out days by the free-running forecast's JSD, forecast and scored as var.fit_population's
origin='rolling'.  Parity with whatever network produced the paper's 0.580 / 0.567 is unpinned.

fit_population() trains, selects, forecasts and scores K independent models -- each with its own hidden size, learning rate,
weight decay, clip, epochs and days -- in the two launches of one ops.rnn_fit_pop call per chunk; cross_validation() puts all
its len(hidden_range) x len(lr_range) x repetitions models into one such call, with the splits of var.var.splits.
"""
from __future__ import annotations

import numpy as np

from . import _lib as L
from .var import METRIC_NAMES, _day_lists, _per_model, _table  # noqa: F401  (the same day-list rules as the VAR population)


def unpack(w, H, d):
    """The packed weights of one model as a dict of views: Wx [4H, d], Wh [4H, H], b [4H], Wo [d, H], bo [d]; gate order i, f, g,
    o (torch.nn.LSTMCell's)."""
    w = np.asarray(w)
    G = 4 * H
    at = np.cumsum([0, G * d, G * H, G, d * H, d])
    return {'Wx': w[at[0]:at[1]].reshape(G, d), 'Wh': w[at[1]:at[2]].reshape(G, H), 'b': w[at[2]:at[3]],
            'Wo': w[at[3]:at[4]].reshape(d, H), 'bo': w[at[4]:at[5]]}


def init_weights(H, d, seed):
    """The packed initial weights of one model, W(H, d) values uniform in +-1/sqrt(H) from np.random.default_rng(seed) (the range
    of torch.nn.LSTM's default).  The device has no random number in this feature: the initial weights are an input."""
    from .ops import rnn_weight_count
    if H < 1 or d < 1:
        raise ValueError('init_weights: H=%r, d=%r' % (H, d))
    bound = 1.0 / np.sqrt(H)
    return np.random.default_rng(seed).uniform(-bound, bound, rnn_weight_count(H, d))


def check_population_args(days, hidden, lrs, epochs, train_days, val_days, test_days, wd, clip, optimizer, eval_every):
    """The argument rules of fit_population, without a GPU (ValueError).  Returns (days, hidden, lrs, epochs, wds, clips, train
    lists, validation lists, test lists, (K, D, Hd, d, W_max, E_max, C_max))."""
    from . import ops
    days = np.ascontiguousarray(days, dtype=np.float64)
    hidden = np.asarray(hidden, dtype=np.int64).reshape(-1)
    K = hidden.shape[0]
    if K < 1:
        raise ValueError('no models')
    if days.ndim != 3:
        raise ValueError('days: expected [D, Hd, d], got %s' % (days.shape,))
    lrs, wds, clips = (_per_model(n, v, K, np.float64) for n, v in (('lrs', lrs), ('wd', wd), ('clip', clip)))
    epochs = _per_model('epochs', epochs, K, np.int64)
    tr = _day_lists('train_days', train_days, K, days.shape[0], False)
    va = _day_lists('val_days', val_days, K, days.shape[0], True)
    te = _day_lists('test_days', test_days, K, days.shape[0], True)
    n_tr, n_va, n_te = ([t.size for t in lists] for lists in (tr, va, te))
    W_max = E_max = C_max = 0
    for c0 in range(0, K, L.POP_MAX_K):      # (per-model rules and the limit of one call; fit_population's chunks are never larger)
        s = slice(c0, c0 + L.POP_MAX_K)
        _, D, Hd, d, Wc, Ec, Cc = ops.check_rnn_fit_args(days.shape, hidden[s], epochs[s], lrs[s], wds[s], clips[s], n_tr[s], n_va[s],
                                                         n_te[s], optimizer, eval_every)
        W_max, E_max, C_max = max(W_max, Wc), max(E_max, Ec), max(C_max, Cc)
    return days, hidden, lrs, epochs, wds, clips, tr, va, te, (K, D, Hd, d, W_max, E_max, C_max)


def model_bytes(hidden, epochs, train_n, val_n, test_n, d, Hd, eval_every=1):
    """An upper bound of the device bytes one model of a fit_population chunk needs (hidden, epochs, train_n, val_n, test_n:
    arrays or lists of K values, laid out POP_MAX_K models at a time): the largest workspace slice
    (mfg_rnn_fit_workspace_bytes lays the slices out; needs the library, no GPU), its initial weights and its outputs."""
    from . import ops
    K = len(hidden)
    ones = np.ones(K)
    largest = 0
    for c0 in range(0, K, L.POP_MAX_K):      # (the layout of ONE call, which takes at most POP_MAX_K models)
        s = slice(c0, c0 + L.POP_MAX_K)
        table, total = ops.rnn_models(hidden[s], epochs[s], ones[s], 0 * ones[s], 0 * ones[s], train_n[s], val_n[s], test_n[s], d, Hd)
        offs = [table[k].ws_offset for k in range(len(table))] + [total]
        largest = max(largest, max(b - a for a, b in zip(offs, offs[1:])))
    W_max = max(ops.rnn_weight_count(int(H), d) for H in hidden)
    C_max = max(ops.rnn_check_count(int(E), int(nv), eval_every) for E, nv in zip(epochs, val_n))
    outputs = 8 * (W_max + int(max(epochs)) + C_max + int(max(test_n)) * (Hd * d + 4) + 8) + 8
    return largest + 8 * W_max + outputs


class RnnFits:
    """The result of fit_population (NumPy): weights [K, W_max] (the selected iterate, packed, zeros beyond W(H, d)), loss
    [K, E_max] (the training loss of each epoch at the weights before its update; NaN beyond the model's epochs), val [K, C_max]
    (the held-out JSD_mean of each check; NaN beyond the model's checks), best_epoch [K], future [K, Nt_max, Hd, d] (hour 0 the
    observed row), per_day [K, Nt_max, 4] (l1_final, l1_mean, JSD_final, JSD_mean per test day), metrics [K, 8] (mean, std over
    the test days of each: the columns of VarFits.metrics), status [K] (bit 0: non-finite input, bit 1: non-finite loss or
    gradient norm; a model with status != 0 is NaN everywhere)."""

    def __init__(self, out, hidden, lrs, epochs, wds, clips, n_val, n_test, hours, d, optimizer, eval_every):
        for name in ('weights', 'loss', 'val', 'best_epoch', 'future', 'per_day', 'metrics', 'status'):
            setattr(self, name, out[name])
        self.hidden, self.lrs, self.epochs, self.wds, self.clips, self.n_val, self.n_test = hidden, lrs, epochs, wds, clips, n_val, n_test
        self.hours, self.d, self.optimizer, self.eval_every = int(hours), int(d), optimizer, int(eval_every)

    def __len__(self):
        return int(self.status.shape[0])

    def model(self, k):
        """Model k alone: its unpacked weight matrices (Wx, Wh, b, Wo, bo) and its cropped outputs."""
        from .ops import rnn_check_count, rnn_weight_count
        H, d, N, E = int(self.hidden[k]), self.d, int(self.n_test[k]), int(self.epochs[k])
        out = {n: a.copy() for n, a in unpack(self.weights[k, :rnn_weight_count(H, d)], H, d).items()}
        out.update(hidden=H, lr=float(self.lrs[k]), wd=float(self.wds[k]), clip=float(self.clips[k]), epochs=E,
                   status=int(self.status[k]), best_epoch=int(self.best_epoch[k]), loss=self.loss[k, :E].copy(),
                   val=self.val[k, :rnn_check_count(E, int(self.n_val[k]), self.eval_every)].copy(), future=self.future[k, :N].copy(),
                   per_day=self.per_day[k, :N].copy(), metrics=self.metrics[k].copy())
        return out

    def traj(self, k):
        """Model k's forecast as [N, Hd, d] fp32 -- N test days, hour 0 the observed row --, the member layout of
        ops.forecast_score: with repeats = 1 that scorer takes traj(k)[None] unchanged, as it takes VarFits.traj(k)."""
        return self.future[k, :int(self.n_test[k])].astype(np.float32)


def fit_population(days, hidden, lrs, epochs, train_days, val_days=None, test_days=None, *, wd=0, clip=0, optimizer='adam',
                   eval_every=1, seed=0, w0=None, budget=None, device=None):
    """Train, select, forecast and score K RNN models on the device.  days [D, Hd, d]: a table of day matrices; hidden [K]: the
    hidden sizes; lrs, epochs, wd, clip: one value or [K]; train_days / val_days / test_days: one list of day indices for every
    model or K lists (val_days None: no selection, the last iterate is returned; test_days None: no forecast); optimizer 'adam'
    or 'sgd' and eval_every, one per call.  The initial weights of model k are init_weights(H_k, d, [seed, k]) unless w0 (a list
    of K packed vectors, or [K, >= W_max]) gives them.  NumPy in, an RnnFits out.  Models go in chunks whose workspaces and
    outputs stay within `budget` bytes (population.consistency_chunks; None: its default); chunking changes no bit.  Runs on a
    context of its own."""
    import torch
    from . import ops
    from .population import consistency_chunks
    days, hidden, lrs, epochs, wds, clips, tr, va, te, (K, D, Hd, d, W_max, E_max, C_max) = check_population_args(
        days, hidden, lrs, epochs, train_days, val_days, test_days, wd, clip, optimizer, eval_every)
    n_tr, n_va, n_te = (np.array([t.size for t in lists]) for lists in (tr, va, te))
    w_tab = np.zeros((K, W_max))
    for k in range(K):
        Wk = ops.rnn_weight_count(int(hidden[k]), d)
        wk = init_weights(int(hidden[k]), d, [int(seed), k]) if w0 is None else np.asarray(w0[k], dtype=np.float64).reshape(-1)[:Wk]
        if wk.shape[0] != Wk:
            raise ValueError('w0: model %d needs %d packed weights, got %d' % (k, Wk, wk.shape[0]))
        w_tab[k, :Wk] = wk
    chunks = consistency_chunks(K, model_bytes(hidden, epochs, n_tr, n_va, n_te, d, Hd, eval_every), budget)
    if not torch.cuda.is_available():
        raise L.MfgError('fit_population needs a ROCm GPU: the HIP hot path has no CPU fallback')
    dev = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
    tabs = [_table(lists, int(n.max())) for lists, n in ((tr, n_tr), (va, n_va), (te, n_te))]
    ctx = ops.Context(dev)
    prev = ctx.bind_scoped()
    try:
        with torch.cuda.device(dev):
            days_dev = torch.as_tensor(days, device=dev)
            parts = []
            for c0, n in chunks:
                s = slice(c0, c0 + n)
                idx = [torch.as_tensor(t[s].copy(), device=dev) if cnt.max() else None for t, cnt in zip(tabs, (n_tr, n_va, n_te))]
                res = ops.rnn_fit_pop(days_dev, torch.as_tensor(w_tab[s].copy(), device=dev), hidden[s], epochs[s], lrs[s], wds[s],
                                      clips[s], idx[0], n_tr[s], idx[1], n_va[s], idx[2], n_te[s], optimizer=optimizer,
                                      eval_every=eval_every, E_max=E_max, C_max=C_max)
                parts.append({name: t.cpu().numpy() for name, t in res.items()})
    finally:
        ctx.restore(prev)
        ctx.close()
    out = {name: np.concatenate([p[name] for p in parts]) for name in parts[0]}
    return RnnFits(out, hidden, lrs, epochs, wds, clips, n_va, n_te, Hd, d, optimizer, eval_every)


def cross_validation(days, hidden_range, lr_range, validation_size=5, repetitions=5, *, epochs=200, wd=0, clip=0, optimizer='adam',
                     eval_every=1, seed=0, split_seed=None, budget=None, device=None):
    """The RNN's counterpart of var.cross_validation (var.py:109-162): for every (hidden size, learning rate), `repetitions`
    random splits of the days into a fitted and a held-out part, scored by the mean JSD of the free-running forecast of the
    held-out days.  The splits are var.var.splits' draws in (H, lr, repetition) order (split_seed None: the global NumPy state;
    else RandomState(split_seed)); all len(hidden_range) x len(lr_range) x repetitions models run in ONE fit_population call, the
    held-out days as each model's test days (no selection: the last iterate is scored).  Returns a dict: 'hidden', 'lr' (the
    grids), 'mean' and 'std' [len(hidden_range), len(lr_range)] of the held-out JSD_mean over the repetitions, 'best' (H, lr) of
    the lowest mean, and 'fits' (the RnnFits, models in (H, lr, repetition) order)."""
    from .var import var as _var
    days = np.ascontiguousarray(days, dtype=np.float64)
    hidden_range, lr_range = [int(h) for h in hidden_range], [float(x) for x in lr_range]
    if days.ndim != 3:
        raise ValueError('days: expected [D, Hd, d], got %s' % (days.shape,))
    num_days = days.shape[0]
    if not 1 <= validation_size < num_days:
        raise ValueError('validation_size=%d of %d days' % (validation_size, num_days))
    if not hidden_range or not lr_range or repetitions < 1:
        raise ValueError('no hidden size, no learning rate or no repetition')
    cells = len(hidden_range) * len(lr_range)
    rng = None if split_seed is None else np.random.RandomState(split_seed)
    splits = _var.splits(num_days, validation_size, cells * repetitions, rng)
    hidden = np.repeat(hidden_range, len(lr_range) * repetitions)
    lrs = np.tile(np.repeat(lr_range, repetitions), len(hidden_range))
    fits = fit_population(days, hidden, lrs, epochs, [s for s, _ in splits], None, [r for _, r in splits], wd=wd, clip=clip,
                          optimizer=optimizer, eval_every=eval_every, seed=seed, budget=budget, device=device)
    score = fits.metrics[:, 6].reshape(len(hidden_range), len(lr_range), repetitions)
    mean, std = score.mean(axis=2), score.std(axis=2)
    i, j = np.unravel_index(int(np.nanargmin(mean)) if np.isfinite(mean).any() else 0, mean.shape)
    return {'hidden': hidden_range, 'lr': lr_range, 'mean': mean, 'std': std, 'best': (hidden_range[i], lr_range[j]), 'fits': fits}


def write_trajectories(fits, k, path):
    """Model k's forecast in the file layout read_rnn reads (mfg_ac2.py:757-761, ac_irl.py:1657-1661: pd.read_csv(path, sep=' ',
    header=None, ...)): one row per hour, the test days one after another, one column per topic, separated by single spaces."""
    rows = fits.future[k, :int(fits.n_test[k])].reshape(-1, fits.d)
    np.savetxt(path, rows, fmt='%.17g', delimiter=' ')
    return rows.shape[0]


def read_trajectories(path, hours=16):
    """A file in read_rnn's layout (one row per hour, one column per topic, space separated) as [N, hours, d] fp32 -- the dtype
    read_rnn asks for --, the member layout of ops.forecast_score."""
    rows = np.loadtxt(path, delimiter=' ', dtype=np.float32, ndmin=2)
    if rows.shape[0] % hours:
        raise ValueError('%s: %d rows are no whole number of days of %d hours' % (path, rows.shape[0], hours))
    return rows.reshape(-1, hours, rows.shape[1])
