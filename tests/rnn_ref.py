"""The RNN population call restated in NumPy from the definitions of include/mfg_hip.h (mfg_rnn_fit_pop): the yardstick of
tests/test_gpu_rnn_pop.py and test_rnn_host.py.  Forward pass, backward pass by hand, Adam / gradient descent, clipping, held-out
selection, forecast and scores.  Every function takes a dtype, so that it also runs in np.longdouble (the restatement's own
rounding error is measured as fp64 against longdouble, as in tests/var_ref.py).  Its gradient is pinned against torch.autograd and
its Adam against torch.optim.Adam in tests/test_rnn_host.py."""
import numpy as np

import var_ref as V

U = 2.0 ** -53
HD = 16

# (d, H, training days, Hd): below one 4-wide tile; short days; the workload's d; one day past 16 columns with 4H = 128; the
# largest H, where the weights leave the LDS
CASES = [(3, 4, 2, 16), (5, 8, 3, 5), (15, 16, 5, 16), (21, 32, 17, 16), (15, 64, 13, 16)]
N_VAL, N_TEST = 2, 3


def case_id(c):
    return 'd%d-H%d-n%d-Hd%d' % c


def weight_count(H, d):
    return 4 * H * (d + H + 1) + d * (H + 1)


def unpack(w, H, d):
    """Views of the packed weights: Wx [4H, d], Wh [4H, H], b [4H], Wo [d, H], bo [d]; gate order i, f, g, o."""
    G = 4 * H
    at = np.cumsum([0, G * d, G * H, G, d * H, d])
    return w[at[0]:at[1]].reshape(G, d), w[at[1]:at[2]].reshape(G, H), w[at[2]:at[3]], w[at[3]:at[4]].reshape(d, H), w[at[4]:at[5]]


def init_weights(H, d, seed, dtype=np.float64):
    return np.random.default_rng(seed).uniform(-1.0 / np.sqrt(H), 1.0 / np.sqrt(H), weight_count(H, d)).astype(dtype)


def dirichlet_days(D, Hd, d, seed):
    """[D, Hd, d] fp64: every row a Dirichlet(0.7) draw."""
    return np.random.RandomState(seed).dirichlet(0.7 * np.ones(d), size=(D, Hd))


def case_days(case, seed=None):
    """The day table of a case and its lists: (days [n_train + 5, Hd, d], train_idx, val_idx, test_idx)."""
    d, H, n, Hd = case
    days = dirichlet_days(n + N_VAL + N_TEST, Hd, d, 2000 + 7 * d + H if seed is None else seed)
    return days, list(range(n)), list(range(n, n + N_VAL)), list(range(n + N_VAL, n + N_VAL + N_TEST))


def sigmoid(x):
    return 1 / (1 + np.exp(-x))


def cell(w, H, d, x, h, c):
    """One LSTM step on a batch: x [N, d], h, c [N, H] -> (h', c', (i, f, g, o))."""
    Wx, Wh, b, _, _ = unpack(w, H, d)
    a = x @ Wx.T + h @ Wh.T + b
    i, f, g, o = sigmoid(a[:, :H]), sigmoid(a[:, H:2 * H]), np.tanh(a[:, 2 * H:3 * H]), sigmoid(a[:, 3 * H:])
    c2 = f * c + i * g
    return o * np.tanh(c2), c2, (i, f, g, o)


def log_softmax(z):
    mx = z.max(axis=-1, keepdims=True)
    return z - (mx + np.log(np.exp(z - mx).sum(axis=-1, keepdims=True)))


def softmax(z):
    e = np.exp(z - z.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)


def loss_and_grad(w, H, d, Y, wd=0.0, dtype=np.float64):
    """(L, dL/dw) of the teacher-forced loss on the days Y [N, Hd, d], the weight-decay term wd/2 ||w||^2 included:
    L = 1/(N (Hd-1)) sum_n sum_t -sum_j y[n,t+1,j] log yhat[n,t,j] + wd/2 ||w||^2.  The backward pass is written out by hand."""
    w, Y = np.asarray(w, dtype=dtype), np.asarray(Y, dtype=dtype)
    N, Hd, _ = Y.shape
    T = Hd - 1
    Wx, Wh, b, Wo, bo = unpack(w, H, d)
    h, c = np.zeros((N, H), dtype=dtype), np.zeros((N, H), dtype=dtype)
    saved = []
    loss = dtype(0)
    dz = []
    for t in range(T):
        c_prev, h_prev = c, h
        h, c, gates = cell(w, H, d, Y[:, t], h, c)
        z = h @ Wo.T + bo
        lp = log_softmax(z)
        y = Y[:, t + 1]
        loss = loss + (-(y * lp).sum())
        dz.append((np.exp(lp) * y.sum(axis=1, keepdims=True) - y) / dtype(N * T))
        saved.append((gates, c, c_prev, h, h_prev))
    loss = loss / dtype(N * T) + dtype(0.5) * dtype(wd) * (w * w).sum()
    g = np.zeros_like(w)
    gWx, gWh, gb, gWo, gbo = unpack(g, H, d)
    dh_next, dc_next = np.zeros((N, H), dtype=dtype), np.zeros((N, H), dtype=dtype)
    for t in range(T - 1, -1, -1):
        (i, f, gg, o), c, c_prev, h, h_prev = saved[t]
        gWo += dz[t].T @ h
        gbo += dz[t].sum(axis=0)
        dh = dz[t] @ Wo + dh_next
        tc = np.tanh(c)
        dc = dh * o * (1 - tc * tc) + dc_next
        da = np.concatenate([dc * gg * i * (1 - i), dc * c_prev * f * (1 - f), dc * i * (1 - gg * gg), dh * tc * o * (1 - o)], axis=1)
        gWx += da.T @ Y[:, t]
        gWh += da.T @ h_prev
        gb += da.sum(axis=0)
        dh_next, dc_next = da @ Wh, dc * f
    g += dtype(wd) * w
    return loss, g


def forecast(w, H, d, Y):
    """[N, Hd, d]: every day of Y from its observed hour 0 with zero state, the model's own output fed back for Hd - 1 hours."""
    w, Y = np.asarray(w), np.asarray(Y, dtype=np.asarray(w).dtype)
    N, Hd, _ = Y.shape
    _, _, _, Wo, bo = unpack(w, H, d)
    out = np.empty_like(Y)
    out[:, 0] = Y[:, 0]
    h, c = np.zeros((N, H), dtype=w.dtype), np.zeros((N, H), dtype=w.dtype)
    for t in range(Hd - 1):
        h, c, _ = cell(w, H, d, out[:, t], h, c)
        out[:, t + 1] = softmax(h @ Wo.T + bo)
    return out


def metrics(future, Y, dtype=np.float64):
    """(per_day [N, 4], metrics [8]) of a forecast [N, Hd, d] against the days Y: tests/var_ref.py's, origin 'rolling'."""
    N, Hd, d = np.asarray(Y).shape
    return V.metrics(np.asarray(future).reshape(N * Hd, d), np.asarray(Y).reshape(N * Hd, d), Hd, dtype)


def train(w0, H, d, Y, epochs, lr, wd=0.0, clip=0.0, optimizer='adam', Yval=None, eval_every=1, dtype=np.float64):
    """The epochs of mfg_rnn_fit_pop for one model: full-batch Adam (torch's form) or gradient descent, optional clipping of the
    global gradient norm, held-out selection.  Returns a dict: weights (the selected iterate), last (the last iterate), loss
    [epochs], val [checks], best_epoch, grads (the clipped-before gradient of every epoch)."""
    w = np.array(w0, dtype=dtype)
    m, v = np.zeros_like(w), np.zeros_like(w)
    b1, b2 = dtype(0.9), dtype(0.999)
    b1t = b2t = dtype(1)
    losses, vals, grads = [], [], []
    best, best_val, best_epoch = None, np.inf, 0
    for ep in range(1, epochs + 1):
        loss, g = loss_and_grad(w, H, d, Y, wd, dtype)
        losses.append(loss)
        grads.append(g.copy())
        gn = np.sqrt((g * g).sum())
        if clip > 0 and gn > clip:
            g = g * (dtype(clip) / gn)
        b1t, b2t = b1t * b1, b2t * b2
        if optimizer == 'adam':
            m = b1 * m + (1 - b1) * g
            v = b2 * v + (1 - b2) * (g * g)
            w = w - dtype(lr) / (1 - b1t) * (m / (np.sqrt(v) / np.sqrt(1 - b2t) + dtype(1e-8)))
        else:
            w = w - dtype(lr) * g
        if Yval is not None and len(Yval) and (ep % eval_every == 0 or ep == epochs):
            vm = metrics(forecast(w, H, d, np.asarray(Yval, dtype=dtype)), Yval, dtype)[0][:, 3].mean()
            vals.append(vm)
            if vm < best_val:
                best, best_val, best_epoch = w.copy(), vm, ep
    chosen = best if best is not None else w
    return {'weights': chosen, 'last': w, 'loss': np.array(losses, dtype=dtype), 'val': np.array(vals, dtype=dtype),
            'best_epoch': best_epoch if best is not None else epochs, 'grads': grads}


def model(days, train_idx, val_idx, test_idx, H, w0, epochs, lr, wd=0.0, clip=0.0, optimizer='adam', eval_every=1,
          dtype=np.float64):
    """Everything mfg_rnn_fit_pop returns for one model, as a dict."""
    days = np.asarray(days)
    d = days.shape[2]
    out = train(w0, H, d, days[list(train_idx)], epochs, lr, wd, clip, optimizer, days[list(val_idx)] if len(val_idx) else None,
                eval_every, dtype)
    if len(test_idx):
        out['future'] = forecast(out['weights'], H, d, days[list(test_idx)].astype(dtype))
        out['per_day'], out['metrics'] = metrics(out['future'], days[list(test_idx)], dtype)
    return out


def bound(x64, xld, magnitude=None):
    """The tolerance of a GPU comparison: 64 x the restatement's own fp64-against-longdouble gap (the maximum over elements) plus
    a floor of 16 u x the largest magnitude in the case."""
    x64, xld = np.asarray(x64, dtype=np.longdouble), np.asarray(xld, dtype=np.longdouble)
    gap = float(np.max(np.abs(x64 - xld))) if x64.size else 0.0
    mag = float(np.max(np.abs(xld))) if magnitude is None and xld.size else float(magnitude or 0.0)
    return 64 * gap + 16 * U * mag
