"""The DEFINITION of mfg_moves_loglik_pop (include/mfg_hip.h) restated in NumPy and math: a plain helper of
tests/test_moves_loglik_host.py and tests/test_gpu_moves_loglik.py, not a conftest.

T(a, m) = sum_{t<m} ln(a + t) and D(a, m) = sum_{t<m} 1 / (a + t) are the finite sums themselves, added by math.fsum (exactly
rounded), so nothing here subtracts two ln Gamma or two digamma values.  The softplus and the sigmoid are those of the oracle's
policy_logpdf (np.log1p(np.exp(z)), e / (1 + e)).  Next to every value stands its condition sum, the scale against which the
device is held (the value itself may cancel):
  S = sum of |ln(a + t)| over every term of every T of the transition, plus |lgamma(n_i + 1)| and the |lgamma(m_j + 1)|
  G = sum over the rows of sum_j |da_j/dp| D(a_j, m_j) + |dA/dp| D(A, n_i), per parameter p
"""
import math

import numpy as np

BAD_DATA, ZERO_ALPHA, BAD_POLICY, BAD_SET = 1, 2, 4, 8
BOUND = 1e-10           # the project's bound for mfg_policy_logpdf (tests/test_gpu_launch_once_kernels.py), on S and G


def log_terms(a, m):
    """ln(a + t), t < m, as an array (empty for m = 0; -inf first for a = 0)."""
    with np.errstate(divide='ignore'):
        return np.log(a + np.arange(int(m), dtype=np.float64))


def T(a, m):
    """(T(a, m), sum of |terms|): T(a, 0) = 0 exactly, T(0, m > 0) = -inf."""
    if m == 0:
        return 0.0, 0.0
    terms = log_terms(a, m)
    if a == 0.0:
        return -math.inf, math.inf
    return math.fsum(terms), math.fsum(np.abs(terms))


def D(a, m):
    """D(a, m) = sum_{t<m} 1 / (a + t); D(a, 0) = 0; D(0, m > 0) = inf."""
    if m == 0:
        return 0.0
    if a == 0.0:
        return math.inf
    return math.fsum(1.0 / (a + np.arange(int(m), dtype=np.float64)))


def alphas(pi, theta, shift, alpha_scale):
    """(a, da/dtheta, da/dshift) [d, d] of one state row, cell (i, j) from x = pi_j - pi_i - shift, every operation in fp64 in
    the order of the header."""
    pi = np.asarray(pi, dtype=np.float32).astype(np.float64)
    x = pi[None, :] - pi[:, None] - shift
    with np.errstate(over='ignore', invalid='ignore'):
        e = np.exp(theta * x)
        a = alpha_scale * np.log1p(e)
        sg = e / (1.0 + e)
        return a, alpha_scale * sg * x, -(alpha_scale * sg * theta)


def transition(pi, moves, theta, shift, alpha_scale):
    """One transition under one policy: pi [d] fp32, moves [d, d] integers (the corner).  Returns (ll, grad [3], S, G [3], flag)."""
    d = len(pi)
    m = np.asarray(moves, dtype=np.int64)
    nan3 = np.full(3, np.nan)
    if (m < 0).any() or not np.isfinite(np.asarray(pi, dtype=np.float64)).all():
        return math.nan, nan3, math.nan, nan3, BAD_DATA
    a, ath, ash = alphas(pi, theta, shift, alpha_scale)
    if ((a == 0.0) & (m > 0)).any():
        return -math.inf, nan3, math.inf, nan3, ZERO_ALPHA
    pieces, cond = [], []
    grad, G = [[], [], []], [[], [], []]
    for i in range(d):
        n_i = int(m[i].sum())
        if n_i == 0:
            continue
        A = 0.0
        for j in range(d):                                  # column order
            A += a[i, j]
        pieces.append(math.lgamma(n_i + 1.0))
        pieces += [-math.lgamma(mj + 1.0) for mj in m[i]]
        cond += [abs(p) for p in pieces[-(d + 1):]]
        for j in range(d):
            if m[i, j] > 0:
                terms = log_terms(a[i, j], m[i, j])
                pieces.append(math.fsum(terms)), cond.append(math.fsum(np.abs(terms)))
        terms = log_terms(A, n_i)
        pieces.append(-math.fsum(terms)), cond.append(math.fsum(np.abs(terms)))
        Dj = np.array([D(a[i, j], m[i, j]) for j in range(d)])
        DA = D(A, n_i)
        for p, da in enumerate((ath[i], ash[i], a[i])):
            dA = math.fsum(da)
            grad[p] += list(Dj * da) + [-DA * dA]
            G[p] += list(Dj * np.abs(da)) + [DA * abs(dA)]
    return (math.fsum(pieces), np.array([math.fsum(g) for g in grad]), math.fsum(cond), np.array([math.fsum(g) for g in G]), 0)


def loglik(state, moves, theta, shift, alpha_scale, d):
    """One policy on one data set: state [N, H, >= d] fp32, moves [N, H-1, width, width] integers.  Returns a dict of ll, S
    [N, H-1], grad, G [N, H-1, 3], flags [N, H-1], and ll_day [N], grad_day [N, 3], status [N] (the sequential sums)."""
    state, moves = np.asarray(state), np.asarray(moves)
    N, H = state.shape[:2]
    out = dict(ll=np.zeros((N, H - 1)), S=np.zeros((N, H - 1)), grad=np.zeros((N, H - 1, 3)), G=np.zeros((N, H - 1, 3)),
               flags=np.zeros((N, H - 1), np.int32))
    ok = np.isfinite([theta, shift, alpha_scale]).all() and alpha_scale > 0
    for n in range(N):
        for h in range(H - 1):
            if ok:
                r = transition(state[n, h, :d], moves[n, h, :d, :d], theta, shift, alpha_scale)
            else:
                r = (math.nan, np.full(3, np.nan), math.nan, np.full(3, np.nan), BAD_POLICY)
            out['ll'][n, h], out['grad'][n, h], out['S'][n, h], out['G'][n, h], out['flags'][n, h] = r
    out.update(day_sums(out['ll'], out['grad'], out['flags']))
    return out


def day_sums(ll, grad, flags):
    """ll_day, grad_day, status from per-transition arrays [..., H-1(, 3)]: h = 0 .. H - 2 in order, every addition rounded on
    its own."""
    ll_day, grad_day = np.zeros(ll.shape[:-1]), np.zeros(grad.shape[:-2] + (3,))
    status = np.zeros(flags.shape[:-1], np.int32)
    with np.errstate(invalid='ignore'):
        for h in range(ll.shape[-1]):
            ll_day = ll_day + ll[..., h]
            grad_day = grad_day + grad[..., h, :]
            status |= flags[..., h]
    return dict(ll_day=ll_day, grad_day=grad_day, status=status)


def adam_step(p, g, m, v, t, lr, mask, beta1=0.9, beta2=0.999, eps=1e-8):
    """The ascent step of likelihood.fit, restated in NumPy fp64: p, g, m, v [K, 3], t the 1-based step, mask [3] of 0 / 1 (the
    free parameters).  Returns (p, m, v)."""
    g = g * mask
    m = beta1 * m + (1.0 - beta1) * g
    v = beta2 * v + (1.0 - beta2) * (g * g)
    mhat = m / (1.0 - beta1 ** t)
    vhat = v / (1.0 - beta2 ** t)
    return p + lr * mhat / (np.sqrt(vhat) + eps), m, v
