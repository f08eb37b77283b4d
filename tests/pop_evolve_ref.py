"""NumPy restatement of ONE exploit / explore step of a population training call (mfg_pop_evolve_t, include/mfg_hip.h),
written from the header's definition: sort the active learners by the key (value not finite, value, k), and when enough of them
are active and the n_top-th value is finite, let each of the last n_bottom draw a donor among the first n_top with the project's
Philox block of counter (0xFFFFFFFE, s, k, 0), copy its parameters and perturb its learning rates.  TEST INFRASTRUCTURE: no
GPU, no library call; the Philox words come from oracle/philox_ref.py."""
import math

import numpy as np

from oracle.philox_ref import philox4x32_10

EVOLVE_DRAW_ELEM = 0xFFFFFFFE


def words(seed, s, k):
    """x0 .. x3 of learner k at step s: Python ints, or for an array of learners a list of such tuples."""
    seed = int(seed)
    x = philox4x32_10(EVOLVE_DRAW_ELEM, int(s), np.asarray(k, dtype=np.uint64), 0, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    if np.ndim(k) == 0:
        return tuple(int(v) for v in x)
    return [tuple(int(v) for v in row) for row in zip(*x)]


def order_of(values, active):
    """The active learners in ascending key order.  The key of the header: (value not finite, value, k), a non-finite value
    counting as +inf."""
    keys = []
    for k in range(len(values)):
        if active[k]:
            v = float(values[k])
            finite = math.isfinite(v)
            keys.append((not finite, v if finite else math.inf, k))
    return [k for _, _, k in sorted(keys)]


def clamp(x, lo, hi):
    return min(max(x, lo), hi)


def step(values, active, theta, w, lr_critic, lr_actor, *, s, seed, n_top, n_bottom, perturb=3, factors=(0.8, 1.25),
         lr_critic_bounds=(1e-6, 10.0), lr_actor_bounds=(1e-8, 1.0), extra=()):
    """One step.  values [K] (the check's column), active [K] bool, theta [K], w [K, F], lr_critic, lr_actor [K] (fp64).
    extra: further per-learner arrays (leading dimension K) a receiver takes over from its donor as it takes theta and w (the
    validation block's best_value, best_check, since_best, best_theta, best_w; theta_prev is theta itself).
    Returns a dict: rank [K] (-1: not active), order (list), parent [K] (-1: not active), replaced (bool), theta, w, lr_critic,
    lr_actor (new arrays), lr [K, 2] (the log row; NaN: not active), extra (list of new arrays)."""
    K = len(values)
    values = np.asarray(values, dtype=np.float64)
    active = np.asarray(active, dtype=bool)
    theta, w = np.array(theta, dtype=np.float64), np.array(w, dtype=np.float64)
    lrc, lra = np.array(lr_critic, dtype=np.float64), np.array(lr_actor, dtype=np.float64)
    extra = [np.array(x) for x in extra]
    order = order_of(values, active)
    A = len(order)
    rank = np.full(K, -1, dtype=np.int32)
    for r, k in enumerate(order):
        rank[k] = r
    parent = np.where(active, np.arange(K), -1).astype(np.int32)
    replaced = A >= n_top + n_bottom and math.isfinite(float(values[order[n_top - 1]]))
    if replaced:
        old = (theta.copy(), w.copy(), lrc.copy(), lra.copy(), [x.copy() for x in extra])      # donors are never receivers
        receivers = order[A - n_bottom:]
        for k, (x0, x1, x2, _) in zip(receivers, words(seed, s, receivers)):
            donor = order[(x0 * n_top) >> 32]
            assert rank[donor] < n_top <= A - n_bottom
            theta[k], w[k] = old[0][donor], old[1][donor]
            for x, o in zip(extra, old[4]):
                x[k] = o[donor]
            c, a = float(old[2][donor]), float(old[3][donor])
            if perturb & 1:
                c = clamp(c * (factors[1] if x1 >> 31 else factors[0]), *lr_critic_bounds)
            if perturb & 2:
                a = clamp(a * (factors[1] if x2 >> 31 else factors[0]), *lr_actor_bounds)
            lrc[k], lra[k] = c, a
            parent[k] = donor
    lr = np.full((K, 2), np.nan)
    lr[active, 0], lr[active, 1] = lrc[active], lra[active]
    return dict(rank=rank, order=order, parent=parent, replaced=bool(replaced), theta=theta, w=w, lr_critic=lrc, lr_actor=lra,
                lr=lr, extra=extra)
