"""Reference for the policy-gradient score of the fused rollout kernels.  TEST INFRASTRUCTURE ONLY (see mfg_oracle.py).

    g = sum_ij (psi(A_i) - psi(alpha_ij) + ln P_ij) alpha'_ij,     A_i = sum_j alpha_ij,
    alpha_ij = softplus(z_ij),  alpha'_ij = x_ij sigmoid(z_ij),  z_ij = theta x_ij,  x_ij = pi_j - pi_i - shift.

Three things live here:

* ``terms``      a stable fp64 restatement (the reference's ``log(1 + exp z)`` loses alpha below z ~ -36 and overflows above
                 709; this one is checked against mpmath in tests/test_score_ref.py),
* ``magnitude``  M, the sum of the magnitudes of the terms the mixed kernels add up: M / |g| is the conditioning of a case,
* ``bound``      a per-trajectory bound on |g_kernel - g| assembled from the error budgets the kernels' own sources state.
                 Nothing in it is fitted to what a kernel returns; every constant cites where it is stated.

and the table of parameter regimes (``REGIMES``, ``regime_case``) shared by the GPU test modules.
"""
from __future__ import annotations

import math

import numpy as np
from scipy import special

ZERO_P_REPLACEMENT = 1e-100        # mfg_ac2.py:369
LOG_ZERO_P = math.log(ZERO_P_REPLACEMENT)

U32 = 2.0 ** -24                   # fp32 unit roundoff: one correctly rounded fp32 operation
ULP32 = 2.0 ** -23                 # "1 ulp" of the hardware transcendentals v_log_f32 / v_exp_f32 / v_rcp_f32 (mfg_device.h:325)
EPS64 = 2.0 ** -52                 # per fp64 operation
FLT_MIN_NORMAL = 2.0 ** -126
SAFETY = 2.0                       # the ONE overall safety factor of bound()

LOG1P_REL = 1.95e-7                # softplus_sigmoid_e: "max relative error 1.95e-7" (mfg_device.h:391)
EXP_FACTOR_REL = 1.0e-7            # exp_f64arg, E_j and F_i: "~1e-7 relative" (mfg_device.h:341)
HTAB_FIT = 1.0e-8                  # h table: "|error| < 1e-8 + fp32 rounding" (mfg_device.h:473)
HTAB_ZMIN, HTAB_PER_UNIT, HTAB_N = -24.0, 16, 1792          # mfg_device.h:478-481
LOG2_ABS = 2.0 ** -22              # v_log_f32 near 1: absolute, in log2 units -- measured (oracle/sampler_ref.py:25, :30-33)
FAST_LOG_ABS = 4.0e-8              # fast_log_f64: "absolute error ~4e-8" (mfg_device.h:401)
DIGAMMA_MIXED_ABS = 1.0e-9         # digamma_pos_mixed: "|error| < 1e-9 + the fast log's 4e-8" (mfg_device.h:416)
DIGAMMA_F64_REL = 2.0e-15          # digamma_pos (DESIGN.md "Numerics")
WAVE = 64


# ---------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------
def terms(pi, P, theta, shift):
    """fp64 pieces of the score for states pi [..., d] and actions P [..., d, d].

    Returns a dict: g [...], the per-element x, z, alpha, sg (sigmoid), ad (alpha'), h (= psi(alpha) sigmoid(z), so that
    psi(alpha) alpha' = x h), lnP, and the per-row A, D (= sum_j alpha'), psiA.  Zeros of P count as 1e-100 (mfg_ac2.py:369).
    """
    pi = np.asarray(pi, dtype=np.float64)
    P = np.asarray(P, dtype=np.float64)
    x = pi[..., None, :] - pi[..., :, None] - shift
    z = theta * x
    alpha = np.logaddexp(0.0, z)
    sg = special.expit(z)
    ad = x * sg
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        h = special.digamma(alpha) * sg
    # alpha -> 0: psi(alpha) = -1/alpha - euler + O(alpha) and sigmoid / alpha -> 1, so h -> -1 (mfg_device.h:470)
    h = np.where(alpha < 1e-290, -1.0, h)
    with np.errstate(divide='ignore'):
        lnP = np.where(P == 0.0, LOG_ZERO_P, np.log(np.where(P == 0.0, 1.0, P)))
    A = alpha.sum(-1)
    D = ad.sum(-1)
    psiA = special.digamma(A)
    g = np.sum(lnP * ad - x * h, axis=(-2, -1)) + np.sum(psiA * D, axis=-1)
    return dict(g=g, x=x, z=z, alpha=alpha, sg=sg, ad=ad, h=h, lnP=lnP, A=A, D=D, psiA=psiA)


def _ln_y_S(t, scale):
    """(|ln y_ij|, |ln S_i|) as the sampling kernels see them.  The gamma variates y and their row sums S are not outputs
    of a launch: S_i ~ scale A_i (the mean of a sum of gamma variates with those shapes) and ln y_ij ~ ln P_ij + ln(scale
    A_i).  This only SIZES the magnitude sum and the bound -- it is not compared with anything.  scale=None: the given-P
    kernels, which read ln P itself and have no S."""
    if scale is None:
        return np.abs(t['lnP']), np.zeros_like(t['A'])
    lnS = np.log(np.maximum(scale * t['A'], 1e-300))
    return np.abs(t['lnP'] + lnS[..., None]), np.abs(lnS)


def magnitude(pi, P, theta, shift, scale=None, t=None):
    """M = sum_ij (|ln y_ij| + |psi(alpha_ij)|) |alpha'_ij| + sum_i (|psi(A_i)| + |ln S_i|) |D_i|: what the mixed kernels add
    up to form g (sum_ij log2(y_ij) alpha'_ij - x h, - ln S_i D_i, + psi(A_i) D_i).  See _ln_y_S for y and S."""
    t = t or terms(pi, P, theta, shift)
    L, lnS = _ln_y_S(t, scale)
    return (np.sum(L * np.abs(t['ad']) + np.abs(t['x'] * t['h']), axis=(-2, -1))
            + np.sum((np.abs(t['psiA']) + lnS) * np.abs(t['D']), axis=-1))


# ---------------------------------------------------------------------------------------------------
# the bound
# ---------------------------------------------------------------------------------------------------
def _fp32_depth(d, sampling):
    """(rows, score): the longest chains of fp32 additions behind a row's A_i / D_i and behind the score terms before they
    are folded into an fp64 sum; a chain of n additions loses at most n 2^-24 of the magnitude sum.
      given P: none -- policy_accumulate (mfg_core.h:232) adds every element to the fp64 sums.
      d <= 64 (k_core_small, k_core_row3): the quad -- three additions (sample_elems, mfg_core.h:420-428), then fp64.
      d > 64 (k_core_large, mfg_core.h:1440-1470, :1516, :1544): a lane adds its R = ceil(d / 64) elements of a row in fp32
        (R/2 + 1 levels), the 64 lanes are summed by a 6-level fp32 butterfly (row_batch_finish3); the score terms of a
        batch of up to 8 rows (large_row_batch) are added per lane in fp32 (4 more levels) before the fp64 fold."""
    if not sampling:
        return 0, 0
    if d <= WAVE:
        return 3, 3
    R = -(-d // WAVE)
    lane = (R + 1) // 2 + 1
    return lane + 6, lane + 1 + 4


def bound(pi, P, theta, shift, scale=None, precision='mixed', sampled=False, t=None, path=None):
    """Per-trajectory bound on |g_kernel - g| for precision 'mixed' / 'f64'.

    sampled=True: g_kernel comes from a SAMPLING launch (separable exponential, quads, ln y - ln S) and g is the oracle on
    that launch's own stored fp32 P; scale is the launch's alpha_scale.  sampled=False: the given-P kernels (ops.score,
    ops.td_pg_accumulate) on the same P the oracle reads.  path ('sampling' / 'given') names the kernel's data path on its own
    where a caller wants the oracle-reading term of `sampled` separately; by default it follows `sampled`.  Every line is first order in the budgets named at the top of this
    file; the sum is multiplied by SAFETY = 2 once (second-order terms, and budgets that their sources state with '~')."""
    t = t or terms(pi, P, theta, shift)
    pi = np.asarray(pi, dtype=np.float64)
    d = pi.shape[-1]
    sampling = (path or ('sampling' if sampled else 'given')) == 'sampling'
    if sampling and scale is None:
        raise ValueError('the sampling path needs alpha_scale')
    x, z, al, sg, ad, h = t['x'], t['z'], t['alpha'], t['sg'], t['ad'], t['h']
    A, D, psiA = t['A'], t['D'], t['psiA']
    aad, ax, ah = np.abs(ad), np.abs(x), np.abs(h)
    xh = ax * ah
    L, lnS = _ln_y_S(t, scale if sampling else None)
    pi_i = pi[..., :, None]
    dpsiA = special.polygamma(1, A)
    sh = abs(shift)
    if precision == 'f64':
        # policy_setup strict branch (mfg_core.h:208-212): x from two fp64 subtractions, z = theta x, exp, log1p, e / (1 + e)
        dx = EPS64 * (np.abs(x + shift) + ax)
        e_rel = abs(theta) * dx + EPS64 * (np.abs(z) + 1.0)
        d_ad = sg * dx + aad * (e_rel + 3 * EPS64)
        d_al = al * 2 * EPS64 + sg * e_rel
        with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
            psi = np.where(al < 1e-290, 0.0, special.digamma(al))
            dpsi_dal = np.where(al < 1e-290, 0.0, special.polygamma(1, al) * d_al)
        # -psi(alpha) alpha' = -x h: digamma_pos 2e-15 relative (absolute near its root), its argument's error, the product
        elem = (L * d_ad + aad * L * 2 * EPS64                               # ln v (fp64 log), times alpha'
                + ah * dx + ax * sg * (DIGAMMA_F64_REL * np.maximum(1.0, np.abs(psi)) + dpsi_dal) + np.abs(psi) * d_ad
                + 2 * EPS64 * (L * aad + xh))
        n_sum = 2 * d                                                       # fp64 chains: a row, then the rows
        dA = n_sum * EPS64 * A + d_al.sum(-1)
        dD = n_sum * EPS64 * aad.sum(-1) + d_ad.sum(-1)
        row = (np.abs(D) * (DIGAMMA_F64_REL * np.maximum(1.0, np.abs(psiA)) + 2 * EPS64 * lnS)
               + dpsiA * dA * np.abs(D) + (np.abs(psiA) + lnS) * dD)
        tot = elem.sum((-2, -1)) + row.sum(-1) + n_sum * EPS64 * magnitude(pi, P, theta, shift, scale if sampling else None, t)
    elif precision == 'mixed':
        if sampling:
            # policy_setup_sep (mfg_core.h:219): x = fl(pi_j - fl(pi_i + fl32(shift))); e = fl(E_j F_i), both factors from
            # fp64 arguments (exp_f64arg), so e does not see the rounding of x
            dx = U32 * (sh + np.abs(pi_i + shift) + ax)
            e_rel = 2 * EXP_FACTOR_REL + U32
        else:
            # policy_setup, FAST (mfg_core.h:200-206; theta_times_x, softplus_sigmoid_fast): x = fl(fl(pi_j - pi_i) - fl32(shift));
            # z = zh + zl carries the product's rounding, but is formed from the ROUNDED x; fast_exp rounds zh log2(e) (u |z|
            # relative in e), v_exp_f32 1 ulp, the fma of the tail, the rounding of theta's and shift's tails
            dx = U32 * (np.abs(x + shift) + sh + ax)
            e_rel = abs(theta) * dx + U32 * np.abs(z) + ULP32 + 3 * U32
        # sigmoid = e * rcp(fl(1 + e)); alpha' = fl(x * sigmoid)  (softplus_sigmoid_e, mfg_device.h:392-395)
        d_ad = sg * dx + aad * (e_rel + U32 + ULP32 + U32 + U32)
        d_al = LOG1P_REL * al + sg * e_rel
        # h table (htab_eval, mfg_device.h:484): the fitted cubic, its fp32 coefficients and three FMAs (the constant term
        # carries |h|, the others less than the interval's rise: |dh/dz| < 1 over 1/16), and the interval coordinate
        # t = fma(x, 16 fl32(theta), 384): one rounding of t, the rounding of theta, and the rounding of x, each mapped to z
        # (divide by 16) and through |dh/dz| < 1 (mfg_core.h:205)
        tt = np.clip(z * HTAB_PER_UNIT - HTAB_ZMIN * HTAB_PER_UNIT, 0.0, HTAB_N)
        d_h = HTAB_FIT + 2 * U32 * ah + U32 / 4 + U32 * tt / HTAB_PER_UNIT + abs(theta) * dx + U32 * np.abs(z)
        n_rows, n_g = _fp32_depth(d, sampling)
        elem = (L * d_ad                                                     # alpha' in log2(y) alpha'
                + aad * np.maximum(L * ULP32, math.log(2.0) * LOG2_ABS)      # v_log_f32: 1 ulp, absolute near 1 (P == 0: a rounded constant)
                + ah * dx + ax * d_h + U32 * xh                              # psi_ad = fl(x * h)
                + U32 * (L * aad + xh)                                       # gt = fma(log2 y, alpha', -psi_ad): one rounding
                + n_g * U32 * (L * aad + xh))                                # fp32 sums of gt
        dA = n_rows * U32 * A + d_al.sum(-1)
        dD = n_rows * U32 * aad.sum(-1) + d_ad.sum(-1)
        # per row (mfg_core.h:846-873): - fast_log_f64(S) D (sampling only), + digamma_pos_mixed(A) D -- the series' 1e-9, its
        # own fast_log_f64, and below A = 4 the recurrence term q'/q in fp64 (two Newton steps, ~8 operations) relative to psi
        row = (np.abs(D) * ((FAST_LOG_ABS if sampling else 0.0) + DIGAMMA_MIXED_ABS + FAST_LOG_ABS + 8 * EPS64 * np.abs(psiA))
               + dpsiA * dA * np.abs(D) + (np.abs(psiA) + lnS) * dD)
        tot = (elem.sum((-2, -1)) + row.sum(-1)
               + 2 * d * EPS64 * magnitude(pi, P, theta, shift, scale if sampling else None, t))   # the fp64 folds
    else:
        raise ValueError(precision)
    if sampled:
        # the oracle reads ln P from the stored fp32 P where the kernel read ln y - ln S: P within 1.5 ulp of fl32(y / S)
        # (DESIGN.md Numerics (e)) -- as long as P is a normal fp32 number.  Below 2^-126 the stored value is rounded to a
        # multiple of 2^-149 (|ln| off by at most 2 * 2^-150 / P), and a stored 0 reads as 1e-100 here while the kernel held
        # ln y - ln S with y >= 2^-126 (v_exp_f32 flushes below; oracle/sampler_ref.py:29, :45): off by at most
        # |ln 1e-100 - ln 2^-126| + |ln S| = 143 + |ln S|.
        Pf = np.asarray(P, dtype=np.float64)
        sub = (Pf > 0) & (Pf < FLT_MIN_NORMAL)
        lost = np.where(sub, 2 * 2.0 ** -150 / np.where(sub, Pf, 1.0), 0.0)
        lost = np.where(Pf == 0, abs(LOG_ZERO_P - math.log(FLT_MIN_NORMAL)) + lnS[..., None], lost)
        tot = tot + np.sum((2 * ULP32 + lost) * aad, axis=(-2, -1))
    return SAFETY * tot


# ---------------------------------------------------------------------------------------------------
# parameter regimes
# ---------------------------------------------------------------------------------------------------
STRADDLE_TARGETS = [1.0, 2.0 / 3.0, 1.0 / 3.0]
X0 = float(np.log(np.e - 1.0))     # softplus(X0) = 1


def regime_case(regime, B, d, rs, k=0, jitter=1e-6):
    """(pi [B, d] fp32, theta, shift, scale) of a shape regime of the sampler tests."""
    if regime == 'policy':           # the reference policy (mfg_ac2.py:832): shapes 1e3 .. 1e5
        return rs.dirichlet(np.ones(d), size=B).astype(np.float32), 8.86349, 0.16, 12000.0
    if regime == 'mid':              # shapes ~1 .. 100
        pi = rs.uniform(0.0, 0.8, size=(B, d)).astype(np.float32)
        return pi, 4.0, 0.0, 30.0
    if regime == 'small':            # every shape below 1, down to ~0.02 (the boost and its underflow)
        pi = rs.uniform(0.2, 0.8, size=(B, d)).astype(np.float32)
        return pi, 4.0, 0.3, 0.65
    # straddle: half the state entries ~1e-6, half X0 + jitter: x = pi_j - pi_i lands on +X0, -X0 and ~0, so with theta = 1,
    # shift = 0 the shapes are target * {1, softplus(-X0), ln 2} (softplus(X0) = 1).  f64 (fp64 alpha, one fp32 rounding):
    # jitter 1e-6, a dense band around the target that resolves the rounding of fl32(alpha * scale) at 1;  mixed (alpha to
    # ~2e-7): jitter 0.1, so that the classification's near ties stay rare
    tgt = STRADDLE_TARGETS[(k // 4) % len(STRADDLE_TARGETS)]
    lo = rs.uniform(0.0, 2e-6, size=(B, d))
    hi = X0 + rs.uniform(-jitter, jitter, size=(B, d))
    pi = np.where(rs.rand(B, d) < 0.5, lo, hi).astype(np.float32)
    return pi, 1.0, 0.0, tgt


def _dirichlet(conc):
    def states(rs, B, d):
        pi = rs.dirichlet(np.full(d, conc), size=B)
        return (pi / pi.sum(-1, keepdims=True)).astype(np.float32)
    return states


def _sampler(regime):
    def states(rs, B, d):
        return regime_case(regime, B, d, rs)[0]
    return states


def _peaked(rs, B, d):
    """A third one-hot rows, a third Dirichlet(0.05), a third Dirichlet(1) with half the entries exactly 0 (renormalised)."""
    pi = np.zeros((B, d))
    for b in range(B):
        kind = b % 3
        if kind == 0:
            pi[b, rs.randint(d)] = 1.0
        elif kind == 1:
            pi[b] = rs.dirichlet(np.full(d, 0.05))
        else:
            v = rs.dirichlet(np.ones(d))
            v[rs.permutation(d)[:d // 2]] = 0.0
            pi[b] = v / v.sum()
    return pi.astype(np.float32)


def _one_dominant(rs, B, d):
    """One entry >= 0.95, a few small ones, the rest exactly 0: pi_j - pi_i comes within 0.05 of 1."""
    pi = np.zeros((B, d))
    for b in range(B):
        top = rs.uniform(0.95, 1.0)
        idx = rs.permutation(d)
        n = max(1, min(3, d - 1))
        pi[b, idx[1:1 + n]] = (1.0 - top) * rs.dirichlet(np.ones(n))
        pi[b, idx[0]] = top
    return pi.astype(np.float32)


def _point(theta, shift, scale, states, **extra):
    return dict(theta=float(theta), shift=float(shift), scale=float(scale), states=states, extra=extra)


# |theta| (1 + |shift|) <= 86 is the mixed sampling kernels' range (mfg_device.h report_sep_range): every point below whose
# 'mixed_in_range' is not False lies inside it.  theta = 120 at shift 0.16 is outside; f64 has no limit.
REGIMES = {
    'mfg_ac2': [_point(8.86349, 0.16, 12000, _dirichlet(1.0))],                                   # the control
    'ac_irl': [_point(8.64, 0.0, 1e4, _dirichlet(1.0), discount_pow=True)],
    'synthetic': [_point(2.6, 0.0, 1e4, _dirichlet(1.0), reward_kind=1),
                  _point(10.0, 0.0, 100.0, _dirichlet(1.0), reward_kind=1)],                        # the class default
    'mid': [_point(4.0, 0.0, 30.0, _sampler('mid'))],
    'small': [_point(4.0, 0.3, 0.65, _sampler('small'))],
    'peaked': [_point(8.86349, 0.16, 12000, _peaked)],
    'steep': [_point(40.0, 0.16, 12000, _dirichlet(1.0)),
              _point(74.0, 0.16, 12000, _dirichlet(0.3)),                                          # 74 * 1.16 = 85.84: just inside
              _point(74.0, 0.16, 12000, _one_dominant),
              _point(-8.86349, 0.16, 12000, _dirichlet(1.0)),
              _point(120.0, 0.16, 12000, _dirichlet(0.3), mixed_in_range=False),
              _point(120.0, 0.16, 12000, _one_dominant, mixed_in_range=False)],
    'flat': [_point(0.0, 0.16, 12000, _dirichlet(1.0)), _point(1e-3, 0.16, 12000, _dirichlet(1.0))],
    'shifted': [_point(8.86349, -0.3, 12000, _dirichlet(1.0)), _point(8.86349, 0.5, 12000, _dirichlet(1.0))],
}


def regime_points():
    """[(name, point)]: every point of every regime, named 'regime' or 'regime.k'."""
    out = []
    for name, pts in REGIMES.items():
        for k, p in enumerate(pts):
            out.append((name if len(pts) == 1 else '%s.%d' % (name, k), p))
    return out
