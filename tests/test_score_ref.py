"""oracle/score_ref.py checked on the CPU: the restatement against 40-digit arithmetic and against the reference's own form,
and its error bound against a float32 emulation of the mixed kernels' documented data path -- the bound has to hold for
correctly rounded fp32 arithmetic before any GPU is held to it.  `-s` prints, per regime, M / |g| and the worst emulated
err / bound (the CPU columns of the table in DESIGN.md "Numerics")."""
import numpy as np
import pytest

from oracle import mfg_oracle as O
from oracle import score_ref as S

f32 = np.float32
LN2 = 0.6931471805599453
POINTS = S.regime_points()
IN_RANGE = [(n, p) for n, p in POINTS if p['extra'].get('mixed_in_range', True)]


def _h64(z):
    al = np.logaddexp(0.0, z)
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        from scipy import special
        h = special.digamma(al) * special.expit(z)
    return np.where(al < 1e-290, -1.0, h)


def _quad_sum(a):
    """[..., d] float32 -> fp64 sums over the last axis: quads of four added in fp32 in order, the quads folded in fp64."""
    d = a.shape[-1]
    pad = (-d) % 4
    if pad:
        a = np.concatenate([a, np.zeros(a.shape[:-1] + (pad,), f32)], -1)
    q = a.reshape(a.shape[:-1] + (-1, 4))
    s = ((q[..., 0] + q[..., 1]) + q[..., 2]) + q[..., 3]
    assert s.dtype == f32
    return s.astype(np.float64).sum(-1)


def emulate_mixed(pi32, theta, shift, scale, rs, drop_lnS=False):
    """The mixed sampling kernels' data path (mfg_core.h policy_setup_sep / policy_terms, the per-row epilogue) in NumPy
    float32 with correctly rounded operations; gamma variates from numpy.  Returns (g [B], P [B, d, d] float32)."""
    from scipy import special
    pi64 = pi32.astype(np.float64)
    sh = f32(shift)
    pas = (pi32 + sh).astype(f32)
    x = (pi32[:, None, :] - pas[:, :, None]).astype(f32)
    E = np.exp(theta * (pi64 - 0.5)).astype(f32)
    F = np.exp(-theta * (pi64 + (shift - 0.5))).astype(f32)
    e = (E[:, None, :] * F[:, :, None]).astype(f32)
    u = (f32(1) + e).astype(f32)
    r = (f32(1) / u).astype(f32)
    sg = (e * r).astype(f32)
    lnu = np.log(u.astype(np.float64)).astype(f32)
    al = ((e - (u - f32(1))).astype(f32).astype(np.float64) * r.astype(np.float64) + lnu.astype(np.float64)).astype(f32)   # fma
    ad = (x * sg).astype(f32)
    y = rs.gamma(np.maximum(al.astype(np.float64) * scale, 1e-300)).astype(f32)
    y[y == 0] = f32(1e-20)
    lnv = np.log2(y.astype(np.float64)).astype(f32)
    h = (_h64(np.float64(f32(theta)) * x.astype(np.float64)) / LN2).astype(f32)
    psi_ad = (x * h).astype(f32)
    gt = (lnv.astype(np.float64) * ad.astype(np.float64) - psi_ad.astype(np.float64)).astype(f32)                         # fma
    A, D, Ssum, G = _quad_sum(al), _quad_sum(ad), _quad_sum(y), _quad_sum(gt)
    g = G * LN2
    if not drop_lnS:
        g = g - np.log(Ssum) * D
    g = g + special.digamma(A) * D
    inv32 = (1.0 / Ssum).astype(f32)
    P = (y * inv32[..., None]).astype(f32)
    return g.sum(-1), P


def _case(name, p, d, B, seed=0):
    rs = np.random.RandomState(seed + 7919 * d + sum(map(ord, name)))
    pi32 = p['states'](rs, B, d)
    return rs, pi32


@pytest.mark.parametrize('d', [3, 21])
@pytest.mark.parametrize('name,p', POINTS, ids=[n for n, _ in POINTS])
def test_terms_against_mpmath(name, p, d):
    mp = pytest.importorskip('mpmath')
    mp.mp.dps = 40
    B = 2
    rs, pi32 = _case(name, p, d, B)
    theta, shift = p['theta'], p['shift']
    al = np.logaddexp(0.0, theta * (pi32.astype(np.float64)[:, None, :] - pi32.astype(np.float64)[:, :, None] - shift))
    y = rs.gamma(np.maximum(al * p['scale'], 1e-300))
    y[y == 0] = 1e-20
    P = (y / y.sum(-1, keepdims=True)).astype(f32)
    P[0, 0, d - 1] = 0.0                                            # the zero rule
    t = S.terms(pi32, P, theta, shift)
    bd = S.bound(pi32, P, theta, shift, precision='f64', sampled=False, t=t)
    th, shf = mp.mpf(theta), mp.mpf(shift)
    for b in range(B):
        g = mp.mpf(0)
        for i in range(d):
            row = []
            for j in range(d):
                xx = mp.mpf(float(pi32[b, j])) - mp.mpf(float(pi32[b, i])) - shf
                zz = th * xx
                row.append((mp.log1p(mp.exp(zz)), xx / (1 + mp.exp(-zz))))
            psiA = mp.digamma(sum(a for a, _ in row))
            for j, (a, adv) in enumerate(row):
                lp = mp.log(mp.mpf('1e-100')) if P[b, i, j] == 0 else mp.log(mp.mpf(float(P[b, i, j])))
                g += (psiA - mp.digamma(a) + lp) * adv
        err = abs(float(mp.mpf(float(t['g'][b])) - g))
        assert np.isfinite(bd[b]) and err <= bd[b], (name, d, b, err, bd[b], float(g))


def test_terms_against_the_reference_form_at_the_control_point():
    p = S.REGIMES['mfg_ac2'][0]
    for d in (3, 21, 128):
        rs, pi32 = _case('mfg_ac2', p, d, 4)
        _, P = emulate_mixed(pi32, p['theta'], p['shift'], p['scale'], rs)
        g = S.terms(pi32, P, p['theta'], p['shift'])['g']
        g_ref = O.calc_gradient(P, pi32, p['theta'], p['shift'])
        assert np.max(np.abs(g - g_ref) / np.abs(g_ref)) < 1e-12


@pytest.mark.parametrize('name,p', IN_RANGE, ids=[n for n, _ in IN_RANGE])
def test_fp32_emulation_stays_below_the_bound(name, p):
    worst, cond = 0.0, []
    for d in (15, 21, 128, 256):
        B = 6 if d <= 21 else 3
        rs, pi32 = _case(name, p, d, B, seed=1)
        g_em, P = emulate_mixed(pi32, p['theta'], p['shift'], p['scale'], rs)
        t = S.terms(pi32, P, p['theta'], p['shift'])
        bd = S.bound(pi32, P, p['theta'], p['shift'], p['scale'], 'mixed', sampled=True, t=t)
        M = S.magnitude(pi32, P, p['theta'], p['shift'], p['scale'], t=t)
        err = np.abs(g_em - t['g'])
        assert np.all(np.isfinite(bd)) and np.all(np.isfinite(g_em))
        worst = max(worst, float(np.max(err / bd)))
        cond.append(float(np.median(M / np.abs(t['g']))))
        assert np.all(err <= bd), (name, d, err, bd)
    print('[score_ref] %-12s emulated err/bound %.3g   M/|g| at d = 15 / 21 / 128 / 256: %s' % (
        name, worst, ' / '.join('%.3g' % c for c in cond)))


@pytest.mark.parametrize('name,p', POINTS, ids=[n for n, _ in POINTS])
def test_bound_is_finite_and_monotone(name, p):
    for d in (4, 21, 100):
        rs, pi32 = _case(name, p, d, 3, seed=2)
        al = np.logaddexp(0.0, p['theta'] * (pi32.astype(np.float64)[:, None, :] - pi32.astype(np.float64)[:, :, None] - p['shift']))
        y = rs.gamma(np.maximum(al * p['scale'], 1e-300)).astype(f32)
        y[y == 0] = f32(1e-20)                                     # shapes that underflow to the replacement
        P = (y / y.sum(-1, keepdims=True)).astype(f32)
        t = S.terms(pi32, P, p['theta'], p['shift'])
        b = {}
        for prec in ('f64', 'mixed'):
            for sampled in (False, True):
                b[prec, sampled] = S.bound(pi32, P, p['theta'], p['shift'], p['scale'], prec, sampled=sampled, path='sampling', t=t)
                assert np.all(np.isfinite(b[prec, sampled])) and np.all(b[prec, sampled] > 0)
            assert np.all(b[prec, True] >= b[prec, False])
            given = S.bound(pi32, P, p['theta'], p['shift'], None, prec, sampled=False, t=t)
            assert np.all(np.isfinite(given)) and np.all(given > 0)
        for sampled in (False, True):
            assert np.all(b['mixed', sampled] >= b['f64', sampled])
        assert np.all(S.bound(pi32, P, p['theta'], p['shift'], None, 'mixed', t=t) >= S.bound(pi32, P, p['theta'], p['shift'], None, 'f64', t=t))


def test_small_regime_reaches_the_replacement():
    """The `small` regime does produce variates that underflow (stored P subnormal or zero): the bound's terms for them are
    exercised, not dead."""
    p = S.REGIMES['small'][0]
    rs, pi32 = _case('small', p, 21, 64, seed=3)
    _, P = emulate_mixed(pi32, p['theta'], p['shift'], p['scale'], rs)
    assert np.any(P < S.FLT_MIN_NORMAL)
