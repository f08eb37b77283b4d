"""NumPy restatement of the in-kernel Dirichlet sampler, element by element (mfg_ac2.py:236-254 drawn from Philox).

TEST INFRASTRUCTURE, beside philox_ref.py (which pins the Philox words).  Written from docs/KERNELS.md "Sampler keying" and
DESIGN section 4 "Sampler", not from the kernel sources.  It returns, for every matrix element, the variate the kernels must
draw together with the discrete story of the draw (which path, which block was accepted), a relative error bound on the
value and a mask of the near-tie decisions where an fp32 kernel may legitimately decide the other way.

Contract (tests/test_gpu_sampler_elementwise.py and the anchored replays):
  * EXACT: keying (which Philox block feeds which element, in which slot), the bit fields, the accept / reject story (path,
    accepted block) and the even-step carry of a row's single trailing element.
  * BOUNDED: the value, |y_dev - y_ref| <= bound * y_ref, and the normalised row likewise (compare).
  * NEAR TIES: decisions whose outcome changes when the inputs move by their fp32 error (below) are flagged `ambiguous`;
    the tests cap how many there may be.

Arithmetic
  * Integer and bit-field work is exact (u01, 20-bit radius uniforms, 16-bit angles, k0..k3).
  * IEEE-exact fp32 steps of the kernel are emulated with np.float32: the acceptance uniform u = fl32(kf + u01) 2^-KB and
    the squeeze threshold fl32(fma(fl32(q q), slope, top)).
  * Transcendentals are fp64 (the kernels use v_log_f32, v_exp_f32, v_sqrt_f32, v_rsq_f32, v_rcp_f32 and v_sin_f32 /
    v_cos_f32, the last two taking revolutions).
  * Marsaglia-Tsang (d = a - 1/3, c = 1/sqrt(9 d)) is evaluated in fp64 on the same normal and the same u.

Error budgets of the hardware transcendentals -- ASSUMED, not measured on gfx950 (the GPU tests print the observed
max(err / bound) of every case so that the head-room is visible):  U = 2^-24 is the fp32 unit round-off.
  v_log_f32            relative 2 U   (EPS_LOG), and absolute 2^-22 in log2 (EPS_LOG_ABS): MEASURED -- see below
  v_exp_f32            relative 2 U   (EPS_EXP)
  v_sqrt_f32, v_rsq_f32, v_rcp_f32     relative 2 U   (EPS_ROOT)
  v_sin_f32, v_cos_f32 absolute 2^-20 in the value, input in revolutions   (EPS_TRIG)
  v_exp_f32 flushes a denormal result to zero: the boost underflows (-> 1e-20) when log2(U) / a < -126.
EPS_LOG_ABS is the one budget that was widened after a GPU run, for a named operation and a recorded reason: the first
element-wise run failed its bound only on boosted elements whose redraw had a radius uniform within 1e-5 of 1 (radius ~0.004:
log2 u ~ -1.4e-5), with x off by ~1e-3 relative -- v_log_f32 of an argument near 1 is accurate to ~2^-24.8 ABSOLUTE, not to a
few ulp of its tiny result.  The absolute term covers that with a factor 4.
From these:
  * the normal x = sqrt(-2 ln u) cos(2 pi phi): |dx| <= |x| EPS_X + r EPS_TRIG + ln 2 EPS_LOG_ABS / r,
    EPS_X = EPS_LOG / 2 + EPS_ROOT + 3 U;
  * c: EPS_C = EPS_ROOT + 4 U relative (plus the shape's error); d = a - 1/3 rounded: 2 U + da / d;
  * hot / exact value y = d (1 + c x)^3: eps_y = eps_d + 3 |dt| / |1 + t| + 6 U, dt = |t| (EPS_C + EPS_X) + c r EPS_TRIG;
  * boosted value y = (a + 2/3) v U^(1/a): + (|ln U| / a) (EPS_LOG + EPS_ROOT + 2 U + da / a) + ln 2 EPS_LOG_ABS / a
    + EPS_EXP + 2 U -- the U^(1/a) amplifies the error of the log by 1 / a;
  * mixed precision forms alpha in fp32 from separable exponentials: DESIGN section 4 (a), (b) put it at ~2e-7 relative;
    the shape error used here is MIXED_ALPHA_REL = 5 x 2e-7 relative plus 2 U absolute (the fp32 d = fma(alpha, scale, -1/3)
    and a = d + 1/3);  f64 forms alpha in fp64 and rounds the shape once: a = fl32(alpha scale), F64_ALPHA_REL = 1e-15.
  * normalisation: eps_P_i = eps_y_i + sum_j P_j eps_y_j + (log2 d + 8) U, plus an absolute 2^-148 / S on y for boosted
    variates that land in the fp32 denormal range and 2^-149 on P itself (its fp32 storage below 2^-126).

Near ties (`ambiguous`) -- by perturbation, not guesswork: every discrete decision is re-evaluated at
x +- dx, c (1 +- DELTA_C), a (1 +- da) and u at its two fp32 neighbours; the element is ambiguous when the decision's margin
is not larger than the sum of the margin's changes (a linearised "some combination flips it").  Decisions: MT accept /
reject (block 1 and every redraw), t > -1, small versus not small, and the boost underflow.  DELTA_C = 16 U stands for the
kernel's fp32 evaluation of the MT exponent, whose x^2 / 2 + d (ln v - v + 1) cancels to ~x^2 t^2 / 12: the kernel's c and d
agree only to a few U, which moves the exponent by ~x^2 DELTA_C.  The hot path's "sure" decision is NOT a near tie: when the
squeeze is sound (tests/test_sampler_ref.py::test_squeeze_is_sound) a sure element is accepted by the full test as well.
"""
import numpy as np

from oracle.philox_ref import philox_elem

U32 = 2.0 ** -24
EPS_LOG = 2 * U32
EPS_LOG_ABS = 2.0 ** -22
LN2 = np.log(2.0)
EPS_EXP = 2 * U32
EPS_ROOT = 2 * U32
EPS_TRIG = 2.0 ** -20
EPS_X = EPS_LOG / 2 + EPS_ROOT + 3 * U32
EPS_C = EPS_ROOT + 4 * U32
DELTA_C = 16 * U32
MIXED_ALPHA_REL = 5 * 2e-7
F64_ALPHA_REL = 1e-15
EXP2_MIN = -126.0                  # v_exp_f32 flushes 2^z, z < -126, to zero
ZERO_GAMMA_REPLACEMENT = np.float32(1e-20)   # mfg_ac2.py:244
MAX_BLOCK = 63                     # continuation blocks 1 .. 63
BOOST_BLOCK = 0xFFFF
K_BM = np.sqrt(2 * np.log(2.0))    # the hot path keeps normals in units of K

# Squeeze of the hot path: u < 1 - x^2 (SLOPE t^2 + SQUEEZE_ABS) implies MT acceptance for |t| <= 1/2,
# SLOPE > 1/6.  As a test on the KB-bit integer k of the uniform ((k + 1) 2^-KB is the top of its cell):
#   k <= TOP_KB - SLOPE 2^KB (x t)^2,  TOP_KB = 2^KB - 1 - 2^KB SQUEEZE_ABS 5.89^2 rounded down (5.89: the largest radius of
#   24-bit uniforms, kept as a margin for the 20-bit ones), evaluated in fp32 with x in units of K: (x t)^2 = 2 ln 2 (xs t)^2.
SQUEEZE_SLOPE = 0.19
SQUEEZE_ABS = 1e-6
SQUEEZE_TOP = {16: np.float32(65532.7), 12: np.float32(4094.85)}
SQUEEZE_LN2X2 = np.float32(1.3862944)

PATH_HOT, PATH_EXACT, PATH_BOOST = 0, 1, 2
PATH_NAMES = ('hot', 'exact', 'boost')

RADIUS_BITS = 20
ANGLE_BITS = 16


def quad_kbits(slot):
    """Width of the acceptance integer of a quad slot: 16 bits for slots 0, 1, 12 bits for slots 2, 3."""
    return np.where(np.asarray(slot) < 2, 16, 12)


def squeeze_consts(kb):
    slope = np.float32(np.float32(-SQUEEZE_SLOPE * 2.0 ** kb) * SQUEEZE_LN2X2)
    return slope, SQUEEZE_TOP[kb]


# ------------------------------------------------------------------------------------------------------------------
# Keying (docs/KERNELS.md "Sampler keying")
# ------------------------------------------------------------------------------------------------------------------
def keying(d, layout='auto'):
    """Per element (i, j) of a d x d matrix: key[i, j] = element id of the quad's block 0 counter, slot[i, j] in 0..3 and
    tail[i, j] = the element is a row's single trailing element (its pair is keyed by the even step).
    layout: 'small' / 'tail1' (d <= 64: packed and row3 kernels), 'large' (k_core_large<R>), 'auto' (small iff d <= 64)."""
    if layout == 'auto':
        layout = 'small' if d <= 64 else 'large'
    i = np.arange(d)[:, None] * np.ones((1, d), dtype=np.int64)
    j = np.ones((d, 1), dtype=np.int64) * np.arange(d)[None, :]
    tail = np.zeros((d, d), dtype=bool)
    if layout in ('small', 'tail1'):
        if layout == 'tail1':
            assert d % 4 == 1, 'tail1 layout: d = 1 mod 4'
        dq = d & ~3
        c0 = np.where(j < dq, (j // 4) * 4, dq)
        slot = j - c0
        key = i * d + c0
        if d - dq == 1:
            tail[:, dq] = True
    elif layout == 'large':
        R = -(-d // 64)
        lane, m = j % 64, j // 64
        if R % 4 == 0:
            m0 = (m // 4) * 4
            key = i * d + lane + 64 * m0
            slot = m - m0
        else:
            i0 = (i // 2) * 2
            m0 = (m // 2) * 2
            pair = m0 + 1 < R
            key = i0 * d + lane + 64 * m0
            slot = np.where(pair, 2 * (i - i0) + (m - m0), i - i0)
    else:
        raise ValueError(layout)
    return key.astype(np.uint64), slot.astype(np.int64), tail


# ------------------------------------------------------------------------------------------------------------------
# Bit fields
# ------------------------------------------------------------------------------------------------------------------
def u01(r):
    """(0, 1] from the top 24 bits: (k + 1/2) 2^-24 (exact in fp32)."""
    return ((np.asarray(r, np.uint32) >> np.uint32(8)).astype(np.float64) + 0.5) * 2.0 ** -24


def quad_fields(words, slot):
    """Fields of block 0 for an element in `slot`: radius uniform (20 bits of r.x / r.y), angle (16 bits: high / low half of
    r.z), acceptance integer k0 = r.w >> 16, k1 = r.w & 0xFFFF, k2 = r.x & 0xFFF, k3 = r.y & 0xFFF, cos for even slots, sin
    for odd ones."""
    x, y, z, w = (np.asarray(a, np.uint32) for a in words)
    slot = np.asarray(slot)
    h = slot >> 1
    radw = np.where(h == 0, x, y)
    radu = ((radw >> np.uint32(32 - RADIUS_BITS)).astype(np.float64) + 0.5) * 2.0 ** -RADIUS_BITS
    angw = np.where(h == 0, z >> np.uint32(16), z & np.uint32(0xFFFF))
    ang = (angw.astype(np.float64) + 0.5) * 2.0 ** -ANGLE_BITS
    k = np.select([slot == 0, slot == 1, slot == 2], [w >> np.uint32(16), w & np.uint32(0xFFFF), x & np.uint32(0xFFF)],
                  y & np.uint32(0xFFF))
    use_sin = (slot & 1) == 1
    return radu, ang, k.astype(np.int64), use_sin


def normal_error(x, r):
    """Absolute error bound of the kernel's normal x = r cos / sin (module docstring)."""
    return np.abs(x) * EPS_X + r * EPS_TRIG + LN2 * EPS_LOG_ABS / r


def box_muller(radu, ang, use_sin):
    r = np.sqrt(-2.0 * np.log(radu))
    phi = 2.0 * np.pi * ang
    return r * np.where(use_sin, np.sin(phi), np.cos(phi)), r


# ------------------------------------------------------------------------------------------------------------------
# Marsaglia-Tsang in fp64
# ------------------------------------------------------------------------------------------------------------------
def _eps_minus_log1p(e):
    """e - ln(1 + e), stable for small e."""
    e = np.asarray(e, np.float64)
    small = np.abs(e) < 0.05
    es = np.where(small, e, 0.0)
    s = np.zeros_like(es)
    for n in range(14, 1, -1):                      # sum_{n>=2} (-1)^n e^n / n
        s = es * (((-1.0) ** n) / n + s)
    s = es * s
    with np.errstate(invalid='ignore', divide='ignore'):
        direct = e - np.log1p(e)
    return np.where(small, s, direct)


def mt_exponent(x, c, d):
    """x^2 / 2 + d (ln v - v + 1), v = (1 + c x)^3: MT accepts u iff ln u < this (and c x > -1)."""
    t = c * x
    e = t * (3.0 + t * (3.0 + t))
    return 0.5 * x * x - d * _eps_minus_log1p(e)


def mt_exponent_exact(t, d):
    """The same for a consistent c = 1 / sqrt(9 d): 3 d [ln(1+t) - t + t^2/2 - t^3/3], series for small t."""
    t = np.asarray(t, np.float64)
    small = np.abs(t) < 0.05
    ts = np.where(small, t, 0.0)
    s = np.zeros_like(ts)
    for n in range(24, 3, -1):                      # sum_{n>=4} (-1)^(n+1) t^n / n
        s = ts * (((-1.0) ** (n + 1)) / n + s)
    s = ts ** 3 * s
    with np.errstate(invalid='ignore', divide='ignore'):
        direct = np.log1p(t) - t + t * t / 2 - t ** 3 / 3
    return 3.0 * d * np.where(small, s, direct)


def _f32_neighbours(u):
    u = np.asarray(u, np.float32)
    return (np.nextafter(u, np.float32(0)).astype(np.float64), np.nextafter(u, np.float32(2)).astype(np.float64))


def _mt_decide(x, dx, a, da, u, is_f32_u):
    """Accept decision of MT for shape a (fp64: d = a - 1/3, c = 1/sqrt(9 d)) and the near-tie mask.
    x, dx: normal and its absolute error; da: absolute error of the shape; u: the acceptance uniform."""
    with np.errstate(invalid='ignore', divide='ignore'):
        return _mt_decide_(x, dx, a, da, u, is_f32_u)


def _mt_decide_(x, dx, a, da, u, is_f32_u):
    # (a perturbation that moves 1 + c x through 0 has no exponent: fmax skips its NaN, the t > -1 margin flags it)
    d = a - 1.0 / 3.0
    c = 1.0 / np.sqrt(9.0 * d)
    lu = np.log(u)
    m0 = mt_exponent(x, c, d) - lu
    t0 = 1.0 + c * x
    acc = (m0 > 0) & (t0 > 0)
    dm = np.zeros_like(m0)
    dt = np.zeros_like(m0)
    for s in (-1.0, 1.0):
        xp = x + s * dx
        dm = np.fmax(dm, np.abs(mt_exponent(xp, c, d) - lu - m0))
        dt = np.fmax(dt, np.abs(c * s * dx))
        cp = c * (1.0 + s * DELTA_C)
        dm = np.fmax(dm, np.abs(mt_exponent(x, cp, d) - lu - m0))
        dt = np.fmax(dt, np.abs(cp * x - c * x))
        ap = a + s * da
        dp = ap - 1.0 / 3.0
        cpa = 1.0 / np.sqrt(9.0 * dp)
        dm = np.fmax(dm, np.abs(mt_exponent(x, cpa, dp) - lu - m0))
        dt = np.fmax(dt, np.abs(cpa * x - c * x))
    if is_f32_u:
        for un in _f32_neighbours(u):
            dm = np.fmax(dm, np.abs(np.log(un) - lu))
    e = c * x * (3.0 + c * x * (3.0 + c * x))
    lnv = np.where(np.abs(e) >= 0.125, d * np.abs(np.log1p(e)) * EPS_LOG, 0.0)           # ln v, direct branch (v not near 1)
    dm = dm + np.abs(lu) * EPS_LOG + LN2 * EPS_LOG_ABS + np.nan_to_num(lnv)               # the kernel's own ln u, ln v
    amb = ((np.abs(m0) <= 2 * dm) & (t0 > 0)) | (np.abs(t0) <= 2 * dt)
    return acc, amb


# ------------------------------------------------------------------------------------------------------------------
# Gamma variates
# ------------------------------------------------------------------------------------------------------------------
def classify_small(shape, precision, da):
    """The kernel's small-shape rule and its near ties.  mixed: fl32(fma(alpha, scale, -1/3)) < fl32(2/3) (the shape here is
    alpha * scale); f64: the shape is already fl32(alpha * scale), small iff < 1."""
    shape = np.asarray(shape, np.float64)
    if precision == 'mixed':
        third = float(np.float32(1.0 / 3.0))
        two3 = np.float32(2.0 / 3.0)
        rule = lambda s: (s - third).astype(np.float32) < two3   # noqa: E731
        small = rule(shape)
        amb = (rule(shape - da) != small) | (rule(shape + da) != small)
    else:
        small = shape < 1.0
        amb = np.zeros(shape.shape, dtype=bool)          # the tie sits in the rounding of alpha * scale: see sample_dirichlet
    return small, amb


def _sure(xs_true, shape, kf, kb):
    """The hot path's decision in the kernel's fp32 arithmetic (c correctly rounded): the squeeze decides the draw."""
    d = shape - 1.0 / 3.0
    with np.errstate(invalid='ignore'):
        c = (K_BM / np.sqrt(9.0 * d)).astype(np.float32)
    xs = (xs_true / K_BM).astype(np.float32)
    t = (c * xs).astype(np.float32)
    q = (xs * t).astype(np.float32)
    qq = (q * q).astype(np.float32)
    out = np.zeros(np.shape(kf), dtype=bool)
    for b in (16, 12):
        slope, top = squeeze_consts(b)
        thr = (qq.astype(np.float64) * float(slope) + float(top)).astype(np.float32)
        out = np.where(kb == b, (np.abs(t) <= np.float32(0.5)) & (np.asarray(kf, np.float32) <= thr), out)
    return out & (d > 0)


def _continuation(seed, step, traj, elem, x0, r0, kf, kb, a, da):
    """Exact path of one set of elements of shape a: block 1 (the quad's normal, u = fl32(kf + u01) 2^-KB), then fresh
    normals from blocks 2..63 of the element's own counter.  Returns (v, x, r, block, ambiguous)."""
    n = elem.size
    v = np.full(n, np.nan)
    xacc = np.full(n, np.nan)
    racc = np.full(n, np.nan)
    blk = np.zeros(n, dtype=np.int64)
    amb = np.zeros(n, dtype=bool)
    left = np.arange(n)
    d = a - 1.0 / 3.0
    for block in range(1, MAX_BLOCK + 1):
        if left.size == 0:
            break
        r = philox_elem(seed, elem[left], step, traj[left], block)
        if block == 1:
            x = x0[left]
            rr = r0[left]
            dx = normal_error(x, rr)
            # fl32(kf + u01) in fp32 arithmetic (one rounding), times the exact power of two 2^-KB
            u = ((kf[left].astype(np.float32) + u01(r[0]).astype(np.float32)).astype(np.float64) *
                 np.where(kb[left] == 16, 2.0 ** -16, 2.0 ** -12))
        else:
            x, rr = box_muller(u01(r[0]), u01(r[1]), np.zeros(left.size, dtype=bool))
            dx = normal_error(x, rr)
            u = u01(r[2])
        acc, am = _mt_decide(x, dx, a[left], da[left], u, True)
        amb[left] |= am
        hit = left[acc]
        c = 1.0 / np.sqrt(9.0 * d[hit])
        v[hit] = (1.0 + c * x[acc]) ** 3
        xacc[hit] = x[acc]
        racc[hit] = rr[acc]
        blk[hit] = block
        left = left[~acc]
    assert left.size == 0, 'the exact path ran out of its 63 blocks'
    return v, xacc, racc, blk, amb


def _value_bound(x, r, a, da, eps_extra=0.0):
    """Relative bound of y = d (1 + c x)^3 (hot and exact paths), see the module docstring."""
    d = a - 1.0 / 3.0
    c = 1.0 / np.sqrt(9.0 * d)
    t = c * x
    dt = np.abs(t) * (EPS_C + EPS_X + 0.5 * da / d) + c * (r * EPS_TRIG + LN2 * EPS_LOG_ABS / r)
    return 2 * U32 + da / d + 3.0 * dt / np.abs(1.0 + t) + 6 * U32 + eps_extra


def sample_gamma(seed, step, traj_ids, d, shape, layout='auto', precision='f64', shape_err=None, first_step_of_launch=None):
    """Gamma(shape) variates of the kernels for one env step.
    traj_ids: [B] global trajectory ids; shape: [B, d, d] fp64 (mixed: alpha * scale; f64: fl32(alpha * scale));
    shape_err: absolute error of the kernel's shape ([B, d, d] or scalar; default from `precision`);
    first_step_of_launch: the launch's first step, None = this step (models the trailing element's even-step carry).
    Returns dict(y, y_raw, path, block, bound, ambiguous, small) over [B, d, d]."""
    traj = np.asarray(traj_ids, dtype=np.uint64).reshape(-1)
    B = traj.size
    shape = np.broadcast_to(np.asarray(shape, np.float64), (B, d, d))
    if shape_err is None:
        shape_err = shape * (MIXED_ALPHA_REL if precision == 'mixed' else F64_ALPHA_REL) + \
            (2 * U32 if precision == 'mixed' else 0.0)
    da = np.broadcast_to(np.asarray(shape_err, np.float64), (B, d, d)).reshape(-1)
    step = int(step) & 0xFFFFFFFF
    key, slot, tail = keying(d, layout)
    # block 0 words per (b, i, j): one Philox evaluation per distinct key
    slotf = np.broadcast_to(slot, (B, d, d)).reshape(-1).copy()
    words = [np.zeros((B, d, d), np.uint32) for _ in range(4)]
    for is_tail in (False, True):
        sel = tail == is_tail
        if not sel.any():
            continue
        keys = np.unique(key[sel])
        qstep = step
        if is_tail:
            qstep = step & ~1
            carry = first_step_of_launch is not None and (step & 1) and int(first_step_of_launch) != step
            # the odd step takes the sine partner of the even step's pair: carried inside the launch, recomputed by a
            # launch that starts on the odd step -- the same block either way
            qstep = (step - 1) & 0xFFFFFFFF if carry else qstep
            slotf.reshape(B, d, d)[:, sel] = step & 1
        wq = philox_elem(int(seed), keys[None, :], qstep, traj[:, None], 0)
        idx = np.searchsorted(keys, key[sel])
        for k in range(4):
            words[k][:, sel] = wq[k][:, idx]
    words = [w.reshape(-1) for w in words]
    radu, ang, kf, use_sin = quad_fields(words, slotf)
    kb = quad_kbits(slotf)
    x, r = box_muller(radu, ang, use_sin)
    a = shape.reshape(-1)
    small, amb = classify_small(a, precision, da)
    n = a.size
    elem = (np.arange(d * d, dtype=np.uint64)[None, :] * np.ones((B, 1), np.uint64)).reshape(-1)
    tr = np.repeat(traj, d * d)
    y = np.full(n, np.nan)
    path = np.full(n, PATH_HOT, dtype=np.int8)
    block = np.zeros(n, dtype=np.int64)
    bound = np.zeros(n)
    # not small: hot path where the squeeze decides, the exact continuation elsewhere
    big = np.nonzero(~small)[0]
    sure = _sure(x[big], a[big], kf[big], kb[big])
    hot = big[sure]
    dh = a[hot] - 1.0 / 3.0
    y[hot] = dh * (1.0 + x[hot] / np.sqrt(9.0 * dh)) ** 3
    bound[hot] = _value_bound(x[hot], r[hot], a[hot], da[hot])
    ex = big[~sure]
    if ex.size:
        v, xa, ra, bl, am = _continuation(seed, step, tr[ex], elem[ex], x[ex], r[ex], kf[ex], kb[ex], a[ex], da[ex])
        y[ex] = (a[ex] - 1.0 / 3.0) * v
        path[ex] = PATH_EXACT
        block[ex] = bl
        amb[ex] |= am
        bound[ex] = _value_bound(xa, ra, a[ex], da[ex], 3 * U32)
    # small: Gamma(a) = Gamma(a + 1) U^(1/a), the boosted draw through the exact test from block 1, U from block 0xFFFF
    sm = np.nonzero(small)[0]
    y_raw = y.copy()
    if sm.size:
        a1 = a[sm] + 1.0
        v, xa, ra, bl, am = _continuation(seed, step, tr[sm], elem[sm], x[sm], r[sm], kf[sm], kb[sm], a1, da[sm])
        ub = u01(philox_elem(seed, elem[sm], step, tr[sm], BOOST_BLOCK)[0])
        lnu = np.log(ub)
        z = np.log2(ub) / a[sm]
        ys = (a1 - 1.0 / 3.0) * v * np.exp(lnu / a[sm])
        y_raw[sm] = ys
        uf = z < EXP2_MIN
        ez = np.abs(z) * (EPS_LOG + EPS_ROOT + 2 * U32 + da[sm] / a[sm]) + EPS_LOG_ABS / a[sm] + 2 * U32
        am |= np.abs(z - EXP2_MIN) <= 2 * ez
        y[sm] = np.where(uf, float(ZERO_GAMMA_REPLACEMENT), ys)
        path[sm] = PATH_BOOST
        block[sm] = bl
        amb[sm] |= am
        bnd = _value_bound(xa, ra, a1, da[sm], 3 * U32) + np.abs(lnu) / a[sm] * (
            EPS_LOG + EPS_ROOT + 2 * U32 + da[sm] / a[sm]) + LN2 * EPS_LOG_ABS / a[sm] + EPS_EXP + 2 * U32
        bound[sm] = np.where(uf, 0.0, bnd)
    shp = (B, d, d)
    return {'y': y.reshape(shp), 'y_raw': y_raw.reshape(shp), 'path': path.reshape(shp), 'block': block.reshape(shp),
            'bound': bound.reshape(shp), 'ambiguous': amb.reshape(shp), 'small': small.reshape(shp)}


# ------------------------------------------------------------------------------------------------------------------
# Dirichlet rows (mfg_ac2.py:236-254)
# ------------------------------------------------------------------------------------------------------------------
def concentrations(pi, theta, shift):
    """alpha_ij = ln(1 + e^{theta (pi_j - pi_i - shift)}) in fp64 from the fp32 state (mfg_ac2.py:228)."""
    p = np.asarray(pi, np.float32).astype(np.float64)
    z = float(theta) * (p[:, None, :] - p[:, :, None] - float(shift))
    return np.logaddexp(0.0, z)


def shapes(pi, theta, shift, scale, precision):
    """(shape, absolute shape error) the sampler is run with.  f64: fl32(alpha * scale) (one rounding, exact here);
    mixed: alpha * scale, the kernel's fp32 alpha carries MIXED_ALPHA_REL."""
    al = concentrations(pi, theta, shift) * float(scale)
    if precision == 'f64':
        s = al.astype(np.float32).astype(np.float64)
        return s, np.abs(s) * F64_ALPHA_REL
    return al, al * MIXED_ALPHA_REL + 2 * U32


def f64_rounding_ties(pi, theta, shift, scale):
    """f64: elements whose fl32(alpha * scale) may round the other way on the device (alpha within F64_ALPHA_REL of a
    rounding boundary) -- the small / not-small near tie of precision f64."""
    al = concentrations(pi, theta, shift) * float(scale)
    lo = (al * (1 - F64_ALPHA_REL)).astype(np.float32)
    hi = (al * (1 + F64_ALPHA_REL)).astype(np.float32)
    return (lo != hi) & ((lo < 1) != (hi < 1))


def auto_layout(d):
    """launch_core: d <= 64 -> the small-d kernels (packed / row3, one keying), otherwise k_core_large<ceil(d/64)>."""
    return 'small' if d <= 64 else 'large'


def sample_dirichlet(pi, theta, shift, scale, seed, step, traj_offset=0, precision='mixed', layout='auto',
                     first_step_of_launch=None):
    """Reference of ops.sample_dirichlet: P_ref [B, d, d] fp64 rows normalised in fp64, `bound` (absolute, on P), `ambiguous`
    (near-tie elements) and the per-element story (`path`, `block`, `y`)."""
    pi = np.asarray(pi, np.float32)
    B, d = pi.shape
    if layout == 'auto':
        layout = auto_layout(d)
    shp, err = shapes(pi, theta, shift, scale, precision)
    traj = np.uint64(traj_offset) + np.arange(B, dtype=np.uint64)
    g = sample_gamma(seed, step, traj, d, shp, layout, precision, err, first_step_of_launch)
    if precision == 'f64':
        g['ambiguous'] |= f64_rounding_ties(pi, theta, shift, scale)
    y = g['y']
    S = y.sum(-1, keepdims=True)
    P = y / S
    eps = g['bound']
    epsP = eps + (P * eps).sum(-1, keepdims=True) + (np.log2(d) + 8) * U32
    bound = P * epsP + 2.0 ** -148 / S + 2.0 ** -149
    out = dict(g)
    out.update({'P_ref': P, 'bound_y': eps, 'bound': bound})
    return out


# ------------------------------------------------------------------------------------------------------------------
# Element-wise comparison of device actions with the reference (tests/test_gpu_sampler_elementwise.py, replays)
# ------------------------------------------------------------------------------------------------------------------
MAX_AMBIGUOUS_FRACTION = 2e-5


def compare(P_dev, pi, theta, shift, scale, seed, step, traj_offset=0, precision='mixed', layout='auto',
            first_step_of_launch=None, traj_ids=None, max_ambiguous=MAX_AMBIGUOUS_FRACTION):
    """Check device actions P_dev [B, d, d] (drawn from the fp32 state pi [B, d]) against sample_dirichlet.
    Rows holding an ambiguous element are EXCLUDED from the value check (a near tie there changes that element's draw and,
    through the row sum, the rest of its row); the ambiguous elements are capped at `max_ambiguous` of all elements.
    traj_ids overrides traj_offset + arange(B) (a subsample of a larger batch).  Raises AssertionError naming (b, i, j),
    the path and the block of the worst mismatches; returns dict(worst=max err/bound, ambiguous=count, n=elements,
    rows_excluded=count, paths=counts)."""
    P_dev = np.asarray(P_dev, np.float64)
    pi = np.asarray(pi, np.float32)
    B, d = pi.shape
    if layout == 'auto':
        layout = auto_layout(d)
    if traj_ids is None:
        traj_ids = np.uint64(traj_offset) + np.arange(B, dtype=np.uint64)
    traj_ids = np.asarray(traj_ids, dtype=np.uint64)
    shp, err = shapes(pi, theta, shift, scale, precision)
    g = sample_gamma(seed, step, traj_ids, d, shp, layout, precision, err, first_step_of_launch)
    if precision == 'f64':
        g['ambiguous'] |= f64_rounding_ties(pi, theta, shift, scale)
    y = g['y']
    S = y.sum(-1, keepdims=True)
    P = y / S
    eps = g['bound']
    bound = P * (eps + (P * eps).sum(-1, keepdims=True) + (np.log2(d) + 8) * U32) + 2.0 ** -148 / S + 2.0 ** -149
    amb = g['ambiguous']
    n_amb = int(amb.sum())
    assert n_amb <= max_ambiguous * amb.size, '%d ambiguous elements of %d (cap %g): %s' % (
        n_amb, amb.size, max_ambiguous, _describe(np.argwhere(amb)[:8], g, P_dev, P, bound))
    keep = ~amb.any(-1, keepdims=True)
    ratio = np.where(keep, np.abs(P_dev - P) / bound, 0.0)
    bad = ~(ratio <= 1.0)
    if bad.any():
        idx = np.argwhere(bad)
        order = np.argsort(-ratio[bad])[:8]
        raise AssertionError('%d of %d elements outside the bound (worst err/bound %.3g):\n%s' % (
            idx.shape[0], amb.size, float(np.max(np.where(np.isnan(ratio), np.inf, ratio))),
            _describe(idx[order], g, P_dev, P, bound)))
    return {'worst': float(ratio.max()), 'ambiguous': n_amb, 'n': int(amb.size),
            'rows_excluded': int((~keep).sum()), 'paths': np.bincount(g['path'].reshape(-1), minlength=3).tolist()}


def _describe(idx, g, P_dev, P, bound):
    lines = []
    for b, i, j in idx:
        lines.append('  (b=%d, i=%d, j=%d) path=%s block=%d: dev %.9g ref %.9g bound %.3g%s' % (
            b, i, j, PATH_NAMES[g['path'][b, i, j]], g['block'][b, i, j], P_dev[b, i, j], P[b, i, j], bound[b, i, j],
            ' (ambiguous)' if g['ambiguous'][b, i, j] else ''))
    return '\n'.join(lines)


def compare_rollout(P_dev, pi_traj, theta, shift, scale, seed, first_step, traj_ids, precision='mixed', steps=None,
                    max_ambiguous=MAX_AMBIGUOUS_FRACTION):
    """compare() for every step s of a fused rollout: P_dev [n, T, d, d] against the reference at the device's own state
    pi_traj[:, s] and step first_step + s (one launch from first_step: the trailing element's even-step carry).  The cap on
    ambiguous elements applies to the whole replay.  Returns compare()'s dict summed over the steps."""
    P_dev = np.asarray(P_dev)
    pi_traj = np.asarray(pi_traj, np.float32)
    T = P_dev.shape[1]
    worst, amb, n, excl, paths = 0.0, 0, 0, 0, np.zeros(3, dtype=np.int64)
    for s in (range(T) if steps is None else steps):
        if isinstance(theta, (list, tuple, np.ndarray)):
            th = float(np.ravel(theta)[s])
        else:
            th = float(theta)
        r = compare(P_dev[:, s], pi_traj[:, s], th, shift, scale, seed, (int(first_step) + s) & 0xFFFFFFFF,
                    precision=precision, first_step_of_launch=first_step, traj_ids=traj_ids, max_ambiguous=1.0)
        worst, amb, n = max(worst, r['worst']), amb + r['ambiguous'], n + r['n']
        excl, paths = excl + r['rows_excluded'], paths + np.asarray(r['paths'])
    assert amb <= max_ambiguous * n, '%d ambiguous elements of %d in the replay (cap %g)' % (amb, n, max_ambiguous)
    return {'worst': worst, 'ambiguous': amb, 'n': n, 'rows_excluded': excl, 'paths': paths.tolist()}
