"""-m gpu: the launch-once kernels of csrc/mfg_launch_once.hip (k_value, k_features, k_alpha, k_jsd, k_policy_logpdf,
k_backward_value, k_dirichlet_from_gamma, k_gather_start, k_draw_start, k_philox_raw, k_apply_update) past the grid cap and
past the 64-lane width, against the NumPy oracles.

Each of these kernels has two loops that the other modules take once only:

* the grid-stride loop.  grid_for(work, per_block, 8) caps the grid at 8 blocks per CU, so a wave-per-row kernel takes a second
  pass above Wc = 8 * CUs * 4 rows and an element-per-thread kernel above Tc = 8 * CUs * 256 elements.  Both are derived from
  the CU count mfg_device_info reports; the `past_cap` case of every kernel has 2 * cap + 3 work items (two full passes and a
  ragged third) at the smallest d that keeps the buffers to a few MB;
* the lane loop `for (j = lane; j < d; j += 64)`: the `d<n>` cases run d in {1, 2, 63, 64, 65, 129, 512} with 2-6 rows.

Every output is pre-filled with a sentinel (NaN / a negative index), so an element no thread wrote fails the comparison.  The
tolerances are the ones of the older test of the same kernel, or follow from the arithmetic the kernel states (see each test);
every case prints its worst error against its bound (`-s`).
"""
import functools
import math
from fractions import Fraction

import numpy as np
import pytest

torch = pytest.importorskip('torch')

pytestmark = pytest.mark.gpu

LANE_EDGES = [1, 2, 63, 64, 65, 129, 512]
THETA, SHIFT = 8.86349, 0.16


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.fail('-m gpu tests need a GPU: the HIP path has no CPU fallback')
    from discrete_mean_field_game_amd import ops
    ops.init()
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def caps(dev):
    """(Wc, Tc): rows / elements one pass of the capped grid covers -- grid_for(.., 8): 8 blocks per CU of 4 waves / 256 threads."""
    import ctypes as C
    from discrete_mean_field_game_amd import _lib as L
    cu = C.c_int(0)
    L.check(L.lib().mfg_device_info(C.byref(cu), None, 0), 'mfg_device_info')
    assert cu.value > 0
    return 8 * cu.value * 4, 8 * cu.value * 256


def _O():
    from oracle import mfg_oracle
    return mfg_oracle


def _call(name, *args):
    """One C ABI call on torch's current stream.  The tests call the ABI themselves (not ops.*) wherever they hand in the
    sentinel-filled outputs."""
    from discrete_mean_field_game_amd import _lib as L
    L.check(getattr(L.lib(), name)(*args, torch.cuda.current_stream().cuda_stream), name)


def _t(a, dev, dtype):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=dtype), device=dev)


def _nan(shape, dev, dtype=torch.float64):
    return torch.full(shape, float('nan'), dtype=dtype, device=dev)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _bits(t):
    """Host copy of a float tensor as integers: bit-for-bit comparisons that NaN cannot slip through."""
    a = t.cpu().numpy()
    return a.view(np.int64 if a.dtype == np.float64 else np.int32)


def _ceil_div(a, b):
    return -(-a // b)


def _case_ids(ds):
    return ['past_cap'] + ['d%d' % d for d in ds]


def _report(kernel, case, what, err, bound):
    print('\n%-22s %-9s %-12s worst err %.3e  bound %.3e' % (kernel, case, what, err, bound), end='')


def _states(rs, B, d, kind='dir1'):
    """[B, d] fp32 states: Dirichlet(1), Dirichlet(0.3) (a few large entries) or one-hot."""
    if kind == 'onehot':
        pi = np.zeros((B, d), dtype=np.float32)
        pi[np.arange(B), rs.randint(d, size=B)] = 1.0
        return pi
    return rs.dirichlet(np.ones(d) * (0.3 if kind == 'dir0.3' else 1.0), size=B).astype(np.float32)


def _shape(case, past_cap, rows=4, rows512=2):
    """(d, B) of a case id: `past_cap` -> the (d, B) given, `d<n>` -> n with `rows` rows (`rows512` at d = 512)."""
    if case == 'past_cap':
        return past_cap
    d = int(case[1:])
    return d, (rows512 if d == 512 else rows)


# ---------------------------------------------------------------------------------------------------
# k_value
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('states', ['onehot', 'dir0.3'])
@pytest.mark.parametrize('case', _case_ids(LANE_EDGES))
def test_value(dev, caps, case, states):
    """V = phi(pi) . w with w of mixed sign.  Kernel and oracle are both fp64 sums of the F terms w_k phi_k (phi_k, a product of
    two fp32 numbers, is exact), each in its own order: |V - V_ref| <= F 2^-52 sum_k |w_k phi_k| per state (F 2^-53 each).  An
    absolute bound: the mixed-sign sum cancels, so a relative one would pass or fail on the conditioning of the state."""
    d, B = _shape(case, (3, 2 * caps[0] + 3), rows=6)
    rs = np.random.RandomState(100 + d)
    pi = _states(rs, B, d, states)
    F = _O().num_features(d)
    w = 10.0 * rs.randn(F)
    pid, wd, out = _t(pi, dev, np.float32), _t(w, dev, np.float64), _nan((B,), dev)
    _call('mfg_value', pid.data_ptr(), wd.data_ptr(), B, d, out.data_ptr())
    got = out.cpu().numpy()
    phi = _O().calc_features(pi)
    ref = phi.dot(w)
    bound = F * 2.0 ** -52 * np.abs(phi * w).sum(-1)
    err = np.abs(got - ref)
    k = int(np.argmax(np.where(np.isnan(err), np.inf, err) / bound))
    _report('k_value', case, states, err[k], bound[k])
    assert not np.isnan(got).any()
    assert np.all(err <= bound)


# ---------------------------------------------------------------------------------------------------
# k_features
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', _case_ids(LANE_EDGES))
def test_features(dev, caps, case):
    """phi(pi): products of two fp32 numbers are exact in fp64, so the comparison is array_equal."""
    d, B = _shape(case, (8, _ceil_div(2 * caps[1] + 3, 64)))
    pi = _states(np.random.RandomState(200 + d), B, d)
    F = _O().num_features(d)
    pid, out = _t(pi, dev, np.float32), _nan((B, F), dev)
    _call('mfg_features', pid.data_ptr(), B, d, out.data_ptr())
    got = out.cpu().numpy()
    ref = _O().calc_features(pi)
    _report('k_features', case, 'B=%d' % B, float(np.max(np.abs(got - ref))), 0.0)
    assert np.array_equal(got, ref)


# ---------------------------------------------------------------------------------------------------
# k_alpha
# ---------------------------------------------------------------------------------------------------
def _alpha_all(dev, pi, theta, shift):
    """(alpha, alpha') of the two-output call, after checking that each single-output call gives the same bits."""
    B, d = pi.shape
    pid, th = _t(pi, dev, np.float32), _t([theta], dev, np.float64)
    a, ad = _nan((B, d, d), dev), _nan((B, d, d), dev)
    _call('mfg_alpha', pid.data_ptr(), B, d, th.data_ptr(), shift, a.data_ptr(), ad.data_ptr())
    a1, ad1 = _nan((B, d, d), dev), _nan((B, d, d), dev)
    _call('mfg_alpha', pid.data_ptr(), B, d, th.data_ptr(), shift, a1.data_ptr(), None)
    _call('mfg_alpha', pid.data_ptr(), B, d, th.data_ptr(), shift, None, ad1.data_ptr())
    assert not torch.isnan(a).any() and not torch.isnan(ad).any()
    assert np.array_equal(_bits(a1), _bits(a)) and np.array_equal(_bits(ad1), _bits(ad))
    return a.cpu().numpy(), ad.cpu().numpy()


def _alpha_check(case, what, a, ad, pi, theta, shift):
    """alpha against ln(1 + e^z) in its log1p form (the reference's log(1 + exp(z)) loses the digits of alpha for z << 0, see
    test_gpu_parity.py::test_score_beyond_the_h_table_and_extreme_theta): 1e-9 relative; alpha' against calc_alpha_deriv:
    1e-14 absolute -- the bounds of test_golden_functions_on_device."""
    p64 = pi.astype(np.float64)
    z = theta * (p64[:, None, :] - p64[:, :, None] - shift)
    ref_a = np.log1p(np.exp(z))
    ea = float(np.max(np.abs(a - ref_a) / np.maximum(np.abs(ref_a), 1e-300)))
    ed = float(np.max(np.abs(ad - _O().calc_alpha_deriv(pi, theta, shift))))
    _report('k_alpha', case, what + ' alpha', ea, 1e-9)
    _report('k_alpha', case, what + " alpha'", ed, 1e-14)
    assert ea < 1e-9
    assert ed < 1e-14
    return z


@pytest.mark.parametrize('case', _case_ids(LANE_EDGES))
def test_alpha(dev, caps, case):
    d, B = _shape(case, (8, _ceil_div(2 * caps[1] + 3, 64)))
    pi = _states(np.random.RandomState(300 + d), B, d)
    a, ad = _alpha_all(dev, pi, THETA, SHIFT)
    _alpha_check(case, 'B=%d' % B, a, ad, pi, THETA, SHIFT)


@pytest.mark.parametrize('theta', [0.5, 8.86349, 60.0, 120.0])
def test_alpha_one_hot_states_reach_the_ends_of_z(dev, theta):
    """One-hot states put x = pi_j - pi_i - shift at 1 - shift, -1 - shift and -shift: z reaches +-theta (1 + |shift|), with
    the shift of either sign -- alpha from 1e-61 to 139."""
    d, B = 21, 6
    pi = _states(np.random.RandomState(int(theta)), B, d, 'onehot')
    for shift in (SHIFT, -SHIFT):
        a, ad = _alpha_all(dev, pi, theta, shift)
        z = _alpha_check('d21', 'theta=%g' % theta, a, ad, pi, theta, shift)
        assert abs(np.max(np.abs(z)) - theta * (1.0 + SHIFT)) < 1e-6 * theta


# ---------------------------------------------------------------------------------------------------
# k_jsd
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', _case_ids([1, 64, 65, 512]))
def test_jsd(dev, caps, case):
    """Rows 0..3 carry an exact zero in p, in q, in both at the same index, and p == q (JSD = 0).  rtol 1e-9 / atol 1e-15, the
    bounds of test_jsd_batched."""
    d, B = _shape(case, (3, 2 * caps[0] + 3), rows=6, rows512=6)
    rs = np.random.RandomState(400 + d)
    p, q = _states(rs, B, d), _states(rs, B, d)
    p[0, 0] = 0.0
    q[1, d - 1] = 0.0
    p[2, d // 2] = q[2, d // 2] = 0.0
    q[3] = p[3]
    if case == 'past_cap':                                    # the same four kinds of row in the ragged third pass
        p[-1, 0] = 0.0
        q[-2, d - 1] = 0.0
        p[-3, d // 2] = q[-3, d // 2] = 0.0
        q[-4] = p[-4]
    pd, qd, out = _t(p, dev, np.float32), _t(q, dev, np.float32), _nan((B,), dev)
    _call('mfg_jsd', pd.data_ptr(), qd.data_ptr(), B, d, out.data_ptr())
    got = out.cpu().numpy()
    ref = _O().JSD(p, q)
    err = np.abs(got - ref)
    bound = 1e-15 + 1e-9 * np.abs(ref)
    k = int(np.argmax(np.where(np.isnan(err), np.inf, err) / bound))
    _report('k_jsd', case, 'B=%d' % B, err[k], bound[k])
    assert not np.isnan(got).any()
    assert np.allclose(got, ref, rtol=1e-9, atol=1e-15)
    assert abs(got[3]) <= 1e-15


# ---------------------------------------------------------------------------------------------------
# k_policy_logpdf
# ---------------------------------------------------------------------------------------------------
def _logpdf_cases():
    out = [pytest.param('past_cap', 3, id='past_cap-K3')]
    for d in LANE_EDGES[:-1]:
        for K in (1, 5):
            out.append(pytest.param('d%d' % d, K, id='d%d-K%d' % (d, K)))
    return out


def _assert_logpdf(got, pi, P, thetas, setting, case, what):
    """got [N, K] against the oracle under setting = (shift, alpha_scale, alpha_floor, p_floor): 1e-10 relative with floor 1."""
    want = _O().policy_logpdf(pi, P, thetas, *setting)
    err = float(np.max(np.abs(got - want) / np.maximum(np.abs(want), 1.0)))
    _report('k_policy_logpdf', case, what, err, 1e-10)
    assert not np.isnan(got).any()
    assert err < 1e-10


@pytest.mark.parametrize('case,K', _logpdf_cases())
def test_policy_logpdf(dev, caps, case, K):
    """The three (alpha_scale, alpha_floor, p_floor) settings and the bound of test_policy_logpdf_vs_oracle: 1e-10 relative with
    floor 1.  One wavefront per (sample, policy): the past_cap case has N K >= 2 Wc + 3 of them."""
    d, N = _shape(case, (4, _ceil_div(2 * caps[0] + 3, K)), rows=3)
    rs = np.random.RandomState(500 + d + K)
    pi = _states(rs, N, d)
    P = rs.dirichlet(np.ones(d) * 2.0, size=(N, d)).astype(np.float32)
    thetas = np.array([2.0, 6.5, 8.64, 0.5, 4.0])[:K] if K != 1 else np.array([6.5])
    pid, Pd, thd = _t(pi, dev, np.float32), _t(P, dev, np.float32), _t(thetas, dev, np.float64)
    for scale, floor, pfloor in [(1.0, 0.0, 0.0), (1.0, 1.0 + 1e-6, 0.0), (50.0, 0.0, 1e-6)]:
        out = _nan((N, K), dev)
        _call('mfg_policy_logpdf', pid.data_ptr(), Pd.data_ptr(), N, d, thd.data_ptr(), K, 0.05, scale, floor, pfloor,
              out.data_ptr())
        _assert_logpdf(out.cpu().numpy(), pi, P, thetas, (0.05, scale, floor, pfloor), case, 'K=%d s=%g' % (K, scale))


# ---------------------------------------------------------------------------------------------------
# k_backward_value
# ---------------------------------------------------------------------------------------------------
def _backward_cases():
    out = [pytest.param('past_cap', 2, 1.0, id='past_cap-T2')]
    out += [pytest.param('d%d' % d, 3, 1.0, id='d%d-T3' % d) for d in LANE_EDGES]
    out += [pytest.param('d21', T, 0.05, id='d21-T%d-near_one_hot' % T) for T in (1, 15)]
    return out


@pytest.mark.parametrize('case,T,conc', _backward_cases())
def test_backward_value(dev, caps, case, T, conc):
    """V^n = r^n + P^n V^{n+1} with V^{n+1} carried in a per-wave LDS line across the grid-stride loop, and the two consistency
    metrics, against evaluate_synthetic_diffs on the same fp32 actions.  Bounds of test_backward_value_kernel_vs_reference_golden:
    V rtol 1e-12 / atol 1e-13, l1 rtol 1e-12, jsd rtol 1e-10 (on these input families the fp64 oracle lies within 4e-15 of an
    extended-precision restatement, so they carry more than 100x margin over the reference's own rounding).  Rows are
    Dirichlet(1) or Dirichlet(0.05) (near one-hot; underflows to exact zeros in fp32), and trajectory 0 -- at past_cap also the
    last one -- has exact zeros planted in every row.  want_jsd = False must give the same V and l1 bits."""
    d, B = _shape(case, (5, 2 * caps[0] + 3), rows=(6 if conc != 1.0 else 4))
    rs = np.random.RandomState(600 + d + T)
    P = rs.dirichlet(np.ones(d) * conc, size=(B, T, d)).astype(np.float32)
    if d > 1:
        for b in sorted({0, B - 1} if case == 'past_cap' else {0}):
            P[b, :, np.arange(d), (np.arange(d) + 1) % d] = 0.0
            P[b, 0, 0, 0] = 0.0
    Pd = _t(P, dev, np.float32)
    V, l1, js = _nan((B, T + 1, d), dev), _nan((B, T), dev), _nan((B, T), dev)
    _call('mfg_backward_value', Pd.data_ptr(), B, T, d, V.data_ptr(), l1.data_ptr(), js.data_ptr())
    V2, l12 = _nan((B, T + 1, d), dev), _nan((B, T), dev)
    _call('mfg_backward_value', Pd.data_ptr(), B, T, d, V2.data_ptr(), l12.data_ptr(), None)
    Vo, l1o, jso = _O().evaluate_synthetic_diffs(P)
    for name, got, ref, rtol, atol in (('V', V.cpu().numpy(), Vo, 1e-12, 1e-13), ('l1', l1.cpu().numpy(), l1o, 1e-12, 0.0),
                                       ('jsd', js.cpu().numpy(), jso, 1e-10, 0.0)):
        err = np.abs(got - ref)
        bound = atol + rtol * np.abs(ref)
        ratio = np.where(np.isnan(err), np.inf, err) / np.where(bound > 0, bound, 1.0)
        ratio = np.where((bound == 0) & (err == 0), 0.0, ratio)
        k = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
        _report('k_backward_value', case, 'T=%d %s' % (T, name), err[k], bound[k])
        assert not np.isnan(got).any()
        assert np.allclose(got, ref, rtol=rtol, atol=atol), name
    assert np.array_equal(_bits(V2), _bits(V)) and np.array_equal(_bits(l12), _bits(l1))


# ---------------------------------------------------------------------------------------------------
# k_dirichlet_from_gamma
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', _case_ids([1, 64, 65, 129, 512]))
def test_dirichlet_from_gamma(dev, caps, case):
    """One wavefront per row of gamma variates [B, d, d] -> B d rows.  The kernel rounds v * (1 / s) (fp64) to fp32, the oracle
    v / s: both lie within half an fp32 ulp (and a few fp64 ulps) of the exact quotient, hence within ONE fp32 ulp of each
    other.  Every entry > 0 (zeros count as 1e-20), an all-zero row becomes uniform 1 / d, and a row of d fp32 roundings sums to 1
    within d 2^-24."""
    d, B = _shape(case, (3, _ceil_div(2 * caps[0] + 3, 3)), rows=2)
    if d == 512:
        B = 1
    rs = np.random.RandomState(700 + d)
    y = rs.gamma(2.0, size=(B, d, d)).astype(np.float32)
    rows = y.reshape(B * d, d)
    n = rows.shape[0]
    zero_rows = [0, n - 1] if n > 1 else [0]
    for r in zero_rows:
        rows[r] = 0.0
    for r in ([1, n - 2] if n > 3 else []):                  # some zeros in a row, one of them past the first 64 lanes
        rows[r, ::3] = 0.0
        rows[r, d - 1] = 0.0
    yd, out = _t(y, dev, np.float32), _nan((B, d, d), dev, torch.float32)
    _call('mfg_dirichlet_from_gamma', yd.data_ptr(), B, d, out.data_ptr())
    got = out.cpu().numpy().reshape(n, d)
    ref = _O().dirichlet_from_gamma(rows).astype(np.float32)
    assert not np.isnan(got).any()
    ulps = np.abs(got.astype(np.float64) - ref.astype(np.float64)) / np.spacing(np.abs(ref)).astype(np.float64)
    sums = np.abs(got.astype(np.float64).sum(-1) - 1.0)
    _report('k_dirichlet_from_gamma', case, 'ulps', float(ulps.max()), 1.0)
    _report('k_dirichlet_from_gamma', case, 'row sums', float(sums.max()), d * 2.0 ** -24)
    assert np.all(ulps <= 1.0)
    assert np.all(got > 0)
    assert np.all(sums <= d * 2.0 ** -24)
    for r in zero_rows:
        assert np.array_equal(got[r], np.full(d, np.float32(1.0 / d)))


# ---------------------------------------------------------------------------------------------------
# k_gather_start
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', _case_ids([512]))
def test_gather_start(dev, caps, case):
    """Index bookkeeping: bit exact.  Indices -5 and num_start + 7 are clamped into the table, as start_row documents."""
    d, B = (3, _ceil_div(2 * caps[1] + 3, 3)) if case == 'past_cap' else (512, 3)
    num_start = 64
    rs = np.random.RandomState(800 + d)
    mat = rs.dirichlet(np.ones(d), size=num_start).astype(np.float32)
    idx = rs.randint(num_start, size=B).astype(np.int32)
    idx[0], idx[-1] = -5, num_start + 7
    if B > 4:
        idx[B // 2], idx[B // 2 + 1] = num_start + 7, -5
    matd, idxd, out = _t(mat, dev, np.float32), _t(idx, dev, np.int32), _nan((B, d), dev, torch.float32)
    _call('mfg_gather_start', matd.data_ptr(), num_start, idxd.data_ptr(), B, d, out.data_ptr())
    got = out.cpu().numpy()
    _report('k_gather_start', case, 'B=%d' % B, float(np.sum(_bits(out) != mat[np.clip(idx, 0, num_start - 1)].view(np.int32))),
            0.0)
    assert np.array_equal(got, mat[np.clip(idx, 0, num_start - 1)])


# ---------------------------------------------------------------------------------------------------
# k_draw_start
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', ['past_cap-idx_only', 'past_cap-rows'])
def test_draw_start(dev, caps, case):
    """The start-state draw against oracle/philox_ref.start_indices, bit exact, with traj_offset = 2^32 - 5 so that the global
    trajectory ids cross the 32-bit word of the counter.  idx only: one thread per trajectory, B = 2 Tc + 3; with rows: one
    thread per element, B d >= 2 Tc + 3, rows with and without idx, and the idx-only call gives the idx of the idx + rows call."""
    from oracle.philox_ref import start_indices
    d, num_start, seed, step, off = 3, 1000, 0x9E3779B97F4A7C15, 4_000_000_000, 2 ** 32 - 5
    B = 2 * caps[1] + 3 if case == 'past_cap-idx_only' else _ceil_div(2 * caps[1] + 3, d)
    mat = np.random.RandomState(900).dirichlet(np.ones(d), size=num_start).astype(np.float32)
    matd = _t(mat, dev, np.float32)
    ref = start_indices(seed, step, off + np.arange(B, dtype=np.uint64), num_start)

    def draw(want_idx, want_rows):
        idx = torch.full((B,), -7, dtype=torch.int32, device=dev) if want_idx else None
        rows = _nan((B, d), dev, torch.float32) if want_rows else None
        _call('mfg_draw_start', matd.data_ptr(), num_start, B, d, seed, step, off, _ptr(idx), _ptr(rows))
        return (None if idx is None else idx.cpu().numpy()), (None if rows is None else rows.cpu().numpy())

    idx, _ = draw(True, False)
    _report('k_draw_start', case, 'B=%d idx' % B, float(np.sum(idx != ref)), 0.0)
    assert np.array_equal(idx, ref)
    if case == 'past_cap-rows':
        idx2, rows = draw(True, True)
        _, rows_only = draw(False, True)
        _report('k_draw_start', case, 'B=%d rows' % B, float(np.sum(rows.view(np.int32) != mat[ref].view(np.int32))), 0.0)
        assert np.array_equal(idx2, idx)
        assert np.array_equal(rows, mat[ref]) and np.array_equal(rows_only, mat[ref])


# ---------------------------------------------------------------------------------------------------
# k_philox_raw
# ---------------------------------------------------------------------------------------------------
def test_philox_raw_past_cap(dev, caps):
    """n = 2 Tc + 3 blocks from the first counter 2^32 - 7: c0 = first + e wraps in 32 bits.  Bit exact against philox4x32_10."""
    from oracle.philox_ref import philox4x32_10
    seed, first, n = 0x9E3779B97F4A7C15, 2 ** 32 - 7, 2 * caps[1] + 3
    out = torch.full((n, 4), 0x55555555, dtype=torch.int32, device=dev)
    _call('mfg_philox_raw', seed, first, 7, 0xDEADBEEF, 0x10002, n, out.data_ptr())
    got = out.cpu().numpy().view(np.uint32)
    c0 = (np.uint64(first) + np.arange(n, dtype=np.uint64)) & np.uint64(0xFFFFFFFF)
    ref = np.stack(philox4x32_10(c0, 7, 0xDEADBEEF, 0x10002, seed & 0xFFFFFFFF, seed >> 32), axis=1)
    _report('k_philox_raw', 'past_cap', 'n=%d' % n, float(np.sum(got != ref)), 0.0)
    assert np.array_equal(got, ref)


# ---------------------------------------------------------------------------------------------------
# k_apply_update
# ---------------------------------------------------------------------------------------------------
def _fma(a, b, c):
    """a * b + c with ONE rounding: math.fma where the interpreter has it, else the exact rational sum rounded once (the
    conversion of a Fraction to float rounds correctly)."""
    if hasattr(math, 'fma'):
        return math.fma(a, b, c)
    return float(Fraction(a) * Fraction(b) + Fraction(c))


LR_C, LR_A, COUNT = 0.1, 0.001, 7.0                         # 1 / 7 is inexact: the order of the operations shows


@functools.lru_cache(maxsize=None)
def _update_case(d):
    """(G, w0, theta0, expected w, expected theta) of an update at d, shared by the cases of that d (read only)."""
    F = _O().num_features(d)
    rs = np.random.RandomState(1000 + d)
    G = rs.randn(F + 3)
    G[F + 2] = COUNT
    w0, th0 = rs.randn(F), 8.86349
    inv = 1.0 / COUNT
    ref_w = np.array([_fma(LR_C, float(g) * inv, float(p)) for g, p in zip(G[:F], w0)])
    return G, w0, th0, ref_w, _fma(LR_A, float(G[F]) * inv, th0)


@pytest.mark.parametrize('with_reward_acc', [False, True], ids=['no_reward_acc', 'reward_acc'])
@pytest.mark.parametrize('d', [1, 21, 22, 64, 512], ids=lambda d: 'd%d' % d)
def test_apply_update(dev, d, with_reward_acc):
    """p <- fma(lr, G_k (1 / N), p) (updated_param, mfg_device.h) for the F weights and theta, bit exact; one element per
    thread: F = 253 at d = 21 is one block, d = 22 the first with two.  reward_acc += G[F + 1] (1 / N) is written as a product
    and a sum in one statement, which the compiler may contract: either rounding of it is accepted, bit exact.  A batch of no
    samples (G[F + 2] = 0) leaves w, theta and reward_acc bit-unchanged; G is never written."""
    from discrete_mean_field_game_amd import ops
    F = _O().num_features(d)
    G0, w0, th0, ref_w, ref_th = _update_case(d)
    acc0 = -3.25
    for count in (COUNT, 0.0):
        G = G0.copy()
        G[F + 2] = count
        Gd, w, th = _t(G, dev, np.float64), _t(w0, dev, np.float64), _t([th0], dev, np.float64)
        acc = _t([acc0], dev, np.float64) if with_reward_acc else None
        ops.apply_update(Gd, d, LR_C, LR_A, w, th, acc)
        got_w, got_th = w.cpu().numpy(), float(th[0])
        assert np.array_equal(Gd.cpu().numpy(), G)
        if count == 0.0:
            assert np.array_equal(got_w.view(np.int64), w0.view(np.int64)) and got_th == th0
            assert acc is None or float(acc[0]) == acc0
            continue
        inv = 1.0 / count
        ulp = np.abs(got_w - ref_w) / np.spacing(np.abs(ref_w))
        _report('k_apply_update', 'd%d' % d, 'w ulps', float(ulp.max()), 0.0)
        assert np.array_equal(got_w.view(np.int64), ref_w.view(np.int64))
        assert got_th == ref_th
        if acc is not None:
            assert float(acc[0]) in (acc0 + float(G[F + 1]) * inv, _fma(float(G[F + 1]), inv, acc0))
