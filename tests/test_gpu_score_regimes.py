"""-m gpu: the policy-gradient score of the fused rollout kernels (k_core_small, k_core_row3, k_core_large) and of the given-P
kernels across parameter regimes, against oracle/score_ref.py.

The older oracle comparisons sit at one parameter point (theta = 8.86349, shift = 0.16, scale = 12000, Dirichlet(1) states), where
the score is well conditioned (M / |g| < 10).  Here every regime of score_ref.REGIMES runs in both precisions at d = 15 / 21 /
128 / 256 and, round-robin, at the other lane layouts; the assertion is |g - g_ref| <= bound per (trajectory, step) -- a bound
assembled from the budgets the kernels' sources state (score_ref.bound), not a relative tolerance, which would pass or fail on
the conditioning of the case.  Every case prints its worst err / bound, worst err / |g| and median M / |g| (`-s`).

Points outside the mixed sampling range |theta| (1 + |shift|) <= 86 (steep.4, steep.5: theta = 120) are held to the report
instead: the launch sets MFG_STATUS_MIXED_RANGE; precision 'f64' has no limit and is checked like every other case.
"""
import numpy as np
import pytest

torch = pytest.importorskip('torch')

pytestmark = pytest.mark.gpu

D_MAIN = [15, 21, 128, 256]
D_OTHER = [3, 4, 5, 47, 64, 65, 100, 192, 320, 449, 512]
GAMMA = 0.9


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.fail('-m gpu tests need a GPU: the HIP path has no CPU fallback')
    from discrete_mean_field_game_amd import ops
    ops.init()
    return torch.device('cuda:0')


@pytest.fixture(autouse=True)
def _auto_mapping_and_clean_status():
    yield
    from discrete_mean_field_game_amd import _lib as L, ops
    L.lib().mfg_set_core_mapping(0)
    ops.clear_status()


def _ops():
    from discrete_mean_field_game_amd import ops
    return ops


def _S():
    from oracle import score_ref
    return score_ref


def _O():
    from oracle import mfg_oracle
    return mfg_oracle


def _points():
    from oracle import score_ref
    return score_ref.regime_points()


def _sizes(d):
    T = 3 if d <= 64 else 2
    return max(3, 300_000 // (T * d * d)), T


def _cases():
    out = []
    pts = _points()
    k = 0
    for d in D_MAIN:
        for name, _ in pts:
            for precision in ('f64', 'mixed'):
                out.append(pytest.param(name, d, precision, k, id='%s-d%d-%s' % (name, d, precision)))
                k += 1
    for n, d in enumerate(D_OTHER):
        for p, precision in enumerate(('f64', 'mixed')):
            name = pts[(2 * n + p) % len(pts)][0]
            out.append(pytest.param(name, d, precision, k, id='%s-d%d-%s' % (name, d, precision)))
            k += 1
    return out


def _t32(a, dev):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device=dev)


def _t64(a, dev):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=dev)


def _reward_ref(P, pi, kind):
    """(r_ref, sum of the magnitudes of its d^2 terms), fp64.  kind 0: sum_ij pi_i (pi_j - pi_i) P_ij^2, which the kernels form
    as sum_j (pi_j s1_j - s2_j) -- a difference; kind 1: -1/2 sum_ij pi_i P_ij^2."""
    P2 = P * P
    if kind == 0:
        r = _O().calc_reward(P, pi)
        mag = np.sum(pi[..., :, None] * (pi[..., None, :] + pi[..., :, None]) * P2, axis=(-2, -1))
    else:
        r = _O().calc_reward_synthetic(P, pi)
        mag = 0.5 * np.sum(pi[..., :, None] * P2, axis=(-2, -1))
    return r, mag


def _launch(dev, pi0, T, p, w, precision, off):
    """The fused TD rollout of a case.  d > 64: with the workspace ops.rollout would allocate, the library defers V and delta of
    multiples of 16 to the matrix cores and forms delta from the fp32 reward OUTPUT (its contract, asserted by
    tests/test_gpu_fullsize.py::test_matrix_core_values_equal_in_kernel_values) -- up to 2^-24 |r| = 3.5e-9 from
    r_ref + disc V' - V where rewards are O(0.1) (measured: 2.3e-10 .. 7.4e-9 in the synthetic, mid and steep regimes at
    d = 128 / 256, against 1e-11 max(1, |V|)).  This module tests the FUSED kernels: a workspace one double short of that keeps V,
    delta and the fp64 reward inside k_core_large; the batch sums need only the part in front."""
    ex = p['extra']
    B, d = pi0.shape
    ws = _ops().workspace(B * T, d, dev)
    if d > 64 and d % 16 == 0:                                          # (the sizes whose values the library would defer)
        ws = ws[:-1]
    return _ops().rollout(_t32(pi0, dev), T, _t64([p['theta']], dev), p['shift'], p['scale'], w=_t64(w, dev), gamma=GAMMA,
                          reward_kind=ex.get('reward_kind', 0), seed=99, first_step=5, traj_offset=off, td=True, write_P=True,
                          discount_pow=ex.get('discount_pow', False), precision=precision, ws=ws)


KEYS = ['pi_traj', 'pi_last', 'reward', 'delta', 'g', 'P', 'G']


@pytest.mark.parametrize('name,d,precision,k', _cases())
def test_fused_rollout_score_across_regimes(dev, name, d, precision, k):
    from discrete_mean_field_game_amd import _lib as L
    S, O, ops = _S(), _O(), _ops()
    p = dict(_points())[name]
    theta, shift, scale = p['theta'], p['shift'], p['scale']
    kind = p['extra'].get('reward_kind', 0)
    discount_pow = p['extra'].get('discount_pow', False)
    B, T = _sizes(d)
    rs = np.random.RandomState(4000 + 13 * d + k)
    pi0 = p['states'](rs, B, d)
    F = O.num_features(d)
    w = 10.0 * rs.randn(F)                                              # critic weights of mixed sign
    off = 2 ** 32 - B // 2 if k % 3 == 0 else 1000
    ops.clear_status()
    out = _launch(dev, pi0, T, p, w, precision, off)
    if precision == 'mixed' and not p['extra'].get('mixed_in_range', True):
        # outside the documented range: reported, never silent (the outputs are unspecified, NaN where a factor overflowed)
        assert ops.status() == L.STATUS_MIXED_RANGE
        ops.clear_status()
        assert ops.status() == 0
        print('[score] %-12s d=%-3d %-5s B=%d T=%d: outside the mixed range, reported (MFG_STATUS_MIXED_RANGE)' % (name, d, precision, B, T))
        return
    assert ops.status() == 0
    for key in KEYS:
        assert bool(torch.isfinite(out[key]).all()), key
    P = out['P'].cpu().numpy()
    P64 = P.astype(np.float64)
    assert np.max(np.abs(P64.sum(-1) - 1)) < 5e-7
    pt32 = out['pi_traj'].cpu().numpy()
    pt = pt32.astype(np.float64)
    g_dev = out['g'].cpu().numpy()
    r_dev = out['reward'].cpu().numpy().astype(np.float64)
    worst_b = worst_r = 0.0
    cond = []
    for t in range(T):
        # 1. the score, per trajectory and step, against the oracle on the kernel's own P and fp32 state
        tm = S.terms(pt[:, t], P64[:, t], theta, shift)
        bd = S.bound(pt[:, t], P64[:, t], theta, shift, scale, precision, sampled=True, t=tm)
        M = S.magnitude(pt[:, t], P64[:, t], theta, shift, scale, t=tm)
        err = np.abs(g_dev[:, t] - tm['g'])
        ag = np.maximum(np.abs(tm['g']), 1e-300)
        worst_b = max(worst_b, float(np.max(err / bd)))
        worst_r = max(worst_r, float(np.max(err / ag)))
        cond.append(np.median(M / ag))
        # 2. the reward: fp64 accumulation of exact products, one fp32 rounding of the result
        r_ref, mag = _reward_ref(P64[:, t], pt[:, t], kind)
        r_err = np.abs(r_dev[:, t] - r_ref)
        r_bd = 2.0 ** -24 * np.abs(r_ref) + d * d * 2.0 ** -52 * mag
        # 3. pi' (<= 2 ulp fp32 per step)
        pn = O.transition(P64[:, t], pt[:, t])
        if t == T - 1:
            print('[score] %-12s d=%-3d %-5s B=%d T=%d: worst err/bound %.3g, worst err/|g| %.3g, M/|g| %.3g, reward err/bound %.3g' % (
                name, d, precision, B, T, worst_b, worst_r, float(np.median(cond)), float(np.max(r_err / np.maximum(r_bd, 1e-300)))))
        assert np.all(np.isfinite(bd)) and np.all(err <= bd), (name, d, precision, t, float(np.max(err / bd)))
        assert np.all(r_err <= r_bd), (name, d, precision, t, float(np.max(r_err / np.maximum(r_bd, 1e-300))))
        assert np.allclose(pt[:, t + 1], pn, rtol=3e-7, atol=1e-12)
    assert np.array_equal(out['pi_last'].cpu().numpy(), pt32[:, T])
    # 3. delta and the batch sums (forms of test_rollout_fused_vs_oracle)
    phi = O.calc_features(pt)
    V = phi.dot(w)
    disc = GAMMA ** np.arange(T) if discount_pow else np.full(T, GAMMA)
    r_all = np.stack([_reward_ref(P64[:, t], pt[:, t], kind)[0] for t in range(T)], 1)
    d_ref = r_all + disc[None] * V[:, 1:] - V[:, :-1]
    dl = out['delta'].cpu().numpy()
    assert np.max(np.abs(dl - d_ref)) < 1e-11 * max(1.0, np.abs(V).max())
    Gh = out['G'].cpu().numpy()
    Gw_ref = np.einsum('bt,btf->f', dl, phi[:, :T])
    assert np.max(np.abs(Gh[:F] - Gw_ref)) < 1e-11 * (np.abs(Gw_ref).max() + 1e-300)
    assert abs(Gh[F] - np.sum(dl * g_dev)) < 1e-10 * max(1.0, abs(np.sum(dl * g_dev)))
    assert abs(Gh[F + 1] - r_all.sum()) < 2e-7 * np.abs(r_all).sum() + 1e-18
    assert Gh[F + 2] == B * T
    # 5. both lane mappings of the packed sizes give the same bits
    if d in (15, 21):
        for mode in (1, 2):
            L.lib().mfg_set_core_mapping(mode)
            o2 = _launch(dev, pi0, T, p, w, precision, off)
            L.lib().mfg_set_core_mapping(0)
            for key in KEYS:
                assert torch.equal(o2[key], out[key]), (key, mode)
        assert ops.status() == 0


def _given_cases():
    out = []
    for k, (name, _) in enumerate(_points()):
        for precision in ('f64', 'mixed'):
            for d in (21, 128):
                out.append(pytest.param(name, d, precision, k, id='%s-d%d-%s' % (name, d, precision)))
    return out


@pytest.mark.parametrize('name,d,precision,k', _given_cases())
def test_given_P_score_with_exact_zeros(dev, name, d, precision, k):
    """ops.score and ops.td_pg_accumulate on a P with ~1 % of its entries exactly 0 (rows renormalised in fp64, stored fp32)."""
    from discrete_mean_field_game_amd import _lib as L
    S, O, ops = _S(), _O(), _ops()
    p = dict(_points())[name]
    theta, shift, scale = p['theta'], p['shift'], p['scale']
    B = max(3, 100_000 // (d * d))
    rs = np.random.RandomState(9000 + 17 * d + k)
    pi = p['states'](rs, B, d)
    pi64 = pi.astype(np.float64)
    al = np.logaddexp(0.0, theta * (pi64[:, None, :] - pi64[:, :, None] - shift))
    y = rs.gamma(np.maximum(al * scale, 1e-300))
    y[y == 0] = 1e-20
    y[rs.rand(B, d, d) < 0.01] = 0.0
    y[:, np.arange(d), np.arange(d)] = np.maximum(y[:, np.arange(d), np.arange(d)], 1e-20)     # no all-zero row
    P = (y / y.sum(-1, keepdims=True)).astype(np.float32)
    assert np.any(P == 0)
    P64 = P.astype(np.float64)
    tm = S.terms(pi64, P64, theta, shift)
    bd = S.bound(pi64, P64, theta, shift, None, precision, sampled=False, t=tm)
    M = S.magnitude(pi64, P64, theta, shift, None, t=tm)
    Pd = _t32(P, dev)
    P_before = Pd.clone()
    th = _t64([theta], dev)
    ops.clear_status()
    g1 = ops.score(_t32(pi, dev), Pd, th, shift, precision=precision).cpu().numpy()
    w = 10.0 * rs.randn(O.num_features(d))
    pn = O.transition(P64, pi64).astype(np.float32)
    r = O.calc_reward(P64, pi64).astype(np.float32)
    dl, g2, _ = ops.td_pg_accumulate(_t32(pi, dev), _t32(pn, dev), Pd, _t32(r, dev), _t64(w, dev), th, shift, GAMMA, precision=precision)
    g2 = g2.cpu().numpy()
    assert torch.equal(Pd, P_before)
    if precision == 'mixed' and not p['extra'].get('mixed_in_range', True):
        assert ops.status() == L.STATUS_MIXED_RANGE
        ops.clear_status()
        return
    assert ops.status() == 0
    ag = np.maximum(np.abs(tm['g']), 1e-300)
    for tag, g in (('score', g1), ('td_pg_accumulate', g2)):
        assert np.all(np.isfinite(g))
        err = np.abs(g - tm['g'])
        print('[score] given-P %-16s %-12s d=%-3d %-5s: worst err/bound %.3g, worst err/|g| %.3g, M/|g| %.3g' % (
            tag, name, d, precision, float(np.max(err / bd)), float(np.max(err / ag)), float(np.median(M / ag))))
        assert np.all(err <= bd), (tag, name, d, precision, float(np.max(err / bd)))
    V = O.calc_features(pi64).dot(w)
    Vn = O.calc_features(pn.astype(np.float64)).dot(w)
    assert np.max(np.abs(dl.cpu().numpy() - (r.astype(np.float64) + GAMMA * Vn - V))) < 1e-11 * max(1.0, np.abs(V).max())
