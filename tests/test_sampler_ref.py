"""CPU tests of oracle/sampler_ref.py, the element-wise restatement of the in-kernel Dirichlet sampler (no GPU).

(a) the keying of docs/KERNELS.md "Sampler keying" is injective for every d and kernel family; (b) the hot path's squeeze is
sound -- the claim behind "the sampler is exact"; (c) the restatement draws Gamma(a); (d) the even-step carry of a row's
single trailing element does not depend on where a rollout is cut into launches.
"""
import numpy as np
import pytest

from oracle import philox_ref as PR
from oracle import sampler_ref as S

FAMILIES = [('small', range(1, 65)), ('large', range(65, 513))]


def _kernel_lane_grid(d):
    """k_core_large<R>: every (row, column) a lane computes, columns c = lane + 64 m >= d included (their results are
    discarded).  Returns (i, c) arrays."""
    R = -(-d // 64)
    i, c = np.meshgrid(np.arange(d), np.arange(64 * R), indexing='ij')
    return i, c


@pytest.mark.parametrize('family,ds', FAMILIES, ids=[f[0] for f in FAMILIES])
def test_keying_is_injective(family, ds):
    for d in ds:
        key, slot, tail = S.keying(d, family)
        ids = np.arange(d * d, dtype=np.uint64).reshape(d, d)
        # each element exactly one (key, slot); a key is a real element id of its own quad's first member
        pairs = key.astype(np.uint64) * np.uint64(4) + slot.astype(np.uint64)
        assert np.unique(pairs).size == d * d, d
        assert slot.min() >= 0 and slot.max() <= 3
        assert np.all(np.isin(key, ids)), d
        # a quad's key is the id of one of its members, and that member sits in slot 0
        k0 = ids[slot == 0]
        assert np.array_equal(np.unique(key), np.unique(k0)), d
        # quads hold at most 4 elements; the small family: columns 4q .. 4q + 3 of one row, 1..3 trailing ones keyed by
        # the first of them, the single trailing element (d = 1 mod 4) alone in its (tail) block
        _, cnt = np.unique(key, return_counts=True)
        assert cnt.max() <= 4
        if family == 'small':
            assert np.array_equal(tail[:, -1], np.full(d, d % 4 == 1)) and tail.sum() == (d if d % 4 == 1 else 0)
            assert np.all(key // np.uint64(d) == np.arange(d, dtype=np.uint64)[:, None])       # quads never cross rows
        else:
            R = -(-d // 64)
            assert not tail.any()
            if R % 4 == 0 and d % 64 == 0:
                assert np.all(cnt == 4)
            # the large family's key is the quad's (even row, column lane + 64 m0) element
            kr, kc = key // np.uint64(d), key % np.uint64(d)
            if R % 4:
                assert np.all(kr % np.uint64(2) == 0)
            assert np.all(kc % np.uint64(64) == np.arange(d, dtype=np.uint64)[None, :] % np.uint64(64))


@pytest.mark.parametrize('d', [65, 100, 129, 191, 193, 255, 257, 320, 383, 449, 511])
def test_large_columns_past_d_alias_but_never_key_a_live_quad(d):
    """The lanes of k_core_large compute columns c >= d too: their ids i d + c alias real elements (i + 1, c - d), but the
    block of a quad that holds any real element is keyed by a real element of that quad, never by such an alias."""
    R = -(-d // 64)
    i, c = _kernel_lane_grid(d)
    lane, m = c % 64, c // 64
    if R % 4 == 0:
        m0 = (m // 4) * 4
        key_i, key_c = i, lane + 64 * m0
    else:
        m0 = (m // 2) * 2
        key_i, key_c = (i // 2) * 2, lane + 64 * m0
    phantom = c >= d
    alias = (i * d + c)[phantom]
    assert alias.size == 0 or alias.max() < d * d + d     # the aliases are ids of real elements (or one past the last row)
    live_keys = np.unique((key_i * d + key_c)[~phantom])
    assert np.all(key_c[~phantom] < d)
    ref_key, _, _ = S.keying(d, 'large')
    assert np.array_equal(np.unique(ref_key).astype(np.int64), live_keys)
    # a quad keyed by a column >= d (an aliasing id) holds no real element: it is computed and discarded
    assert np.all(phantom[key_c >= d])


def test_counters_of_quads_and_continuations_never_collide():
    """block 0 = quads, 1..63 = continuation, 0xFFFF = boost: the block sits above the 16 high trajectory bits of c3."""
    traj = np.array([0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 2 ** 47, 2 ** 48 - 1], dtype=np.uint64)
    c3 = {}
    for blk in [0] + list(range(1, 64)) + [0xFFFF]:
        for t in traj:
            v = (int(t) & 0xFFFFFFFF, ((int(t) >> 32) & 0xFFFF) | (blk << 16))
            assert v not in c3, (blk, t)
            c3[v] = (blk, t)


def test_trajectory_ids_across_2_32_and_the_48_bit_edge():
    seed, elem, step = 0x1234567890ABCDEF, 17, 3
    ts = np.array([2 ** 32 - 2, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 2 ** 47, 2 ** 48 - 2, 2 ** 48 - 1], dtype=np.uint64)
    w = np.stack(PR.philox_elem(seed, elem, step, ts, 0), 1)
    assert np.unique(w, axis=0).shape[0] == ts.size             # distinct ids below 2^48: distinct streams
    # the counter keeps 48 bits of the id: 2^48 + t draws t's stream -- the C entry points reject traj_offset + B > 2^48
    # (include/mfg_hip.h; tests/test_gpu_sampler_elementwise.py::test_trajectory_ids_past_2_48_are_rejected)
    wrap = np.stack(PR.philox_elem(seed, elem, step, ts[:3] + np.uint64(2 ** 48), 0), 1)
    assert np.array_equal(wrap, w[:3])


# ------------------------------------------------------------------------------------------------------------------------
def _sure_threshold_kf(x, a, kb, c_ulps):
    """Largest acceptance integer the kernel's fp32 squeeze calls sure (-1: none), with the kernel's c moved by c_ulps."""
    d = a - 1.0 / 3.0
    c = (S.K_BM / np.sqrt(9.0 * d)).astype(np.float32)
    for _ in range(abs(c_ulps)):
        c = np.nextafter(c, np.float32(np.inf if c_ulps > 0 else 0))
    xs = (x / S.K_BM).astype(np.float32)
    t = (c * xs).astype(np.float32)
    q = (xs * t).astype(np.float32)
    qq = (q * q).astype(np.float32)
    slope, top = S.squeeze_consts(kb)
    thr = (qq.astype(np.float64) * float(slope) + float(top)).astype(np.float32)
    kf = np.floor(thr.astype(np.float64))
    kf = np.minimum(kf, 2 ** kb - 1)
    return np.where(np.abs(t) <= np.float32(0.5), kf, -1.0)


def _squeeze_slack(x, a, kb):
    """min over c +- 2 ulp of  E(x) - ln(top of the highest sure cell)  (>= 0: fp64 MT accepts every u of every sure cell)."""
    d = a - 1.0 / 3.0
    E = S.mt_exponent_exact(x / np.sqrt(9.0 * d), d)
    slack = np.full(np.shape(x), np.inf)
    for cu in (-2, -1, 0, 1, 2):
        kf = _sure_threshold_kf(x, a, kb, cu)
        with np.errstate(divide='ignore', invalid='ignore'):
            s = E - np.log(np.maximum(kf + 1.0, 1.0) * 2.0 ** -kb)
        slack = np.minimum(slack, np.where(kf >= 0, s, np.inf))
    return slack


@pytest.mark.parametrize('kb', [16, 12])
def test_squeeze_is_sound(kb):
    rmax = np.sqrt(-2.0 * np.log(0.5 * 2.0 ** -S.RADIUS_BITS))        # the largest 20-bit Box-Muller radius, ~5.40
    a = np.concatenate([2.0 / 3.0 + np.logspace(-7, 0, 120), np.logspace(np.log10(5.0 / 3.0), 7, 600)])
    x = np.linspace(-rmax, rmax, 2401)
    A, X = np.meshgrid(a, x, indexing='ij')
    slack = _squeeze_slack(X, A, kb)
    fin = np.isfinite(slack)
    assert fin.sum() > 0.5 * slack.size
    print('squeeze KB=%d: min slack %.3g over %d grid points' % (kb, slack[fin].min(), fin.sum()))
    assert slack[fin].min() >= 0.0
    # the actual quads of 1e6 Philox blocks at the policy's shapes (1e3 .. 1e5)
    rs = np.random.RandomState(kb)
    nb = 1_000_000
    w = PR.philox_elem(7, np.arange(nb, dtype=np.uint64), 5, 99, 0)
    slots = (0, 1) if kb == 16 else (2, 3)
    for slot in slots:
        radu, ang, kf, use_sin = S.quad_fields(w, np.full(nb, slot))
        xq, _ = S.box_muller(radu, ang, use_sin)
        aq = 10.0 ** rs.uniform(3, 5, nb)
        top = _sure_threshold_kf(xq, aq, kb, 0)
        sure = kf <= top
        d = aq - 1.0 / 3.0
        E = S.mt_exponent_exact(xq / np.sqrt(9.0 * d), d)
        s = E[sure] - np.log((kf[sure] + 1.0) * 2.0 ** -kb)
        print('squeeze KB=%d slot %d: %d sure of %d, min slack %.3g' % (kb, slot, sure.sum(), nb, s.min()))
        assert sure.mean() > 0.99 and s.min() >= 0.0


# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('a', [0.05, 0.4, 0.999, 1.0, 1.001, 3.0, 100.0, 1.2e4, 1e6])
def test_reference_draws_gamma(a):
    stats = pytest.importorskip('scipy.stats')
    B, d = 25_000, 4                     # one quad per row: slots 0, 1 (16-bit) and 2, 3 (12-bit), 2e5 draws each
    g = S.sample_gamma(0xC0FFEE, 11, np.arange(B, dtype=np.uint64) + np.uint64(2 ** 40), d, np.full((B, d, d), a), 'small',
                       'f64')
    y = g['y_raw']
    for cols, name in (((0, 1), '16-bit'), ((2, 3), '12-bit')):
        v = y[:, :, list(cols)].reshape(-1)
        p = stats.kstest(v, stats.gamma(a).cdf).pvalue
        assert p > 1e-4, (a, name, p)
    path = g['path'].reshape(-1)
    fe = np.mean(path == S.PATH_EXACT)
    fb = np.mean(path == S.PATH_BOOST)
    print('a=%g: exact path %.3g, boost %.3g of the elements; a wave pair (128 elements) takes the exact branch with '
          'probability %.3g' % (a, fe, fb, 1 - (1 - fe) ** 128))
    assert (fb == 1.0) == (a < 1)
    assert g['ambiguous'].mean() < S.MAX_AMBIGUOUS_FRACTION
    if a == 1.2e4:                      # ~1.8 % of the wave pairs at the reference policies
        assert 0.01 < 1 - (1 - fe) ** 128 < 0.03


# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('d', [5, 21])
@pytest.mark.parametrize('first', [6, 7])
def test_tail_carry_is_independent_of_launch_cuts(d, first):
    T, B = 6, 300
    rs = np.random.RandomState(d + first)
    traj = np.arange(B, dtype=np.uint64) + np.uint64(2 ** 32 - 150)
    for s in range(first, first + T):
        sh = 10.0 ** rs.uniform(-1, 4, (B, d, d))
        one = S.sample_gamma(5, s, traj, d, sh, 'small', 'f64', first_step_of_launch=first)
        cut = S.sample_gamma(5, s, traj, d, sh, 'small', 'f64', first_step_of_launch=s)
        for k in ('y', 'path', 'block'):
            assert np.array_equal(one[k], cut[k]), (s, k)
    # the odd step's trailing element is the SINE partner of the even step's pair (slot 1 of the block keyed by step & ~1)
    key, _, tail = S.keying(d, 'small')
    kt = key[tail][0]
    w = PR.philox_elem(5, kt, 8, traj, 0)
    xc = S.box_muller(*S.quad_fields(w, np.zeros(B, int))[:2], np.zeros(B, bool))[0]
    xs = S.box_muller(*S.quad_fields(w, np.ones(B, int))[:2], np.ones(B, bool))[0]
    a = np.full((B, d, d), 1e4)
    for s, x in ((8, xc), (9, xs)):
        g = S.sample_gamma(5, s, traj, d, a, 'small', 'f64')
        dd = 1e4 - 1.0 / 3.0
        hot = g['path'][:, 0, -1] == S.PATH_HOT           # row 0's trailing element (its id is the tail key kt)
        assert hot.mean() > 0.99
        assert np.allclose(g['y'][hot, 0, -1], dd * (1 + x[hot] / np.sqrt(9 * dd)) ** 3, rtol=1e-12)
