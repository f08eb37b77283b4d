"""-m gpu: mfg_row_distribution (ops.row_distribution) against NumPy and SciPy called on the fp64 copy of the same fp32 values:
np.histogram (what plt.hist runs, ac_irl.py:1116-1119) exactly, np.min / max / mean / var within the bounds of the summation
length, scipy.stats.gaussian_kde (ac_irl.py:1087-1100) to rtol 1e-11; non-finite rows, independence of R, refusals."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# (R, N, stride): one value | two | below, at and above the block width of 256 | many tiles and a count past 65535
SHAPES = ((1, 1, 1), (1, 2, 2), (3, 255, 300), (3, 256, 256), (2, 257, 512), (2, 70001, 70001))
BINS = (1, 2, 20, 64, 1024)
SCALES = (1e-3, 0.3, 3.0)
GRIDS = ((-0.1, 0.4), (-5.0, 5.0))          # the reference's grid and a far-tail one
U = 2.0 ** -52


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.fail('-m gpu tests need a GPU')
    return torch.device('cuda:0')


@functools.lru_cache(maxsize=None)
def _values(R, N, scale):
    """tanh of scaled normals as fp32 [R, N] (computed once per shape and scale; never changed)."""
    rs = np.random.RandomState(1000 * R + N % 997 + int(scale * 1e4))
    x = np.tanh(scale * rs.standard_normal((R, N))).astype(np.float32)
    x.setflags(write=False)
    return x


def _padded(x, stride, dev):
    """x [R, N] as a device tensor [R, stride] whose gaps hold NaN: a kernel that ignored the stride would report it."""
    R, N = x.shape
    buf = np.full((R, stride), np.nan, dtype=np.float32)
    buf[:, :N] = x
    return torch.tensor(buf, device=dev)


def _run(x, stride, dev, **kw):
    from discrete_mean_field_game_amd import ops
    out = ops.row_distribution(_padded(x, stride, dev), N=x.shape[1], **kw)
    torch.cuda.synchronize()
    return {k: (None if v is None else v.cpu().numpy()) for k, v in out.items()}


def _check_hist(got, x, bins, rng=None):
    for r in range(x.shape[0]):
        x64 = x[r].astype(np.float64)
        counts, edges = np.histogram(x64, bins, range=rng)
        assert got['counts'].dtype == np.int64
        assert np.array_equal(got['edges'][r], edges), (r, bins)
        assert np.array_equal(got['counts'][r], counts), (r, bins, got['counts'][r], counts)
        assert got['moments'][r, 0] == counts.sum()


def _check_moments(got, x):
    R, N = x.shape
    for r in range(R):
        x64 = x[r].astype(np.float64)
        m = got['moments'][r]
        assert m[1] == x64.min() and m[2] == x64.max()
        assert abs(m[3] - np.mean(x64)) <= N * U * np.abs(x64).max()
        if N >= 2:
            var = np.var(x64, ddof=1)
            assert abs(m[4] - var) <= 4 * N * U * var
            assert abs(m[5] - var * float(N) ** -0.4) <= (4 * N + 8) * U * var * float(N) ** -0.4
        else:
            assert np.isnan(m[4]) and np.isnan(m[5])


@pytest.mark.parametrize('scale', SCALES)
@pytest.mark.parametrize('shape', SHAPES)
def test_histogram_and_moments_are_numpys(dev, shape, scale):
    R, N, stride = shape
    x = _values(R, N, scale)
    for bins in BINS:
        got = _run(x, stride, dev, bins=bins)
        _check_hist(got, x, bins)
        _check_moments(got, x)
        want = 2 if N < 2 else 0
        assert np.array_equal(got['status'], np.full(R, want, dtype=np.int32))
        assert got['density'] is None


def test_histogram_all_equal_row_and_values_on_the_edges(dev):
    same = np.full((1, 300), 0.25, dtype=np.float32)
    for bins in BINS:
        got = _run(same, 300, dev, bins=bins, G=4, x_lo=0.0, x_hi=1.0)
        _check_hist(got, same, bins)
        assert got['edges'][0, 0] == -0.25 and got['edges'][0, -1] == 0.75
        assert got['moments'][0, 4] == 0.0 and got['status'][0] == 2 and np.isnan(got['density']).all()
    for bins in (2, 20, 64):
        e = np.linspace(-0.5, 0.75, bins + 1).astype(np.float32)       # steps of 1.25 / bins: exact in fp32
        assert np.array_equal(e.astype(np.float64), np.linspace(-0.5, 0.75, bins + 1))
        on = np.concatenate([e, e[1:bins // 2 + 1], e[-1:], e[:1]])[None]
        got = _run(on, on.shape[1] + 3, dev, bins=bins)
        _check_hist(got, on, bins)


def test_histogram_common_range(dev):
    lo, hi = -0.25, 0.5                       # both fp32 numbers
    x = _values(3, 255, 0.3).copy()
    x[:, :4] = (lo, hi, np.nextafter(np.float32(lo), np.float32(-1)), np.nextafter(np.float32(hi), np.float32(1)))
    assert (x < lo).any() and (x > hi).any()
    for bins in BINS:
        got = _run(x, 300, dev, bins=bins, hist_range=(lo, hi))
        _check_hist(got, x, bins, rng=(lo, hi))
        assert (got['moments'][:, 0] < 255).all()
        _check_moments(got, x)                # mean and variance over all N values: the range touches the histogram alone
    outside = _run(x, 300, dev, bins=20, hist_range=(2.0, 3.0))
    assert not outside['counts'].any() and not outside['moments'][:, 0].any()


@pytest.mark.parametrize('scale', SCALES)
@pytest.mark.parametrize('shape', ((1, 2, 2), (3, 255, 300), (3, 256, 256), (2, 257, 512), (2, 70001, 70001)))
def test_kde_is_scipys(dev, shape, scale):
    from scipy.stats import gaussian_kde
    R, N, stride = shape
    x = _values(R, N, scale)
    for x_lo, x_hi in GRIDS:
        for G in (1, 200):
            got = _run(x, stride, dev, bins=20, G=G, x_lo=x_lo, x_hi=x_hi)
            grid = np.linspace(x_lo, x_hi, G)
            for r in range(R):
                kde = gaussian_kde(x[r].astype(np.float64))
                want = kde(grid)
                np.testing.assert_allclose(got['density'][r], want, rtol=1e-11, atol=1e-300)
                cov = float(kde.covariance[0, 0])
                assert abs(got['moments'][r, 5] - cov) <= (4 * N + 8) * U * cov
            assert not got['status'].any()
    if scale == 0.3:                          # something to compare: the density of the last grid is not all zeros
        assert (got['density'] > 0).any()


def test_kde_undefined(dev):
    one = _run(_values(1, 1, 0.3), 1, dev, bins=5, G=7, x_lo=-1.0, x_hi=1.0)
    assert one['status'][0] == 2 and np.isnan(one['density']).all() and one['counts'].sum() == 1
    same = _run(np.full((2, 40), -0.5, dtype=np.float32), 40, dev, bins=5, G=200, x_lo=-1.0, x_hi=1.0)
    assert np.array_equal(same['status'], [2, 2]) and np.isnan(same['density']).all()
    assert np.array_equal(same['moments'][:, 1:5], [[-0.5, -0.5, -0.5, 0.0]] * 2)


@pytest.mark.parametrize('poison', (np.nan, np.inf, -np.inf))
def test_non_finite_row_leaves_the_others_alone(dev, poison):
    x = _values(3, 257, 0.3).copy()
    x[1, 200] = poison
    kw = dict(bins=20, G=50, x_lo=-0.5, x_hi=0.5)
    got = _run(x, 300, dev, **kw)
    assert np.array_equal(got['status'], [0, 1, 0])
    assert np.isnan(got['moments'][1]).all() and np.isnan(got['edges'][1]).all() and np.isnan(got['density'][1]).all()
    assert not got['counts'][1].any()
    clean = _run(x[[0, 2]], 300, dev, **kw)
    for name in ('moments', 'counts', 'edges', 'density', 'status'):
        assert np.array_equal(got[name][[0, 2]], clean[name]), name


def test_rows_do_not_depend_on_R(dev):
    for N, stride in ((257, 512), (70001, 70001)):
        x = _values(3, N, 0.3)
        kw = dict(bins=64, G=20, x_lo=-0.1, x_hi=0.4, hist_range=(-0.5, 0.7))
        got = _run(x, stride, dev, **kw)
        for r in range(3):
            alone = _run(x[r:r + 1], stride, dev, **kw)
            for name in ('moments', 'counts', 'edges', 'density', 'status'):
                assert np.array_equal(got[name][r:r + 1], alone[name]), (N, r, name)


def test_refusals_write_nothing(dev):
    """Bad arguments through the binding with real device buffers that hold a sentinel: MfgError, and nothing is written.  (The
    call needs no workspace -- mfg_row_distribution_workspace_bytes is 0 -- so there is no short one to hand it; the
    short-workspace refusal of this family is checked on mfg_action_mean_pop in test_gpu_action_mean.py.)"""
    from discrete_mean_field_game_amd import _lib as L
    R, N, bins, G = 2, 100, 20, 10
    v = _padded(_values(R, N, 0.3), N, dev)
    bufs = {'moments': torch.full((R, 6), -7.0, dtype=torch.float64, device=dev),
            'counts': torch.full((R, bins), -7, dtype=torch.int64, device=dev),
            'edges': torch.full((R, bins + 1), -7.0, dtype=torch.float64, device=dev),
            'density': torch.full((R, G), -7.0, dtype=torch.float64, device=dev),
            'status': torch.full((R,), -7, dtype=torch.int32, device=dev)}

    def call(**kw):
        a = dict(R=R, N=N, stride=N, bins=bins, use_range=0, lo=0.0, hi=1.0, G=G, x_lo=0.0, x_hi=1.0)
        a.update(kw)
        rc = L.lib().mfg_row_distribution(v.data_ptr(), a['R'], a['N'], a['stride'], a['bins'], a['use_range'], a['lo'], a['hi'],
                                          a['G'], a['x_lo'], a['x_hi'], bufs['moments'].data_ptr(), bufs['counts'].data_ptr(),
                                          bufs['edges'].data_ptr(), bufs['density'].data_ptr(), bufs['status'].data_ptr(), None, 0,
                                          torch.cuda.current_stream().cuda_stream)
        L.check(rc, 'mfg_row_distribution')
    assert L.lib().mfg_row_distribution_workspace_bytes(R, N, bins, G) == 0
    for kw in (dict(bins=0), dict(bins=1025), dict(G=4097), dict(stride=N - 1), dict(use_range=1, lo=1.0, hi=0.0), dict(R=0),
               dict(N=0), dict(x_hi=float('nan'))):
        with pytest.raises(L.MfgError) as e:
            call(**kw)
        assert e.value.code == -1, kw
    torch.cuda.synchronize()
    for name, t in bufs.items():
        assert bool((t == -7).all()), name
    call()                                     # ... and the same buffers are filled by a good call
    torch.cuda.synchronize()
    assert not bool((bufs['status'] == -7).any()) and not bool((bufs['density'] == -7.0).any())
