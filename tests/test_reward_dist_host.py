"""CPU checks of the reward-distribution diagnostics (mfg_row_distribution, mfg_action_mean_pop, ops.row_distribution /
action_mean_pop / hist_edges, reward_dist.host_jsd, AC_IRL / AC_IRLPopulation.reward_distribution and action_heatmap): the header
and the binding agree, the argument rules raise before the library is called, the restated edge rule is np.histogram's, the
host JSD is the reference's formula, and the public methods have the stated signatures.  No GPU."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('mfg_row_distribution_workspace_bytes', 'mfg_row_distribution', 'mfg_action_mean_pop_workspace_bytes', 'mfg_action_mean_pop')


@pytest.fixture(scope='module')
def lib():
    from discrete_mean_field_game_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib


def _declared_params(name):
    text = open(os.path.join(ROOT, 'include', 'mfg_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    m = re.search(r'\b%s\s*\(([^)]*)\)' % name, text)
    assert m, name
    return [p for p in m.group(1).split(',') if p.strip()]


def test_header_and_signatures_agree(lib):
    for name in NEW:
        assert name in lib.SIGNATURES
        assert len(_declared_params(name)) == len(lib.SIGNATURES[name][1]), name
        assert getattr(lib.lib(), name) is not None


def test_abi_version_unchanged(lib):
    assert lib.lib().mfg_abi_version() == 18


def test_workspace_sizes(lib):
    h = lib.lib()
    assert h.mfg_row_distribution_workspace_bytes(3, 1000, 20, 200) == 0       # LDS only
    assert h.mfg_action_mean_pop_workspace_bytes(0, 10, 15) == 0
    one = h.mfg_action_mean_pop_workspace_bytes(1, 1000, 15)
    assert one == 32 * 225 * 8                                                  # ceil(1000 / 32) chunks of d d doubles
    assert h.mfg_action_mean_pop_workspace_bytes(5, 1000, 15) == 5 * one
    assert h.mfg_action_mean_pop_workspace_bytes(1, 10 ** 6, 15) == 1024 * 225 * 8   # the chunk cap


def test_entry_points_refuse_before_any_launch(lib):
    """Fake device addresses: every call must be refused by the argument checks (no GPU is touched)."""
    h = lib.lib()
    p = 4096

    def dist(R=2, N=10, stride=10, bins=20, use_range=0, lo=0.0, hi=1.0, G=5, x_lo=0.0, x_hi=1.0, values=p, density=p):
        return h.mfg_row_distribution(values, R, N, stride, bins, use_range, lo, hi, G, x_lo, x_hi, p, p, p, density, p, None, 0,
                                      None)
    for kw in (dict(R=0), dict(N=0), dict(N=2 ** 31), dict(stride=9), dict(bins=0), dict(bins=1025), dict(G=-1), dict(G=4097),
               dict(use_range=1, lo=1.0, hi=1.0), dict(use_range=1, lo=0.0, hi=float('inf')), dict(x_lo=float('nan')),
               dict(values=None), dict(density=None)):
        assert dist(**kw) == -1, kw
        assert lib.lib().mfg_last_error()

    def mean(K=2, N=10, d=15, s=2250, action=p, ws=p, nbytes=1 << 30):
        return h.mfg_action_mean_pop(action, s, K, N, d, p, ws, nbytes, None)
    for kw in (dict(K=0), dict(K=65536), dict(N=0), dict(d=0), dict(s=2249), dict(action=None), dict(ws=None)):
        assert mean(**kw) == -1, kw
    assert mean(d=65, s=10 * 65 * 65) == -3
    need = h.mfg_action_mean_pop_workspace_bytes(2, 10, 15)
    assert mean(nbytes=need - 1) == -4


def test_check_row_distribution_args():
    from discrete_mean_field_game_amd import ops
    ok = dict(R=3, N=10, stride=12, bins=20, hist_range=None, G=200, x_lo=-0.1, x_hi=0.4)
    assert ops.check_row_distribution_args(**ok) == (0, 0.0, 0.0)
    assert ops.check_row_distribution_args(**dict(ok, hist_range=(-1, 2))) == (1, -1.0, 2.0)
    assert ops.check_row_distribution_args(**dict(ok, G=0, x_lo=float('nan'))) == (0, 0.0, 0.0)
    for bad in (dict(bins=0), dict(bins=1025), dict(G=-1), dict(G=4097), dict(hist_range=(1.0, 1.0)), dict(hist_range=(2.0, 1.0)),
                dict(hist_range=(0.0, float('inf'))), dict(stride=9), dict(N=0), dict(R=0), dict(x_hi=float('inf')),
                dict(dtype=torch.float64), dict(is_cuda=False)):
        with pytest.raises(ValueError):
            ops.check_row_distribution_args(**dict(ok, **bad))
    # the wrapper refuses a host tensor / a wrong dtype before the library is called
    with pytest.raises(ValueError):
        ops.row_distribution(torch.zeros(2, 8))
    with pytest.raises(ValueError):
        ops.row_distribution(torch.zeros(2, 8, dtype=torch.float64))
    with pytest.raises(ValueError):
        ops.action_mean_pop(torch.zeros(4, 15, 15))


def _cases():
    rs = np.random.RandomState(0)
    for i in range(300):
        n = int(rs.randint(1, 400))
        scale = (1e-3, 0.3, 3.0)[i % 3]
        x = np.tanh(scale * rs.standard_normal(n)).astype(np.float32).astype(np.float64)
        yield x, int(rs.choice([1, 2, 3, 20, 64, 1024]))
    yield np.full(7, 0.25), 20                       # all equal
    yield np.zeros(1), 5
    yield np.array([-1.0, 1.0]), 1024
    yield np.array([1e-30, 3e-30]), 7


def _numpy_rule_counts(x, edges, bins):
    """The index rule of the kernel restated with the restated edges: NumPy's guess, truncated, corrected twice."""
    first, last = edges[0], edges[-1]
    counts = np.zeros(bins, dtype=np.int64)
    for v in x:
        if not first <= v <= last:
            continue
        i = int(((v - first) / (last - first)) * bins)
        i = min(i, bins - 1)
        if v < edges[i]:
            i -= 1
        if i != bins - 1 and v >= edges[i + 1]:
            i += 1
        counts[i] += 1
    return counts


def test_hist_edges_are_numpys():
    from discrete_mean_field_game_amd import ops
    for x, bins in _cases():
        counts, edges = np.histogram(x, bins)
        mine = ops.hist_edges(x.min(), x.max(), bins)
        assert mine.dtype == np.float64 and np.array_equal(mine, edges), (x[:4], bins)
        assert np.array_equal(_numpy_rule_counts(x, mine, bins), counts)
        lo, hi = -0.37, 0.61
        counts, edges = np.histogram(x, bins, range=(lo, hi))
        mine = ops.hist_edges(lo, hi, bins)
        assert np.array_equal(mine, edges)
        assert np.array_equal(_numpy_rule_counts(x, mine, bins), counts)
    # values exactly on the edges
    e = np.linspace(-0.5, 0.75, 21)
    x = np.concatenate([e, e[3:9], e[-1:]])
    counts, edges = np.histogram(x, 20)
    assert np.array_equal(ops.hist_edges(x.min(), x.max(), 20), edges)
    assert np.array_equal(_numpy_rule_counts(x, edges, 20), counts)


def test_host_jsd_is_the_reference_formula():
    from scipy.stats import entropy
    from discrete_mean_field_game_amd.reward_dist import JSD_PAIRS, SETS, host_jsd
    assert SETS == ('demo_train', 'demo_test', 'gen_train', 'gen_test')
    assert JSD_PAIRS == ((0, 1), (0, 2), (1, 3))
    rs = np.random.RandomState(1)
    for _ in range(50):
        p = rs.randint(0, 30, size=20).astype(np.int64)
        q = rs.randint(0, 5, size=20).astype(np.int64)
        p[0] = 1
        q[-1] = 2
        p0, q0 = p.copy(), q.copy()
        got = host_jsd(p, q)
        assert np.array_equal(p, p0) and np.array_equal(q, q0)           # copies: the arguments are not written
        P, Q = p.astype(np.float64), q.astype(np.float64)
        P[P == 0] = 1e-100
        Q[Q == 0] = 1e-100
        M = 0.5 * (P + Q)
        want = 0.5 * (entropy(P, M) + entropy(Q, M))
        assert abs(got - want) <= 1e-14 * max(1.0, abs(want)), (got, want)
    assert host_jsd([3, 0, 1], [3, 0, 1]) == 0.0


def test_public_methods_and_defaults():
    from discrete_mean_field_game_amd.ac_irl import AC_IRL
    from discrete_mean_field_game_amd.irl_population import AC_IRLPopulation
    from discrete_mean_field_game_amd.reward_dist import RewardDistribution
    want = dict(num_bins=20, xmin=-0.1, xmax=0.4, num_points=200, hist_range=None, want_rewards=False)
    for cls, first in ((AC_IRLPopulation, dict(thetas=None, pi0_test=None)), (AC_IRL, dict(theta=None))):
        sig = inspect.signature(cls.reward_distribution)
        params = [p for n, p in sig.parameters.items() if n != 'self']
        assert all(p.kind is inspect.Parameter.KEYWORD_ONLY for p in params)
        assert {p.name: p.default for p in params} == dict(first, **want)
        sig = inspect.signature(cls.action_heatmap)
        params = [p for n, p in sig.parameters.items() if n != 'self']
        assert all(p.kind is inspect.Parameter.KEYWORD_ONLY for p in params)
        assert [p.name for p in params] == [list(first)[0]] and params[0].default is None
    assert [f for f in RewardDistribution.__dataclass_fields__] == ['sets', 'moments', 'counts', 'edges', 'xs', 'density', 'jsd',
                                                                   'status', 'rewards']
    # the optional arguments the two generators gained default to what they did before
    for fn, names in ((AC_IRLPopulation._generate, ('mat_dev', 'theta')), (AC_IRL._generate_device, ('mat_dev', 'theta'))):
        sig = inspect.signature(fn)
        assert all(sig.parameters[n].default is None for n in names)
