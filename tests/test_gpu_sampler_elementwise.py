"""-m gpu: the in-kernel Dirichlet sampler element by element against oracle/sampler_ref.py.

Every element of P is compared with the NumPy restatement drawn from the same Philox words: the keying, the bit fields and the
accept / reject story are exact, the value agrees within the restatement's fp32-derived bound, and only near-tie decisions
(`ambiguous`, capped at 2e-5 of the elements of every case) may differ.  Rows that hold an ambiguous element are excluded from
the value check (sampler_ref.compare).  Every case prints its worst err / bound and its ambiguous count.

Grid: every small-d tail length and large-d lane layout (R = 2 .. 8, ragged last column, odd row count, odd R), both
precisions, four shape regimes (the reference policy, shapes 1-100, all shapes < 1, shapes straddling 1/3, 2/3 and 1), steps
0 / odd / 0xFFFFFFFE / 0xFFFFFFFF, trajectory ids from 0, across 2^32 and near 2^47; both lane mappings at d = 15 and 21; fused
rollouts that take the in-launch even-to-odd carry of a row's single trailing element.
"""
import numpy as np
import pytest

torch = pytest.importorskip('torch')

pytestmark = pytest.mark.gpu

D_SMALL = [3, 4, 5, 6, 7, 15, 21, 47, 64]
D_LARGE = [65, 100, 128, 129, 192, 193, 256, 320, 448, 449, 512]
BIG = {15, 21, 128, 256}           # >= 1e6 elements per case there, >= 2.5e5 elsewhere
REGIMES = ['policy', 'mid', 'small', 'straddle']
STEPS = [0, 7, 0xFFFFFFFE, 0xFFFFFFFF]


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.fail('-m gpu tests need a GPU: the HIP path has no CPU fallback')
    from discrete_mean_field_game_amd import ops
    ops.init()
    return torch.device('cuda:0')


@pytest.fixture(autouse=True)
def _auto_mapping():
    yield
    from discrete_mean_field_game_amd import _lib as L
    L.lib().mfg_set_core_mapping(0)


def _ops():
    from discrete_mean_field_game_amd import ops
    return ops


def _ref():
    from oracle import sampler_ref
    return sampler_ref


from oracle.score_ref import regime_case  # noqa: E402  (shared with tests/test_gpu_score_regimes.py)


def _batch(d, big=False):
    n = 1_000_000 if big else 250_000
    return max(1, -(-n // (d * d)))


def _cases():
    out = []
    for k, d in enumerate(D_SMALL + D_LARGE):
        reg = REGIMES[k % 4]
        for p, precision in enumerate(('f64', 'mixed')):
            step = STEPS[(k + p) % 4]
            out.append(pytest.param(d, precision, reg, step, (k + 2 * p) % 3, k, id='d%d-%s-%s-s%x' % (d, precision, reg, step)))
    return out


def _offset(kind, B):
    return [0, 2 ** 32 - B // 2, 2 ** 47 + 12345][kind]


def _report(tag, r):
    print('[sampler] %s: worst err/bound %.3g, ambiguous %d of %d, rows excluded %d, paths hot/exact/boost %s' % (
        tag, r['worst'], r['ambiguous'], r['n'], r['rows_excluded'], r['paths']))


@pytest.mark.parametrize('d,precision,regime,step,offk,k', _cases())
def test_sample_dirichlet_elementwise(dev, d, precision, regime, step, offk, k):
    B = _batch(d, d in BIG)
    rs = np.random.RandomState(1000 * d + k)
    pi, theta, shift, scale = regime_case(regime, B, d, rs, k, 1e-6 if precision == 'f64' else 0.1)
    off = _offset(offk, B)
    seed = 0x5EED0000 + d
    th = torch.tensor([theta], dtype=torch.float64, device=dev)
    P = _ops().sample_dirichlet(torch.as_tensor(pi, device=dev), th, shift, scale, seed=seed, step=step, traj_offset=off,
                                precision=precision)
    r = _ref().compare(P.cpu().numpy(), pi, theta, shift, scale, seed, step, off, precision)
    _report('d=%d %s %s step=%#x traj_offset=%#x' % (d, precision, regime, step, off), r)
    if regime == 'small':
        assert r['paths'][2] == r['n']
    if regime == 'policy':
        assert r['paths'][0] > 0.99 * r['n']


@pytest.mark.parametrize('d', [15, 21])
@pytest.mark.parametrize('mode', [1, 2])
@pytest.mark.parametrize('regime', ['policy', 'small'])
def test_both_lane_mappings_against_the_reference(dev, d, mode, regime):
    """mfg_set_core_mapping forces the packed kernel (1) or k_core_row3 (2): each is compared with the reference."""
    from discrete_mean_field_game_amd import _lib as L
    B = _batch(d, True)
    rs = np.random.RandomState(77 + d + mode)
    pi, theta, shift, scale = regime_case(regime, B, d, rs)
    th = torch.tensor([theta], dtype=torch.float64, device=dev)
    for step in (6, 7):
        L.lib().mfg_set_core_mapping(mode)
        P = _ops().sample_dirichlet(torch.as_tensor(pi, device=dev), th, shift, scale, seed=321, step=step,
                                    traj_offset=2 ** 32 - B // 2, precision='mixed')
        L.lib().mfg_set_core_mapping(0)
        r = _ref().compare(P.cpu().numpy(), pi, theta, shift, scale, 321, step, 2 ** 32 - B // 2, 'mixed')
        _report('d=%d mapping %d %s step=%d' % (d, mode, regime, step), r)


@pytest.mark.parametrize('d', [5, 21, 15, 129])
@pytest.mark.parametrize('T', [4, 5])
@pytest.mark.parametrize('first_step', [10, 11])
@pytest.mark.parametrize('precision', ['mixed', 'f64'])
def test_rollout_steps_against_the_reference(dev, d, T, first_step, precision):
    """Each step's P of a fused rollout against the reference at the device's own state of that step: a launch that starts on
    an even step carries the trailing element's Box-Muller partner into the odd step behind it, one that starts on an odd
    step recomputes it.  The cap on ambiguous elements applies to the whole rollout (T B d^2 >= 2.8e5 elements)."""
    B = max(1, 70_000 // (d * d))
    rs = np.random.RandomState(d * 10 + T + first_step)
    pi0 = rs.dirichlet(np.ones(d), size=B).astype(np.float32)
    theta, shift, scale = 8.86349, 0.16, 12000.0
    seed, off = 4242, 2 ** 32 - B // 2
    out = _ops().rollout(torch.as_tensor(pi0, device=dev), T, torch.tensor([theta], dtype=torch.float64, device=dev), shift,
                         scale, seed=seed, first_step=first_step, traj_offset=off, td=False, write_P=True, precision=precision)
    r = _ref().compare_rollout(out['P'].cpu().numpy(), out['pi_traj'].cpu().numpy(), theta, shift, scale, seed, first_step,
                               np.uint64(off) + np.arange(B, dtype=np.uint64), precision)
    _report('rollout d=%d T=%d first_step=%d %s' % (d, T, first_step, precision), r)


def test_trajectory_ids_past_2_48_are_rejected(dev):
    """The Philox counter keeps 48 bits of the trajectory id: traj_offset + B > 2^48 would silently draw other trajectories'
    actions, so every entry point that takes traj_offset rejects it (MFG_EINVAL, include/mfg_hip.h MFG_TRAJ_ID_LIMIT)."""
    from discrete_mean_field_game_amd import _lib as L
    ops = _ops()
    d, B = 21, 8
    pi = torch.as_tensor(np.random.RandomState(1).dirichlet(np.ones(d), size=B).astype(np.float32), device=dev)
    th = torch.tensor([8.86349], dtype=torch.float64, device=dev)
    lim = 2 ** 48
    P = ops.sample_dirichlet(pi, th, 0.16, 12000.0, seed=3, step=1, traj_offset=lim - B)      # the last ids: accepted
    r = _ref().compare(P.cpu().numpy(), pi.cpu().numpy(), 8.86349, 0.16, 12000.0, 3, 1, lim - B, 'mixed')
    assert r['n'] == B * d * d
    calls = [lambda off: ops.sample_dirichlet(pi, th, 0.16, 12000.0, seed=3, step=1, traj_offset=off),
             lambda off: ops.rollout(pi, 2, th, 0.16, 12000.0, seed=3, traj_offset=off, td=False),
             lambda off: ops.draw_start(pi, B, 3, 0, traj_offset=off)]
    for call in calls:
        for off in (lim - B + 1, lim, 2 ** 64 - 1):
            with pytest.raises(L.MfgError) as e:
                call(off)
            assert e.value.code == -1          # MFG_EINVAL
        call(lim - B)
    torch.cuda.synchronize()
