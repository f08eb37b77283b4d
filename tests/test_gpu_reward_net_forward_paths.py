"""The reward network's forward kernels OFF the matrix-core path (csrc/mfg_reward_net.hip: k_reward_net_runs and k_reward_net<PP,
...> with compile-time and with run-time conv geometry), case by case of oracle/reward_forward_cases.py, whose CPU admission rule
is tests/test_reward_forward_cases.py.  One parametrised test per family; each case prints one line (-s) with its worst ratio
|deviation| / tolerance.

a. Per sample against the fp64 oracle (RO.forward_cache): within 1e-5 max(|r_ref|, m), m = |h4| . |out_w| + |out_b| -- the
   layer-1 bound of tests/test_gpu_reward_train_shapes.py --, and at gain 1 / concentration 1 also within the absolute bounds of
   the existing forward tests (2e-6, with dropout 5e-6).  Dropout off, and for the dropout networks on, with the oracle's masks
   redrawn from the documented Philox counters; seed and sample offset lie above 2^32 outside the regime family.
b. Staged = unstaged, bit for bit: a sample's reward must not depend on the batch it travels in.  A launch copies the FC3
   weights into LDS from MFG_RN_LDS_MIN = 16 samples per block; the grid is capped at 256 MFG_RN_BPC = 512 blocks of
   MFG_RN_WAVES = 8 waves, so from B = 7 681 (FC.STAGE_B).  IF THOSE DEFAULTS CHANGE THIS TEST SILENTLY STOPS REACHING THE STAGED
   PATH.  Every staged case is evaluated again in slices of 4 099 samples (<= 7 680: unstaged; odd: a sample meets another wave
   and block), each slice from its own contiguous copy with the sample offset advanced by its start, and compared with
   np.array_equal -- both branches of the FC3 loop run the same fmaf chain.  The n3 = 19 control (67 032 B of weights: never
   staged) satisfies the same equality.
c. The LDS corner: the staged launches are the family's largest dynamic-LDS requests (FC.lds_bytes restates the host formulas):
   run-mapped d = 21, n3 = 18, n4 = 32: 107 232 B; d = 32 at (5, 2, 3), n3 = 8, n4 = 32: 149 600 B; d = 32 at (7, 2, 7), n3 = 8,
   n4 = 4: 159 264 B; the same with n4 = 32: 163 968 B, 128 B more than the 160 KB of a CU.  Outcome: see MEASURED below.
d. state_T > 0: mfg_train_rollout_irl hands the launch the rollout's pi_traj [B, T + 1, d] and the key and sample offset it was
   given, unchanged (train_rollout_impl: reward_net_forward_sums(pi_traj, P, B T, ..., ext->key, ext->sample_offset, ...,
   state_T = T)); its rewards equal reward_net_forward on the gathered states, bit for bit, and the oracle under criterion a.

MEASURED on an MI355X (a ratio is deviation / tolerance, 1 = at the bound; the 83 tests take 5 s).  Worst ratio per family,
dropout off / on:
  generic (run-time geometry) 0.101 / 0.102   ref (pixel-per-lane at (5, 2, 3), fc3 offsets) 0.050 / 0.104
  runs 0.095 / 0.325   staged 0.063 / 0.673 (run-mapped d = 15, n3 = 17, B = 7 681)   regime 0.297 / 0.324
(figures of the run before the last fifteen reseedings of the table; those cases passed at their earlier seeds as listed)
and per gain over the four kernels' regime shapes: 1e-3 0.010 / 0.008, 1 0.060 / 0.109, 8 0.287 / 0.324, 30 0.297 / 0.244; rollout
states in place 0.058 (d = 21, n3 = 24) and 0.031 (d = 12).  Every staged launch equals its slices bit for bit.
One ratio above 1 was met on the way and was the table's, not a kernel's: regime-ct-d15-gain8-conc1 at network seed 0 gave 0.040
with dropout off and 4.33 under its masks -- and networks.RewardNet in fp32 on the CPU, under the SAME masks, 1.37: a mask had left
a sample whose FC4 inputs cancel, which the tolerance's scale m does not see.  The admission rule now evaluates a dropout case
under its masks too, with a bit-reproducible fp32 evaluation (oracle/reward_forward_cases.py); fifteen cases left seed 0.
LDS corner, outcome: the launches of 107 232, 149 600 and 159 264 B run as they are -- this runtime wants no attribute for dynamic
LDS between 64 KB and the CU's 160 KB -- and satisfy a and b.  The 163 968 B launch came back as MFG_ELAUNCH ("reward_net: launch
failed", one call, not repeated): reward_net_forward_sums staged the FC3 weights whenever THEY fit 64 KB, whatever the tiles
took.  Fixed in the host rule: stage only when the launch's whole request fits 160 KB; that shape now runs unstaged (98 432 B).
Mutation check (scratch builds, in-bounds changes, nothing committed), each against this file and against the 38 existing
test_reward_net_hip_* cases of tests/test_gpu_classes.py, which stayed green under all four:
  * run-time geometry, conv1 tap `sc1[dy * k1 + dx]` -> `sc1[dx * k1 + dy]` (K1 == 0 only): 19 cases fail (every generic-rt case
    with k1 > 1 whose FC3 units are alive; d = 1 sees the centre tap alone);
  * run-mapped kernel, scalar tail of the staged copy dropped: both 17 x 450 staged cases and the 7 800-transition rollout fail;
  * pixel-per-lane kernel, the staged float4 copy stores the neighbouring piece: the six staged generic cases fail;
  * run-mapped kernel, the prefetched state row ignores state_T: the 7 800-transition rollout fails (at 200 transitions every
    wave has one sample and never prefetches).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import reward_forward_cases as FC
from oracle import reward_net_oracle as RO

SLICE = 4099


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    return torch.device('cuda:0')


def _forward(case, net, s_t, a_t, dropout, lo=0):
    from discrete_mean_field_game_amd import ops
    seed, off = FC.dropout_key(case)
    return ops.reward_net_forward(net, s_t, a_t, dropout=dropout, seed=seed, sample_offset=off + lo).cpu().numpy()


def _modes(case):
    return (False, True) if 'dropout' in case.reg else (False,)


def _check(case, dev, sliced=False):
    """Criterion a for every mode of the case (and b when `sliced`); returns {dropout: worst ratio}."""
    from discrete_mean_field_game_amd import ops
    net, state, action = FC.build(case, dev)
    assert ops.reward_net_supported(net)
    s_t, a_t = torch.as_tensor(state, device=dev), torch.as_tensor(action, device=dev)
    idx = FC.oracle_indices(case)
    out = {}
    for dropout in _modes(case):
        got = _forward(case, net, s_t, a_t, dropout)
        assert got.shape == (case.B,) and np.isfinite(got).all() and np.abs(got).max() <= 1.0
        ref, tol = FC.oracle(case, net, state, action, idx, dropout)
        out[dropout] = FC.ratio(got[idx].astype(np.float64) - ref, tol)
        if sliced:
            parts = [_forward(case, net, s_t[lo:lo + SLICE].clone(), a_t[lo:lo + SLICE].clone(), dropout, lo)
                     for lo in range(0, case.B, SLICE)]
            out['equal', dropout] = bool(np.array_equal(np.concatenate(parts), got))
    print('\n%-52s %-10s B %4d  LDS %6d B%s  ratio %s' % (
        case.name, FC.kernel_of(case), case.B, FC.lds_bytes(case, FC.stages(case)) if FC.kernel_of(case) != 'mfma' else 0,
        ' (staged)' if FC.stages(case) else '', '  '.join('%s %.3f' % ('dropout' if k else 'plain', v) for k, v in out.items()
                                                          if isinstance(k, bool))))
    return out


def _assert_a(out):
    for dropout, q in out.items():
        if isinstance(dropout, bool):
            assert q <= 1.0, ('against the oracle', 'dropout' if dropout else 'plain', q)


def _ids(family):
    return dict(argvalues=FC.by_family(family), ids=[c.name for c in FC.by_family(family)])


@pytest.mark.parametrize('case', **_ids('generic'))
def test_forward_paths_run_time_geometry(dev, case):
    assert FC.kernel_of(case) == 'generic-rt'
    _assert_a(_check(case, dev))


@pytest.mark.parametrize('case', **_ids('ref'))
def test_forward_paths_reference_geometry_pixel_per_lane(dev, case):
    _assert_a(_check(case, dev))


@pytest.mark.parametrize('case', **_ids('runs'))
def test_forward_paths_run_mapped(dev, case):
    assert FC.kernel_of(case) == 'runs'
    _assert_a(_check(case, dev))


@pytest.mark.parametrize('case', **_ids('regime'))
def test_forward_paths_reward_regimes(dev, case):
    _assert_a(_check(case, dev))


@pytest.mark.parametrize('case', **_ids('staged'))
def test_forward_paths_staged_equals_unstaged(dev, case):
    """Criteria a, b and c: a launch that stages the FC3 weights in LDS (or, for the control and the 163 968 B corner, is big
    enough to but must not) returns -- no MFG_ELAUNCH --, matches the oracle and equals its unstaged slices bit for bit."""
    assert case.B >= FC.STAGE_B and not FC.stages(case, SLICE)
    out = _check(case, dev, sliced=True)
    _assert_a(out)
    for dropout in _modes(case):
        assert out['equal', dropout], ('one launch differs from its slices', 'dropout' if dropout else 'plain')


@pytest.mark.parametrize('d,n3,B,T', [(21, 24, 40, 5), (12, 8, 40, 3), (15, 17, 520, 15)])
def test_forward_paths_rollout_states_in_place(dev, d, n3, B, T):
    """Criterion d: run-mapped, pixel-per-lane and (7 800 transitions) staged run-mapped launches over a rollout's pi_traj."""
    from discrete_mean_field_game_amd import ops
    from oracle.reward_train_cases import _net
    ops.init()
    rs = np.random.RandomState(100 * d + T)
    net = _net(d, 'dropout_l1l2', n3, 4, dev)
    mat = torch.as_tensor(rs.dirichlet(np.ones(d), size=11).astype(np.float32), device=dev)
    F = ops.num_features(d)
    th = torch.tensor([8.64], dtype=torch.float64, device=dev)
    w = torch.as_tensor(rs.rand(F) * 0.1, device=dev)
    G = torch.zeros(F + 3, dtype=torch.float64, device=dev)
    N = B * T
    ws = ops.workspace(N, d, dev)
    bufs = {'pi_traj': torch.empty(B, T + 1, d, dtype=torch.float32, device=dev),
            'pi_last': torch.empty(B, d, dtype=torch.float32, device=dev),
            'P': torch.empty(B, T, d, d, dtype=torch.float32, device=dev),
            'reward': torch.full((N,), float('nan'), dtype=torch.float32, device=dev),
            'delta': torch.empty(B, T, dtype=torch.float64, device=dev),
            'g': torch.empty(B, T, dtype=torch.float64, device=dev)}
    key, off = 0x9E3779B97F4A7C15 ^ d, (1 << 33) + 977 * T
    ops.train_rollout_irl(mat, None, T, th, 0.1, 1e4, w, 0.95, 0.1, 0.001, net, G, ws, bufs, seed=7, first_step=40, traj_offset=5,
                          rn_key=key, rn_sample_offset=off, apply=False)
    torch.cuda.synchronize()
    assert float(th[0]) == 8.64
    states = bufs['pi_traj'][:, :T].reshape(-1, d).contiguous()
    actions = bufs['P'].reshape(-1, d, d)
    again = ops.reward_net_forward(net, states, actions, seed=key, sample_offset=off)
    got = bufs['reward'].cpu().numpy()
    assert np.isfinite(got).all() and np.array_equal(got, again.cpu().numpy())
    assert not torch.equal(states[:B * T - 1], bufs['pi_traj'].reshape(-1, d)[:B * T - 1])      # (the row map is no identity)
    if N < FC.STAGE_B:
        prm = RO.params_from_torch(net)
        masks = RO.dropout_masks(net.keep_prob, key, off, N, n3, 4)
        ref, cache = RO.forward_cache(prm, states.cpu().numpy().astype(np.float64), actions.cpu().numpy().astype(np.float64), masks)
        m = np.abs(cache['h4']).dot(np.abs(prm['out_w'])) + np.abs(prm['out_b'])
        q = FC.ratio(got.astype(np.float64) - ref[:, 0], FC.TOL_REL * np.maximum(np.abs(ref), m)[:, 0])
        print('\nrollout states in place d %d n3 %d B %d T %d: ratio %.3f' % (d, n3, B, T, q))
        assert q <= 1.0
