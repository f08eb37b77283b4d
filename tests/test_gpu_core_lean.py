"""-m gpu: the training call's instantiation of the packed rollout kernel gives the SAME BITS as the general one.

A mixed-precision training rollout at d = 21 / 15 that asks for nothing optional -- the in-kernel mfg_ac2 reward, pi_traj / reward /
delta / g all present, no actions written out, a constant bootstrap factor -- runs `k_core_small_lean` (csrc/mfg_core.h): the
packed kernel's body with those options compiled out.  Every other launch takes `k_core_small` as before.  Which one runs must
never show in the results.  `mfg_set_core_mapping` (include/mfg_hip.h) is the hook: mode 1 is "packed" (the specialised
instantiation where the launch allows it), mode 3 "packed, general instantiation"; every output is compared with array_equal.

Shapes: a tile holds 12 trajectories at d = 21 (16 at d = 15), a wavefront 3 (4).  B = 1 is a partial wave, 11 a partial tile,
13 one past a tile, 25 two tiles + 1.  T = 2 / 3 from an even and an odd first step walk the carried Box-Muller pair of the row's
trailing element (d = 21) through have / have-not on both parities.
"""
import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

THETA, SHIFT, SCALE, GAMMA = 8.86349, 0.16, 12000.0, 0.9
BATCHES = (1, 11, 13, 25)


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.fail('-m gpu tests need a GPU')
    from discrete_mean_field_game_amd import ops
    ops.init()
    return torch.device('cuda', 0)


@pytest.fixture(autouse=True)
def _auto_mapping():
    yield
    from discrete_mean_field_game_amd import _lib as L
    L.lib().mfg_set_core_mapping(0)


def _both(fn):
    """fn() under mode 1 (packed: the specialised instantiation where the launch allows it) and mode 3 (packed, general)."""
    from discrete_mean_field_game_amd import _lib as L
    out = []
    for mode in (1, 3):
        L.lib().mfg_set_core_mapping(mode)
        out.append(fn())
    L.lib().mfg_set_core_mapping(0)
    return out


def _same(a, b, keys):
    for k in keys:
        x, y = a[k], b[k]
        if x is None and y is None:
            continue
        assert np.array_equal(x.cpu().numpy(), y.cpu().numpy()), 'output %r differs between the instantiations (max |diff| %g)' % (
            k, float((x.double() - y.double()).abs().max()))


def _inputs(dev, d, B, seed=0):
    from discrete_mean_field_game_amd import ops
    rs = np.random.RandomState(100 * d + B + seed)
    pi0 = torch.as_tensor(rs.dirichlet(np.ones(d), size=B).astype(np.float32), device=dev)
    th = torch.tensor([THETA], dtype=torch.float64, device=dev)
    w = torch.as_tensor(rs.rand(ops.num_features(d)), device=dev)
    return pi0, th, w


def _train_bufs(dev, d, B, T):
    # (NaN-filled: an output the kernel did not write cannot pass for one it did)
    return {'pi_traj': torch.full((B, T + 1, d), float('nan'), device=dev), 'pi_last': torch.full((B, d), float('nan'), device=dev),
            'reward': torch.full((B, T), float('nan'), device=dev),
            'delta': torch.full((B, T), float('nan'), dtype=torch.float64, device=dev),
            'g': torch.full((B, T), float('nan'), dtype=torch.float64, device=dev)}


@pytest.mark.parametrize('start', ['given', 'gathered', 'drawn'])
@pytest.mark.parametrize('T,first_step', [(2, 0), (2, 1), (3, 4), (3, 7)])
@pytest.mark.parametrize('d', [21, 15])
def test_training_rollout_is_bit_identical_in_both_instantiations(dev, d, T, first_step, start):
    """The launch the specialised kernel exists for, over the batch sizes around a wave and a tile: start rows given as states
    (mfg_rollout), gathered through indices and drawn in the kernel (mfg_train_rollout); with and without the final-state output."""
    from discrete_mean_field_game_amd import ops
    F = ops.num_features(d)
    for B in BATCHES:
        pi0, th, w = _inputs(dev, d, B)
        if start == 'given':
            def run():
                return ops.rollout(pi0, T, th, SHIFT, SCALE, w=w, gamma=GAMMA, seed=99, first_step=first_step,
                                   traj_offset=12345678901, td=True)
            keys = ['pi_traj', 'pi_last', 'reward', 'delta', 'g', 'G']
        else:
            rs = np.random.RandomState(B)
            mat = torch.as_tensor(rs.dirichlet(np.ones(d), size=7).astype(np.float32), device=dev)
            idx = torch.as_tensor(rs.randint(7, size=B).astype(np.int32), device=dev) if start == 'gathered' else None

            def run():
                bufs = _train_bufs(dev, d, B, T)
                if B == 13:
                    bufs['pi_last'] = None      # (pi_next_out stays a run-time option of the specialised kernel)
                G = torch.zeros(F + 3, dtype=torch.float64, device=dev)
                ops.train_rollout(mat, idx, T, th, SHIFT, SCALE, w, GAMMA, G, ops.workspace(B * T, d, dev), bufs, seed=99,
                                  first_step=first_step, traj_offset=77)
                return dict(bufs, G=G)
            keys = ['pi_traj', 'pi_last', 'reward', 'delta', 'g', 'G']
        a, b = _both(run)
        _same(a, b, keys)
        for k in ('pi_traj', 'reward', 'delta', 'g'):
            assert torch.isfinite(a[k]).all(), '%s was not written completely (B = %d)' % (k, B)


@pytest.mark.parametrize('d', [21, 15])
def test_deferred_update_chain_in_both_instantiations(dev, d):
    """mfg_train_rollout_deferred, two chained episodes: the second applies the first one's update while it stages its weights
    and block 0 publishes the new parameters -- the deferred update stays a run-time option of the specialised kernel."""
    from discrete_mean_field_game_amd import ops
    B, T = 25, 3
    rs = np.random.RandomState(2)
    mat = torch.as_tensor(rs.dirichlet(np.ones(d), size=9).astype(np.float32), device=dev)
    F = ops.num_features(d)

    def run():
        theta = torch.tensor([THETA], dtype=torch.float64, device=dev)
        w = torch.as_tensor(np.random.RandomState(1).rand(F), device=dev)
        ta, wa = torch.empty_like(theta), torch.empty_like(w)
        G = torch.zeros(F + 3, dtype=torch.float64, device=dev)
        ws = ops.workspace(B * T, d, dev)
        bufs = _train_bufs(dev, d, B, T)
        racc = torch.zeros(4, dtype=torch.float64, device=dev)
        pending = None
        snaps = []
        for ep in range(2):
            ops.train_rollout_deferred(mat, None, T, theta, w, pending, ta, wa, SHIFT, SCALE, GAMMA, G, ws, bufs, seed=8,
                                       first_step=ep * T, traj_offset=77)
            if pending is not None:
                theta, ta = ta, theta
                w, wa = wa, w
            pending = (G, 0.1 / (ep + 1), 0.001 / (ep + 1), racc.data_ptr() + 8 * ep)
            snaps.append((theta.clone(), w.clone(), G.clone(), bufs['delta'].clone(), bufs['pi_last'].clone(), bufs['g'].clone()))
        return {'theta': torch.cat([s_[0] for s_ in snaps]), 'w': torch.cat([s_[1] for s_ in snaps]),
                'G': torch.cat([s_[2] for s_ in snaps]), 'delta': torch.cat([s_[3] for s_ in snaps]),
                'pi_last': torch.cat([s_[4] for s_ in snaps]), 'g': torch.cat([s_[5] for s_ in snaps]), 'racc': racc.clone()}
    a, b = _both(run)
    _same(a, b, ['theta', 'w', 'G', 'delta', 'pi_last', 'g', 'racc'])
    assert not torch.equal(a['theta'][0:1], a['theta'][1:2])     # the update was applied
    assert torch.isfinite(a['delta']).all()


@pytest.mark.parametrize('d', [21, 15])
def test_class_training_does_not_depend_on_the_instantiation(dev, d):
    """Two episodes of actor_critic.train, one update per episode (native episode loop, start rows drawn in the kernel):
    theta, w, the per-episode mean rewards, the last episode's rewards and the final states, bit for bit."""
    from discrete_mean_field_game_amd import _lib as L
    from discrete_mean_field_game_amd.mfg_ac2 import actor_critic
    rs = np.random.RandomState(0)
    mat = rs.dirichlet(np.ones(d), size=16)
    res = []
    for m in (1, 3):
        L.lib().mfg_set_core_mapping(m)
        np.random.seed(7)
        ac = actor_critic(d=d, pi0=mat, batch=25, rng='philox', seed=5, update_every='rollout', verbose=0)
        ac.train(num_episodes=2, gamma=GAMMA)
        (bufs,) = ac._train_bufs.values()
        res.append((float(np.ravel(ac.theta)[0]), ac.w[:, 0].copy(), bufs['ep_reward'][:2].cpu().numpy().copy(),
                    bufs['rollout']['reward'].cpu().numpy().copy(), ac._last_pi.cpu().numpy().copy()))
    L.lib().mfg_set_core_mapping(0)
    assert res[0][0] == res[1][0]
    for x, y in zip(res[0][1:], res[1][1:]):
        assert np.array_equal(x, y)
    assert res[0][0] != THETA and np.all(res[0][2] != 0.0)


@pytest.mark.parametrize('option', ['write_P', 'external', 'synthetic', 'discount_pow'])
@pytest.mark.parametrize('d', [21, 15])
def test_launches_with_an_option_take_the_general_kernel(dev, d, option):
    """One launch each with the actions written out, an external reward, the synthetic reward kind (and the running bootstrap
    factor): the specialised kernel has none of these, so mode 1 must hand the launch to the general instantiation -- the outputs
    equal mode 3's, the option's effect is there (P written and row-stochastic, no in-kernel reward in delta, the synthetic reward
    of the given-P kernel), and it differs from the plain training launch, which is what the specialised kernel would have produced."""
    from discrete_mean_field_game_amd import ops, _lib as L
    B, T = 13, 3
    pi0, th, w = _inputs(dev, d, B, seed=3)
    kw = dict(w=w, gamma=GAMMA, seed=99, first_step=1, traj_offset=5, td=True)
    opt = {'write_P': dict(write_P=True), 'external': dict(reward_kind=L.REWARD_EXTERNAL), 'synthetic': dict(reward_kind=L.REWARD_SYNTHETIC),
           'discount_pow': dict(discount_pow=True)}[option]

    def run():
        out = {'P': torch.full((B, T, d, d), float('nan'), device=dev)} if option == 'write_P' else None
        return ops.rollout(pi0, T, th, SHIFT, SCALE, out=out, **kw, **opt)
    a, b = _both(run)
    _same(a, b, ['pi_traj', 'pi_last', 'reward', 'delta', 'g', 'P', 'G'])
    L.lib().mfg_set_core_mapping(1)
    plain = ops.rollout(pi0, T, th, SHIFT, SCALE, **kw)
    assert torch.equal(plain['pi_traj'], a['pi_traj'])          # the same trajectories either way
    if option == 'write_P':
        assert torch.isfinite(a['P']).all() and float((a['P'].double().sum(-1) - 1).abs().max()) < 5e-7
        pn, r1 = ops.step_given_P(a['pi_traj'][:, 0].contiguous(), a['P'][:, 0].contiguous())
        assert torch.equal(pn, a['pi_traj'][:, 1]) and torch.equal(r1, a['reward'][:, 0])
    elif option == 'external':
        assert a['reward'] is None
        # delta without a reward: the plain launch's delta minus its reward, up to the rounding of that subtraction
        assert not torch.equal(a['delta'], plain['delta'])
        assert torch.allclose(a['delta'], plain['delta'] - plain['reward'].double(), rtol=0, atol=1e-6)
    elif option == 'synthetic':
        assert not torch.equal(a['reward'], plain['reward'])
        wp = ops.rollout(pi0, T, th, SHIFT, SCALE, write_P=True, **kw, **opt)
        _, r1 = ops.step_given_P(wp['pi_traj'][:, 0].contiguous(), wp['P'][:, 0].contiguous(), reward_kind=L.REWARD_SYNTHETIC)
        assert torch.equal(r1, a['reward'][:, 0])
    else:
        assert not torch.equal(a['delta'], plain['delta'])       # gamma^t in place of gamma (1 at the first step)
