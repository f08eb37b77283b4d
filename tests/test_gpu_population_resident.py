"""-m gpu: the resident step-mode episodes of a small-batch population (mfg_train_episodes_pop_resident: one workgroup per
learner, no launch per env step; the reference's per-step updates, mfg_ac2.py:478-526) leave, bit for bit, what the per-step
launches of mfg_train_episodes_pop leave -- theta, w, G, pi, reward, delta, g and reward_acc, torch.equal -- and one case goes
against the fp64 oracle directly.  All runs are a few episodes at the reference point (theta 8.86349, shift 0.16, alpha
12 000, default learning rates; seeds and theta differ per learner), so everything stays finite and nothing reports a range.
"""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

KEYS = ('theta', 'w', 'G', 'pi', 'reward', 'delta', 'g', 'acc')


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.fail('-m gpu tests need a GPU')
    from discrete_mean_field_game_amd import ops
    ops.init()
    return torch.device('cuda', 0)


def _features(d):
    return d * (d + 1) // 2 + d + 1


def _inputs(d, K, seed):
    rs = np.random.RandomState(seed)
    return dict(mat=rs.dirichlet(np.ones(d), size=9).astype(np.float32), theta=8.86349 + 0.05 * np.arange(K),
                w=rs.rand(K, _features(d)) * 0.1, seed=(1000 + 7 * np.arange(K)).astype(np.int64),
                acc0=rs.rand(K, 65) * 1e-3)


def _run(dev, resident, inp, d, K, Bk, T, E, precision='mixed', kind=0, constant=0, first_step=0, first_episode=0,
         traj_offset=0):
    """One call of either entry point from identical inputs; every output as a dict of device tensors."""
    from discrete_mean_field_game_amd import ops
    F = _features(d)
    t64 = lambda x: torch.as_tensor(np.ascontiguousarray(x), dtype=torch.float64, device=dev)
    full = lambda v: torch.full((K,), v, dtype=torch.float64, device=dev)
    theta, w = t64(inp['theta']), t64(inp['w'])
    G = torch.zeros(K, F + 3, dtype=torch.float64, device=dev)
    ws = torch.zeros(K, ops.pop_workspace_slice(Bk, d, T) // 8, dtype=torch.float64, device=dev)
    acc = t64(inp['acc0'][:, :E])           # (the returns are ADDED to what the slots hold)
    pi = torch.zeros(K, Bk, d, dtype=torch.float32, device=dev)
    bufs = dict(scratch=torch.zeros_like(pi), reward=torch.zeros(K, Bk, dtype=torch.float32, device=dev),
                delta=torch.zeros(K, Bk, dtype=torch.float64, device=dev), g=torch.zeros(K, Bk, dtype=torch.float64, device=dev))
    fn = ops.train_episodes_pop_resident if resident else ops.train_episodes_pop
    fn(torch.as_tensor(inp['mat'], device=dev), pi, T, E, first_episode, constant, theta, full(0.16), full(12000.0), w, 1.0,
       full(0.1), full(0.001), torch.as_tensor(inp['seed'], device=dev), G, ws, bufs, reward_kind=kind, first_step=first_step,
       traj_offset=traj_offset, reward_acc=acc, precision=precision)
    return dict(theta=theta, w=w, G=G, pi=pi, reward=bufs['reward'], delta=bufs['delta'], g=bufs['g'], acc=acc)


def _identical(dev, d, K, Bk, T, E, **kw):
    inp = _inputs(d, K, 100 * d + Bk)
    a = _run(dev, True, inp, d, K, Bk, T, E, **kw)
    b = _run(dev, False, inp, d, K, Bk, T, E, **kw)
    torch.cuda.synchronize()
    for key in KEYS:
        assert torch.isfinite(b[key]).all(), key
        assert torch.equal(a[key], b[key]), '%s differs (d=%d K=%d Bk=%d T=%d E=%d %s)' % (key, d, K, Bk, T, E, kw)
    assert not torch.equal(b['theta'], torch.as_tensor(inp['theta'], device=dev)), 'nothing trained'
    from discrete_mean_field_game_amd import ops
    assert ops.status() == 0


# Bk: a partial tile, exactly one tile (12 at d = 21, 16 at d = 15), a second tile holding one trajectory, three tiles.
# T = 1 and 15 leave the final states in the scratch side.  Both rewards, both precisions, constant 0 and 1 along the way.
@pytest.mark.parametrize('d,K,Bk,T,E,precision,kind,constant', [
    (21, 1, 2, 1, 1, 'mixed', 0, 0), (21, 3, 12, 2, 3, 'mixed', 0, 1), (21, 3, 13, 15, 3, 'mixed', 0, 0),
    (21, 3, 30, 15, 1, 'mixed', 1, 0), (21, 3, 13, 2, 3, 'f64', 0, 0), (21, 1, 30, 1, 3, 'f64', 1, 1),
    (15, 1, 2, 15, 1, 'mixed', 1, 1), (15, 3, 16, 1, 3, 'mixed', 0, 0), (15, 3, 17, 2, 3, 'mixed', 0, 0),
    (15, 3, 40, 15, 3, 'mixed', 0, 1), (15, 3, 17, 15, 1, 'f64', 1, 0), (15, 1, 40, 2, 3, 'f64', 0, 0)])
def test_resident_equals_per_step_launches(dev, d, K, Bk, T, E, precision, kind, constant):
    _identical(dev, d, K, Bk, T, E, precision=precision, kind=kind, constant=constant)


def test_more_learners_than_resident_blocks(dev):
    _identical(dev, 21, 600, 2, 2, 1)      # 600 workgroups > 256 CUs x 2


def test_one_episode_more_than_a_launch_holds(dev):
    _identical(dev, 21, 2, 13, 2, 65)      # 64 + 1 episodes: two launches, the schedule and the Philox step carry over


def test_nonzero_first_step_and_first_episode(dev):
    _identical(dev, 21, 3, 13, 2, 3, first_step=1000, first_episode=5)


def test_trajectory_ids_beyond_32_bits(dev):
    _identical(dev, 15, 3, 17, 2, 1, traj_offset=2 ** 32 + 5)


def test_the_cap_of_64_tiles(dev):
    _identical(dev, 21, 2, 768, 2, 1)


def test_against_the_fp64_oracle(dev):
    """K = 2, d = 21, Bk = 13, T = 2, 2 episodes in strict precision, replayed by the oracle on the sampled actions as
    tests/test_gpu_classes.py replays a step-mode episode (_replay_step_mode: the same start draw, the same action counters,
    oracle math in fp64), with that test's tolerance: 1e-9 on theta and w."""
    from discrete_mean_field_game_amd import ops
    from oracle import mfg_oracle as O
    from oracle.philox_ref import start_indices
    d, K, Bk, T, E = 21, 2, 13, 2, 2
    inp = _inputs(d, K, 5)
    inp['acc0'] = np.zeros_like(inp['acc0'])
    out = _run(dev, True, inp, d, K, Bk, T, E, precision='f64')
    for k in range(K):
        seed = int(inp['seed'][k])
        w, theta = inp['w'][k].copy(), float(inp['theta'][k])
        for e in range(E):
            pi = inp['mat'][start_indices(seed, e * T, np.arange(Bk), inp['mat'].shape[0])].astype(np.float32)
            sc, sa = O.lr_scales(e, False)
            for t in range(T):
                th = torch.tensor([theta], dtype=torch.float64, device=dev)
                P = ops.sample_dirichlet(torch.as_tensor(pi, device=dev), th, 0.16, 12000.0, seed=seed, step=e * T + t,
                                         precision='f64').cpu().numpy()
                pn = O.transition(P, pi).astype(np.float32)
                P64, pi64 = P.astype(np.float64), pi.astype(np.float64)
                r = O.calc_reward(P64, pi64)
                _, _, G_w, G_theta, _ = O.batched_td_pg(pi, pn, P, r, w, theta, 0.16, 1.0)
                w = w + 0.1 * sc * G_w / Bk
                theta = theta + 0.001 * sa * G_theta / Bk
                pi = pn
        dt, dw = abs(float(out['theta'][k]) - theta), float(np.max(np.abs(out['w'][k].cpu().numpy() - w)))
        print('[resident oracle] learner %d: |theta - ref| %.3g, max |w - ref| %.3g' % (k, dt, dw))
        assert dt < 1e-9 and dw < 1e-9


def _population(resident, **kw):
    from discrete_mean_field_game_amd import ActorCriticPopulation
    rs = np.random.RandomState(3)
    d = 21
    table = rs.dirichlet(np.ones(d), size=40)
    w0 = rs.rand(3, _features(d)) * 0.1
    return ActorCriticPopulation([8.86349, 8.9, 8.8], 0.16, 12000, d, batch=13, seeds=[5, 9, 11], w0=w0, pi0=table,
                                 resident=resident, **kw), table, w0


def test_class_resident_equals_per_step_and_actor_critic(dev):
    from discrete_mean_field_game_amd.mfg_ac2 import actor_critic
    E = 2
    runs = []
    for resident in (True, False):
        pop, table, w0 = _population(resident)
        r1 = pop.train(E)
        r2 = pop.train(E, first_episode=E)      # (the carried Philox step)
        runs.append((pop.thetas, pop.w, r1, r2))
        assert pop.status() == 0
    for a, b in zip(*runs):
        assert np.array_equal(a, b)
    assert np.all(np.isfinite(runs[0][0])) and not np.array_equal(runs[0][0], [8.86349, 8.9, 8.8])
    ac = actor_critic(8.9, 0.16, 12000, 21, pi0=table, batch=13, seed=9, update_every='step', verbose=0)
    ac.w = w0[1]
    ac.train(E)
    ac.train(E, first_episode=E)
    assert np.array_equal(runs[0][0][1], ac.theta[0]) and np.array_equal(runs[0][1][1], ac.w.reshape(-1))


def test_class_under_a_control_block(dev):
    """resident=True refuses a call that needs the control block; resident=None takes the per-step launches for it."""
    pop, _, _ = _population(True)
    before = pop.thetas
    with pytest.raises(ValueError):
        pop.train(2, stop_criteria=0.01)
    assert np.array_equal(pop.thetas, before) and pop._rng_step == 0
    runs = []
    for resident in (None, False):
        pop, _, _ = _population(resident)
        r = pop.train(2, stop_criteria=0.01)
        runs.append((pop.thetas, pop.w, r, pop.learner_state, pop.episodes_run))
    for a, b in zip(*runs):
        assert np.array_equal(a, b)


def test_library_refusals(dev):
    """d = 20, Bk = 769 at d = 21 and a bound control block: MFG_EUNSUPPORTED (-3) before anything is launched."""
    from discrete_mean_field_game_amd import _lib as L
    from discrete_mean_field_game_amd import ops
    lib = L.lib()
    K, T = 2, 2
    f32 = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev)
    f64 = lambda *s: torch.zeros(*s, dtype=torch.float64, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def make(d, Bk):
        F = _features(d)
        t = dict(mat=torch.full((8, d), 1.0 / d, dtype=torch.float32, device=dev), pi=f32(K, Bk, d), scr=f32(K, Bk, d),
                 rew=f32(K, Bk), dl=f64(K, Bk), g=f64(K, Bk), theta=f64(K) + 8.86349, w=f64(K, F), G=f64(K, F + 3),
                 sh=f64(K) + 0.16, al=f64(K) + 12000.0, lc=f64(K) + 0.1, la=f64(K) + 1e-3,
                 seeds=torch.zeros(K, dtype=torch.int64, device=dev))
        sb = ops.pop_workspace_slice(Bk, d, T)
        t['ws'] = f64(K, sb // 8)

        def call(wsb=sb):
            return lib.mfg_train_episodes_pop_resident(
                t['mat'].data_ptr(), 8, t['pi'].data_ptr(), t['scr'].data_ptr(), Bk, K, d, T, 1, 0, 0, t['theta'].data_ptr(),
                t['sh'].data_ptr(), t['al'].data_ptr(), t['w'].data_ptr(), 1.0, 0, t['seeds'].data_ptr(), 0, 0, 1,
                t['lc'].data_ptr(), t['la'].data_ptr(), t['rew'].data_ptr(), t['dl'].data_ptr(), t['g'].data_ptr(),
                t['G'].data_ptr(), None, t['ws'].data_ptr(), wsb, stream)
        return t, call

    def untouched(t):
        torch.cuda.synchronize()
        return (bool((t['theta'] == 8.86349).all()) and not t['w'].any() and not t['G'].any() and not t['pi'].any()
                and not t['rew'].any() and not t['dl'].any() and not t['g'].any())

    for d, Bk in ((20, 13), (21, 769)):
        t, call = make(d, Bk)
        assert call() == -3, (d, Bk)
        assert untouched(t), 'a refused call launched work'
    t, call = make(21, 13)
    assert call(wsb=256) == -4 and untouched(t)
    # a control block on the bound context
    ctx = ops.Context(dev)
    prev = ctx.bind_scoped()
    try:
        ints, theta_prev, stop = torch.zeros(3, K, dtype=torch.int32, device=dev), f64(K), f64(K) - 1.0
        ctx.set_pop_control(ints[0], ints[1], theta_prev, ints[2], stop)
        assert call() == -3
        assert untouched(t) and not ints.any(), 'a refused call launched work'
        ctx.set_pop_control()
        assert call() == 0
        torch.cuda.synchronize()
        assert not untouched(t) and bool(torch.isfinite(t['theta']).all())
        assert ctx.status() == 0
    finally:
        ctx.restore(prev)
        ctx.close()
