"""The importance weights of the max-ent IRL loss on the device (reference ac_irl.py:292-379 calc_z, :404-406 the weighted loss):
mfg_traj_log_z_pop against oracle.mfg_oracle.calc_z, and the weighted training step (mfg_reward_net_train_step_z through
RewardTrainer.step(gen_log_z=...)) against the oracle's fp64 rewards -> softmax(S + ln z) -> the oracle's backward pass."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import mfg_oracle as O
from oracle import reward_net_oracle as RO
from oracle.reward_train_cases import _batch_np, _net, _stores

EINVAL, EWORKSPACE = -1, -4


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.fail('-m gpu tests need a GPU')
    return torch.device('cuda:0')


# ------------------------------------------------------------------ 1. the log weights
def _filled_store(K, d, T, dev, rs, n=4, stacked=True):
    """A store that has rotated: n + 2 trajectories pushed, then n more with the 3 oldest dropped -- physical != logical rows."""
    from discrete_mean_field_game_amd.reward_learning import StackedTrajectoryStore, TrajectoryStore
    st = StackedTrajectoryStore(K, d, T, dev) if stacked else TrajectoryStore(d, T, dev)
    lead = (K,) if stacked else ()
    for count, drop in ((n + 2, 0), (n, 3)):
        s = torch.as_tensor(rs.dirichlet(np.ones(d) * 0.7, size=lead + (count, T)), dtype=torch.float32)
        a = torch.as_tensor(rs.dirichlet(np.ones(d) * 0.5, size=lead + (count, T, d)), dtype=torch.float32)
        st.push(s.to(dev), a.to(dev), drop=drop)
    assert st.rows != list(range(len(st.rows)))
    return st


def _oracle_rows(st, k, thetas, shift, nss):
    """oracle calc_z of learner k's trajectories, in LOGICAL order"""
    s, a = st.gather(k=k) if st.state.dim() == 4 else st.gather()
    return O.calc_z(s.cpu().numpy(), a.cpu().numpy(), thetas, shift, nss)


def _assert_log_z(got, want):
    """ln z of some rows against the oracle's calc_z on the same rows."""
    np.testing.assert_allclose(got, want, rtol=1e-9, atol=1e-6)


@pytest.mark.parametrize('n_pol', [1, 3, 10, 70])
@pytest.mark.parametrize('steps', [3, 15])
@pytest.mark.parametrize('d', [4, 15, 21])
def test_log_weights_match_the_oracle(dev, d, steps, n_pol):
    """K = 3 learners with their own theta tables and shifts on per-learner stores; the K = 1 form of every learner gives the
    same bits; rows listed are written, the others keep what the output held."""
    from discrete_mean_field_game_amd import ops
    K, nss = 3, 7
    rs = np.random.RandomState(1000 * d + 10 * steps + n_pol)
    st = _filled_store(K, d, steps, dev, rs)
    thetas = 7.9 + 1.1 * rs.rand(K, n_pol)
    shifts = np.array([0.0, 0.1, -0.05])
    th_dev, sh_dev = torch.as_tensor(thetas, device=dev), torch.as_tensor(shifts, device=dev)
    cap = st.capacity
    out = torch.full((K, cap), 123.0, dtype=torch.float64, device=dev)
    ops.traj_log_z_pop(st.state, st.action, st.rows, th_dev, sh_dev, np.log(nss), out=out)
    got = out.cpu().numpy()
    unlisted = sorted(set(range(cap)) - set(st.rows))
    assert unlisted and np.all(got[:, unlisted] == 123.0)
    for k in range(K):
        _assert_log_z(got[k, st.rows], _oracle_rows(st, k, thetas[k], shifts[k], nss))
        one = ops.traj_log_z_pop(st.state[k].contiguous(), st.action[k].contiguous(), st.rows, th_dev[k:k + 1].contiguous(),
                                 sh_dev[k:k + 1].contiguous(), np.log(nss))
        assert torch.equal(one[0, st.rows], out[k, st.rows]), k
        assert torch.isnan(one[0, unlisted]).all()


@pytest.mark.parametrize('K', [1, 3])
def test_log_weights_shared_store_and_subset(dev, K):
    """One TrajectoryStore read by all K learners, and a strict subset of its rows: the unlisted rows of a pre-filled output
    are untouched, the listed ones equal the full call's bit for bit."""
    from discrete_mean_field_game_amd import ops
    d, T, n_pol, nss = 15, 15, 5, 9
    rs = np.random.RandomState(77 + K)
    st = _filled_store(1, d, T, dev, rs, stacked=False)
    thetas = 7.9 + 1.1 * rs.rand(K, n_pol)
    shifts = 0.05 * rs.randn(K)
    th_dev, sh_dev = torch.as_tensor(thetas, device=dev), torch.as_tensor(shifts, device=dev)
    full = ops.traj_log_z_pop(st.state, st.action, st.rows, th_dev, sh_dev, np.log(nss))
    s, a = st.gather()
    for k in range(K):
        want = O.calc_z(s.cpu().numpy(), a.cpu().numpy(), thetas[k], shifts[k], nss)
        np.testing.assert_allclose(full[k, st.rows].cpu().numpy(), want, rtol=1e-9, atol=1e-6)
    some = st.rows[1::2]
    out = torch.full_like(full, -1.0)
    ops.traj_log_z_pop(st.state, st.action, some, th_dev, sh_dev, np.log(nss), out=out)
    rest = sorted(set(range(out.shape[1])) - set(some))
    assert torch.equal(out[:, some], full[:, some]) and bool((out[:, rest] == -1.0).all())
    # calc_z's alpha floor and p_floor are parameters of the call: an exact zero in P with p_floor = 0 gives +inf, a floor hides it
    a0 = st.action.clone()
    a0[st.rows[0], 2, 1, 3] = 0.0
    z = ops.traj_log_z_pop(st.state, a0, st.rows[:2], th_dev, sh_dev, np.log(nss))
    assert bool(torch.isinf(z[:, st.rows[0]]).all()) and bool((z[:, st.rows[0]] > 0).all()) and bool(torch.isfinite(z[:, st.rows[1]]).all())
    assert bool(torch.isfinite(ops.traj_log_z_pop(st.state, a0, st.rows[:2], th_dev, sh_dev, np.log(nss), p_floor=1e-30)[:, st.rows[:2]]).all())


def test_log_weights_error_paths(dev):
    """Every refusal comes with its code before anything is launched: the pre-filled output is untouched."""
    from discrete_mean_field_game_amd import _lib as L
    K, d, T, n_pol, cap = 2, 4, 3, 2, 6
    rs = np.random.RandomState(5)
    state = torch.as_tensor(rs.dirichlet(np.ones(d), size=(K, cap, T)), dtype=torch.float32, device=dev)
    action = torch.as_tensor(rs.dirichlet(np.ones(d), size=(K, cap, T, d)), dtype=torch.float32, device=dev)
    thetas = torch.full((K, n_pol), 8.0, dtype=torch.float64, device=dev)
    shift = torch.zeros(K, dtype=torch.float64, device=dev)
    out = torch.full((K, cap), 5.0, dtype=torch.float64, device=dev)
    scratch = torch.empty(8, dtype=torch.int32, device=dev)
    fn = L.lib().mfg_traj_log_z_pop

    def call(rows=(0, 1, 2), state_p=state.data_ptr(), thetas_p=thetas.data_ptr(), out_p=out.data_ptr(), capacity=cap, steps=T,
             d_=d, n_pol_=n_pol, K_=K, scratch_p=scratch.data_ptr(), scratch_bytes=32, n_rows=None):
        rw = (C.c_int32 * max(len(rows), 1))(*rows)
        return fn(state_p, action.data_ptr(), capacity, rw, len(rows) if n_rows is None else n_rows, steps, d_, thetas_p, n_pol_,
                  shift.data_ptr(), K_, 1, 1.0, 1.0 + 1e-6, 0.0, 0.0, out_p, scratch_p, scratch_bytes, None)
    for kw in (dict(state_p=None), dict(thetas_p=None), dict(out_p=None), dict(scratch_p=None), dict(capacity=0), dict(steps=0),
               dict(d_=0), dict(n_pol_=0), dict(K_=0), dict(n_rows=-1), dict(rows=(0, cap)), dict(rows=(-1,)), dict(rows=(1, 3, 1))):
        assert call(**kw) == EINVAL, kw
        assert L.lib().mfg_last_error()
    assert call(scratch_bytes=8) == EWORKSPACE
    torch.cuda.synchronize()
    assert bool((out == 5.0).all())
    assert call(rows=()) == 0 and call() == 0
    torch.cuda.synchronize()
    assert bool((out[:, 3:] == 5.0).all()) and bool((out[:, :3] != 5.0).all())


# ------------------------------------------------------------------ 2. the weighted training step
GEOMS = [(21, 8, 4, 5, 2, 3), (15, 8, 4, 5, 2, 3), (4, 3, 2, 5, 2, 3), (12, 32, 32, 7, 2, 7)]   # d, n3, n4, k1, f2, k2; the last: no matrix cores
# n_gen -> (n_demo, steps): 64 trajectories of 15 steps are beyond the step's LDS limit at n_fc3 = 32 (N (1 + n3) 4 B <= 60 KB)
BATCH = {1: (5, 15), 5: (5, 15), 64: (3, 5)}
U32 = 2.0 ** -24


def _weighted_reference(prm, ds, da, gs, ga, ng, T, lz, l1l2, masks):
    nd_t = ds.shape[0]
    r, _ = RO.forward_cache(prm, np.concatenate([ds, gs], 0), np.concatenate([da, ga], 0), masks)
    D = r[nd_t:].reshape(ng, T).sum(1) + lz
    e = np.exp(D - D.max())
    c = e / e.sum()
    second = float(D.max() + np.log(e.sum() / ng))
    dr = np.concatenate([np.full(nd_t, -1.0 / 5), np.repeat(c, T)])[:, None]
    (_, first, _, reg), g, _ = RO.irl_loss_and_grad(prm, ds, da, gs, ga, 5, ng, l1l2=l1l2, steps=T, masks=masks, dr=dr)
    scale = RO.grad_scale(prm, ds, da, gs, ga, 5, ng, masks, l1l2, steps=T, coeff=dr)
    return (first + second + reg, first, second, reg), RO.flatten_like_kernel(g), scale, c


def _run_weighted(dev, geom, reg, nd, ng, T, lz_of, data_seed=None, check_ess=True):
    """One gradient-only weighted step against the reference; lz_of(rs, ng) -> the batch's ln z.  Returns what the caller may
    want to look at."""
    from discrete_mean_field_game_amd.reward_learning import RewardTrainer
    d, n3, n4, k1, f2, k2 = geom
    rs = np.random.RandomState(d * 100 + n3 + ng if data_seed is None else data_seed)
    net = _net(d, reg, n3, n4, dev, k1, f2, k2)
    demo, gen = _stores(d, max(nd, 1) + 2, ng + 4, dev, rs, T=T)
    tr = RewardTrainer(net, 1e-4)
    demo_idx = list(rs.permutation(len(demo))[:nd])
    gen_idx = list(rs.permutation(len(gen))[:ng])
    lz = np.asarray(lz_of(rs, ng), dtype=np.float64)
    lz_store = torch.full((gen.state.shape[0],), float('nan'), dtype=torch.float64, device=dev)
    rows = [gen.rows[i] for i in gen_idx]
    lz_store[torch.as_tensor(rows, device=dev)] = torch.as_tensor(lz, device=dev)
    seed = 0xABCDEF0123 + d
    before = tr.flat.clone()
    tr.step(demo, [demo.rows[i] for i in demo_idx], gen, rows, 5, seed, grad_only=True, gen_log_z=lz_store)
    torch.cuda.synchronize()
    assert torch.equal(before, tr.flat) and tr.step_count == 0
    ds, da = _batch_np(demo, demo_idx)
    gs, ga = _batch_np(gen, gen_idx)
    prm = RO.params_from_torch(net)
    masks = RO.dropout_masks(net.keep_prob, seed, 0, (nd + ng) * T, n3, n4) if net.use_dropout else None
    (loss, first, second, regv), ref, scale, c = _weighted_reference(prm, ds, da, gs, ga, ng, T, lz, net.use_l1l2, masks)
    ess = 1.0 / np.sum(c * c)
    print('geom', geom, reg, 'nd', nd, 'ng', ng, 'T', T, 'ess %.3f' % ess)
    if check_ess and ng > 1:
        assert ess >= 2.0, ess                      # a condition on the inputs: the weights are not one-hot, the test not vacuous
    got = tr.grad.cpu().numpy().astype(np.float64)
    offs = np.cumsum([0] + [p.numel() for p in net.parameters()])
    for k in range(10):                             # the tolerance of tests/test_gpu_reward_train.py, per tensor
        a, b, sc = got[offs[k]:offs[k + 1]], ref[offs[k]:offs[k + 1]], scale[offs[k]:offs[k + 1]]
        print(' ', RO.FLAT_ORDER[k], 'err %.3e' % np.max(np.abs(a - b)), 'ref %.3e' % np.max(np.abs(b)), 'scale %.3e' % np.max(sc))
        assert np.max(np.abs(a - b)) <= 1e-5 * max(np.max(np.abs(b)), np.max(sc), 1e-3), \
            (RO.FLAT_ORDER[k], np.max(np.abs(a - b)), np.max(np.abs(b)), np.max(sc))
    st = tr.stats.cpu().numpy().astype(np.float64)
    print('  stats', st, 'ref', (loss, first, second, regv))
    big = 1e-5 + 4 * U32 * max(1.0, abs(second))   # an fp32 number of magnitude |second|: its rounding, plus the existing budget
    assert abs(st[1] - first) <= 1e-5 and abs(st[3] - regv) <= 2e-6 * max(1.0, regv)
    assert abs(st[2] - second) <= big and abs(st[0] - loss) <= big
    return dict(trainer=tr, demo=demo, gen=gen, demo_rows=[demo.rows[i] for i in demo_idx], gen_rows=rows, seed=seed, lz=lz,
                lz_store=lz_store, stats=st, second=second, c=c, ref=ref, scale=scale)


def _unit_spread(rs, ng):
    return -5700.0 + rs.randn(ng)


@pytest.mark.parametrize('n_gen', [1, 5, 64])
@pytest.mark.parametrize('reg', ['none', 'dropout_l1l2'])
@pytest.mark.parametrize('geom', GEOMS, ids=lambda g: 'd%d-n%d-%d-k%d%d' % (g[0], g[1], g[2], g[3], g[5]))
def test_weighted_gradient_and_loss_match_the_fp64_reference(dev, geom, reg, n_gen):
    """ln z = -5700 + N(0, 1) per row: the common offset catches an fp32 hand-over (5e-4 per weight), the unit spread keeps
    the soft-max from collapsing."""
    nd, T = BATCH[n_gen]
    _run_weighted(dev, geom, reg, nd, n_gen, T, _unit_spread)


# data seeds of the three extra cases: the first for which the REFERENCE (fp64 oracle, CPU) has an effective sample size >= 2 and
# keeps its ReLU inputs 3e-6 away from the kink (oracle/reward_train_cases.py: closer, an fp32 evaluation may take the other branch)
def test_weighted_step_without_demonstrations(dev):
    _run_weighted(dev, GEOMS[1], 'dropout_l1l2', 0, 5, 15, _unit_spread, data_seed=2)


def test_weighted_step_with_nearly_one_hot_weights(dev):
    """Spread 40: what the estimator gives at d = 15 (effective sample size 2 of 8) and beyond."""
    out = _run_weighted(dev, GEOMS[0], 'dropout_l1l2', 5, 5, 15, lambda rs, ng: -5700.0 + 40.0 * rs.randn(ng), check_ess=False)
    assert 1.0 / np.sum(out['c'] ** 2) < 1.1          # the input condition of this case: one trajectory carries the batch


@pytest.mark.parametrize('geom', [GEOMS[1], GEOMS[3]], ids=['d15', 'd12'])
def test_constant_log_weights_leave_the_gradient_and_shift_the_second_term(dev, geom):
    const = -5700.0
    out = _run_weighted(dev, geom, 'dropout_l1l2', 5, 5, 15, lambda rs, ng: np.full(ng, const), data_seed=1)
    tr = out['trainer']
    gz = tr.grad.double().cpu().numpy()
    tr.step(out['demo'], out['demo_rows'], out['gen'], out['gen_rows'], 5, out['seed'], grad_only=True)
    g0 = tr.grad.double().cpu().numpy()
    st0 = tr.stats.double().cpu().numpy()
    offs = np.cumsum([0] + [p.numel() for p in tr.net.parameters()])
    for k in range(10):             # a constant ln z cancels in the soft-max: the unweighted gradient meets the SAME reference
        a, b, sc = g0[offs[k]:offs[k + 1]], out['ref'][offs[k]:offs[k + 1]], out['scale'][offs[k]:offs[k + 1]]
        assert np.max(np.abs(a - b)) <= 1e-5 * max(np.max(np.abs(b)), np.max(sc), 1e-3), RO.FLAT_ORDER[k]
    # second: the weighted one's budget (fp32 rounding at 5.7e3 + 1e-5) and the unweighted one's 1e-5
    assert abs((out['stats'][2] - st0[2]) - const) <= 1e-5 + 4 * U32 * abs(out['second']) + 1e-5


def test_null_path_is_unchanged_by_a_weighted_call(dev):
    """Nothing sticky: the unweighted step gives the same bits before and after a weighted one on the same trainer."""
    from discrete_mean_field_game_amd.reward_learning import RewardTrainer
    d = 15
    rs = np.random.RandomState(9)
    demo, gen = _stores(d, 7, 9, dev, rs)
    tr = RewardTrainer(_net(d, 'dropout_l1l2', 8, 4, dev), 1e-4)
    dr, gr = [demo.rows[i] for i in (4, 1, 6, 2, 5)], [gen.rows[i] for i in (7, 0, 3, 8, 1)]
    lz = torch.as_tensor(-5700.0 + rs.randn(gen.state.shape[0]), device=dev)
    tr.step(demo, dr, gen, gr, 5, 321, grad_only=True)
    g0, s0 = tr.grad.clone(), tr.stats.clone()
    tr.step(demo, dr, gen, gr, 5, 321, grad_only=True, gen_log_z=lz)
    gz = tr.grad.clone()
    tr.step(demo, dr, gen, gr, 5, 321, grad_only=True)
    assert torch.equal(tr.grad, g0) and torch.equal(tr.stats, s0)
    assert not torch.equal(gz, g0)
    with pytest.raises(ValueError):
        tr.step(demo, dr, gen, gr, 5, 321, grad_only=True, gen_log_z=lz.float())
    with pytest.raises(ValueError):
        tr.step(demo, dr, gen, gr, 5, 321, grad_only=True, gen_log_z=lz[:-1].contiguous())
