"""CPU checks of the reward-learning infrastructure: the fp64 analytic gradient added to
oracle/reward_net_oracle.py against PyTorch autograd of networks.RewardNet and central differences, the oracle's
tf.train.AdamOptimizer formula, the device store's FIFO bookkeeping (on CPU tensors), and the flat parameter layout the
HIP training step expects (host-only entry points; no compute without a GPU)."""
import ctypes as C

import numpy as np
import pytest
import torch

from discrete_mean_field_game_amd.networks import REG_VARIANTS, RewardNet, maxent_irl_loss
from discrete_mean_field_game_amd.reward_learning import TrajectoryStore
from oracle import reward_net_oracle as RO


def _batch(rs, d, n):
    return rs.dirichlet(np.ones(d), size=n), rs.dirichlet(np.ones(d) * 0.5, size=(n, d))


@pytest.mark.parametrize('reg', ['none', 'l1l2'])
@pytest.mark.parametrize('d,k1,f2,k2', [(7, 5, 2, 3), (5, 3, 1, 5)])
def test_oracle_gradient_equals_autograd(reg, d, k1, f2, k2):
    torch.manual_seed(0)
    net = RewardNet(d=d, reg=reg, k1=k1, f2=f2, k2=k2, n_fc3=5, n_fc4=3).double()
    with torch.no_grad():
        for p in net.parameters():
            p.add_(0.05 * torch.randn_like(p))
    rs = np.random.RandomState(1)
    nd, ng, T = 2, 3, 15
    ds, da = _batch(rs, d, nd * T)
    gs, ga = _batch(rs, d, ng * T)
    (loss, first, second, reg_v), g, _ = RO.irl_loss_and_grad(RO.params_from_torch(net), ds, da, gs, ga, 5, ng, l1l2=net.use_l1l2)
    tl, tf_, ts = maxent_irl_loss(net(torch.tensor(ds), torch.tensor(da)), net(torch.tensor(gs), torch.tensor(ga)), 5, ng,
                                  net.regularization() if net.use_l1l2 else None)
    grads = torch.autograd.grad(tl, list(net.parameters()))
    ref = np.concatenate([x.numpy().reshape(-1) for x in grads])
    got = RO.flatten_like_kernel(g)
    assert abs(float(tl) - loss) < 1e-12 and abs(float(tf_) - first) < 1e-12 and abs(float(ts) - second) < 1e-12
    assert np.max(np.abs(got - ref)) <= 1e-12 * max(1.0, np.abs(ref).max())


def test_oracle_gradient_with_masks_equals_central_differences():
    """Dropout masks are constants of the graph: the analytic gradient with masks against finite differences of the masked
    forward (a few entries of every tensor)."""
    d, n3, n4 = 6, 4, 3
    torch.manual_seed(2)
    net = RewardNet(d=d, reg='dropout', n_fc3=n3, n_fc4=n4).double()
    with torch.no_grad():
        for p in net.parameters():
            p.add_(0.1 * torch.randn_like(p))
    rs = np.random.RandomState(5)
    ds, da = _batch(rs, d, 15)
    gs, ga = _batch(rs, d, 30)
    keep = 0.4
    m3 = np.where(rs.rand(45, n3) <= keep, 1 / keep, 0.0)
    m4 = np.where(rs.rand(45, n4) <= keep, 1 / keep, 0.0)
    prm = RO.params_from_torch(net)
    _, g, _ = RO.irl_loss_and_grad(prm, ds, da, gs, ga, 5, 2, masks=(m3, m4))

    def loss_of(pp):
        return RO.irl_loss_and_grad(pp, ds, da, gs, ga, 5, 2, masks=(m3, m4))[0][0]
    for name in RO.FLAT_ORDER:
        flat = prm[name].reshape(-1)
        for k in rs.choice(flat.size, size=min(4, flat.size), replace=False):
            pp = {n: v.copy() for n, v in prm.items()}
            h = 1e-6
            pp[name].reshape(-1)[k] += h
            up = loss_of(pp)
            pp[name].reshape(-1)[k] -= 2 * h
            dn = loss_of(pp)
            fd = (up - dn) / (2 * h)
            assert abs(fd - g[name].reshape(-1)[k]) <= 1e-6 * max(1.0, abs(fd)), (name, k)


def test_oracle_adam_is_tf_formula():
    """One hand-computed step of tf.train.AdamOptimizer (epsilon outside the bias correction: 'epsilon hat')."""
    p, g = np.array([1.0, -2.0]), np.array([0.5, -1e-9])
    p1, m1, v1 = RO.adam_tf(p, g, np.zeros(2), np.zeros(2), 1, lr=1e-2)
    lr_t = 1e-2 * np.sqrt(1 - 0.999) / (1 - 0.9)
    assert np.allclose(m1, 0.1 * g) and np.allclose(v1, 0.001 * g * g)
    assert np.allclose(p1, p - lr_t * m1 / (np.sqrt(v1) + 1e-8), rtol=0, atol=1e-18)
    assert abs((p - p1)[0] - 1e-2) < 1e-8                    # |g| >> eps: a full lr step


def test_store_fifo_matches_list_semantics():
    d, T = 3, 15
    rs = np.random.RandomState(0)

    def mk(n):
        return [[(rs.rand(d), rs.rand(d, d)) for _ in range(T)] for _ in range(n)]
    st = TrajectoryStore(d, T, 'cpu')
    ref = mk(4)
    st.assign_list(ref)
    for it in range(25):
        n = rs.randint(0, 5)
        drop = rs.randint(0, len(ref) + n + 1) if it % 3 == 0 else min(n, len(ref))
        new = mk(n)
        s = torch.tensor(np.array([[p[0] for p in t] for t in new]).reshape(n, T, d), dtype=torch.float32)
        a = torch.tensor(np.array([[p[1] for p in t] for t in new]).reshape(n, T, d, d), dtype=torch.float32)
        v0 = st.version
        st.push(s, a, drop=drop)
        assert st.version == v0 + 1
        ref = (ref + new)[drop:]                              # ac_irl.py:929-932
        got = st.to_list()
        assert got is st.to_list() and len(got) == len(ref)   # cached view
        for x, y in zip(got, ref):
            for (p0, P0), (p1, P1) in zip(x, y):
                assert np.array_equal(p0, p1.astype(np.float32)) and np.array_equal(P0, P1.astype(np.float32))
        assert len(set(st.rows)) == len(st.rows) and not (set(st.rows) & set(st._free))
    with pytest.raises(ValueError):
        st.assign_list([[(np.zeros(d), np.zeros((d, d)))] * 3])


def test_flat_layout_of_the_training_step_is_the_module_parameter_order():
    from discrete_mean_field_game_amd import _lib as L
    lib = L.lib()
    for d, k1, f2, k2, n3, n4 in [(21, 5, 2, 3, 8, 4), (15, 5, 2, 3, 8, 4), (9, 3, 1, 5, 6, 7)]:
        net = RewardNet(d=d, k1=k1, f2=f2, k2=k2, n_fc3=n3, n_fc4=n4)
        offs = (C.c_int64 * 11)()
        assert lib.mfg_reward_net_param_offsets(d, k1, f2, k2, n3, n4, offs) == 0
        sizes = [p.numel() for p in net.parameters()]
        assert list(offs) == list(np.cumsum([0] + sizes))
        assert lib.mfg_reward_net_num_params(d, k1, f2, k2, n3, n4) == sum(sizes)
        N = 150
        need = lib.mfg_reward_net_train_workspace_bytes(d, k1, f2, k2, n3, n4, N)
        assert need >= 4 * N * (1 + f2 * d * d + n3 + sum(sizes) - n3 * f2 * d * d)
    assert sum(p.numel() for p in RewardNet(d=21).parameters()) == 7235     # "~7k floats"


# ------------------------------------------------------------------ the coefficient phase restated (oracle/reward_net_oracle.py)
def _oracle_batch(reg='none', nd=3, ng=4, T=7, d=6, seed=3):
    torch.manual_seed(seed)
    net = RewardNet(d=d, reg=reg, n_fc3=5, n_fc4=3).double()
    with torch.no_grad():
        for p in net.parameters():
            p.add_(0.05 * torch.randn_like(p))
    rs = np.random.RandomState(seed)
    ds, da = _batch(rs, d, nd * T)
    gs, ga = _batch(rs, d, ng * T)
    return RO.params_from_torch(net), net, ds.reshape(nd * T, d), da.reshape(nd * T, d, d), gs.reshape(ng * T, d), ga.reshape(ng * T, d, d)


@pytest.mark.parametrize('reg', ['none', 'l1l2'])
def test_coefficients_from_rewards_agree_with_the_fp64_loss(reg):
    """Fed the oracle's own rewards rounded to fp32, the restated coefficient phase gives irl_loss_and_grad's loss terms and
    (through the `dr` override) its gradient, up to what the rounding of the inputs and the fp32 running sum can move them:
    |dS_j| <= T U (inputs) + T^2 U / 2 (running sum of |r| <= 1), and a soft-max weight moves by at most 2 max |dS| relative."""
    nd, ng, T = 3, 4, 7
    prm, net, ds, da, gs, ga = _oracle_batch(reg, nd, ng, T)
    (loss, first, second, regv), g, r = RO.irl_loss_and_grad(prm, ds, da, gs, ga, 5, ng, l1l2=net.use_l1l2, steps=T)
    co = RO.coefficients_from_rewards(r.astype(np.float32), nd, ng, T, 5)
    dS = (T + T * T / 2) * RO.U32
    assert co['S32'].dtype == np.float32 and co['c'].shape == (r.shape[0], 1)
    assert np.max(np.abs(co['S32'].astype(np.float64) - r[nd * T:].reshape(ng, T).sum(1))) <= dS
    ref_c = RO._coefficients(r, nd * T, ng, T, -1.0 / 5)
    assert np.max(np.abs(co['c'] / ref_c - 1.0)) <= 2 * dS and abs(co['c_traj'][nd:].sum() - 1.0) <= 1e-15
    assert np.all(co['c'][:nd * T] == -0.2)
    assert abs(co['first'] - first) <= nd * T * RO.U32 / 5 and abs(co['second'] - second) <= dS
    assert np.all(np.isfinite(co['eps'])) and co['eps'].shape == (ng,) and np.all(co['eps'] >= RO.C0_SOFTMAX * RO.U32)
    assert 0 < co['first_bound'] < 1e-5 and 0 < co['second_bound'] < 1e-5 and co['loss_rounding'](regv) <= 2.001 * RO.U32 * max(abs(loss), abs(first + second))
    (loss2, first2, second2, _), g2, _ = RO.irl_loss_and_grad(prm, ds, da, gs, ga, 5, ng, l1l2=net.use_l1l2, steps=T, dr=co['c'])
    assert (loss2, first2, second2) == (loss, first, second)            # the override drives the backward pass only
    a, b = RO.flatten_like_kernel(g2), RO.flatten_like_kernel(g)
    scale = RO.grad_scale(prm, ds, da, gs, ga, 5, ng, None, net.use_l1l2, steps=T)
    assert np.max(np.abs(a - b) - 2 * dS * scale) <= 1e-15 and np.max(np.abs(a - b)) > 0
    # the scale with given coefficients is the scale of those coefficients; steps may be left to the split over n_traj
    assert np.array_equal(scale, RO.grad_scale(prm, ds, da, gs, ga, 5, ng, None, net.use_l1l2))
    assert np.allclose(RO.grad_scale(prm, ds, da, gs, ga, 5, ng, None, False, steps=T, coeff=co['c']), scale, rtol=4 * dS, atol=1e-15)


def test_zero_trajectory_halves():
    """An empty demonstration half: first = 0 and the gradient is the generated half's; no generated trajectories: second = 0
    and the gradient is the demonstrations'.  The loss is linear in the two halves' gradients, so they add up to the full one."""
    nd, ng, T, d = 3, 4, 7, 6
    prm, net, ds, da, gs, ga = _oracle_batch('none', nd, ng, T, d)
    e_s, e_a = np.zeros((0, d)), np.zeros((0, d, d))
    (loss, first, second, _), g, r = RO.irl_loss_and_grad(prm, ds, da, gs, ga, 5, ng, steps=T)
    (l_g, f_g, s_g, _), g_g, r_g = RO.irl_loss_and_grad(prm, e_s, e_a, gs, ga, 5, ng, steps=T)
    (l_d, f_d, s_d, _), g_d, r_d = RO.irl_loss_and_grad(prm, ds, da, e_s, e_a, 5, 0, steps=T)
    assert f_g == 0 and s_g == second and l_g == second and r_g.shape == (ng * T, 1)
    assert s_d == 0 and f_d == first and l_d == first and r_d.shape == (nd * T, 1)
    full, parts = RO.flatten_like_kernel(g), RO.flatten_like_kernel(g_g) + RO.flatten_like_kernel(g_d)
    assert np.max(np.abs(full - parts)) <= 1e-13 * np.abs(full).max()
    co = RO.coefficients_from_rewards(r_d.astype(np.float32), nd, 0, T, 5)
    assert co['second'] == 0 and co['second_bound'] == 0 and co['eps'].size == 0 and co['S32'].size == 0 and co['c'].shape == (nd * T, 1)
    co = RO.coefficients_from_rewards(r_g.astype(np.float32), 0, ng, T, 5)
    assert co['first'] == 0 and co['first_bound'] == 0 and co['c'].shape == (ng * T, 1) and abs(co['c_traj'].sum() - 1) <= 1e-15
    alone = RO.grad_scale(prm, e_s, e_a, gs, ga, 5, ng, None, False, steps=T)          # the generated half alone, both ways
    assert np.allclose(alone, RO.grad_scale(prm, ds, da, gs, ga, 5, ng, None, False, steps=T, gen_only=True), rtol=1e-12, atol=1e-18)
    assert RO.grad_scale(prm, ds, da, e_s, e_a, 5, 0, None, False, steps=T).shape == full.shape
    with pytest.raises(ValueError):
        RO.coefficients_from_rewards(np.zeros(5, dtype=np.float32), 1, 1, 3, 5)


def _softmax_fp32(S32):
    """The kernel's soft-max arithmetic in NumPy float32: subtract the maximum, exp, a pairwise tree over 64 lanes, divide."""
    e = np.zeros(64, dtype=np.float32)
    e[:S32.size] = np.exp((S32 - S32.max()).astype(np.float32)).astype(np.float32)
    z = e.copy()
    while z.size > 1:
        z = (z[0::2] + z[1::2]).astype(np.float32)
    return (e[:S32.size] / z[0]).astype(np.float32)


def test_eps_over_the_gpu_grid():
    """Every case of the GPU tests' grid, on the CPU: the chosen seeds keep the oracle away from the ReLU kinks, eps is finite
    and below 1e-5, and an fp32 evaluation of the soft-max (NumPy's) stays within eps of the fp64 weights."""
    from oracle import reward_train_cases as RC
    assert len({c.name for c in RC.CASES}) == len(RC.CASES) == 28
    for case in RC.CASES:
        net, demo, gen, di, gi = RC.build(case, 'cpu')
        prm, ds, da, gs, ga, masks = RC.oracle_inputs(case, net, demo, gen, di, gi)
        r, cache = RO.forward_cache(prm, np.concatenate([ds, gs], 0), np.concatenate([da, ga], 0), masks)
        assert cache['kink'] >= 1e-6, case.name
        N = (case.n_demo + case.n_gen) * case.steps
        assert r.shape == (N, 1) and N <= 2048 and N * (1 + case.n3) * 4 <= 60 * 1024, case.name
        co = RO.coefficients_from_rewards(r.astype(np.float32), case.n_demo, case.n_gen, case.steps, RC.DEMO_DIVISOR)
        assert co['eps'].shape == (case.n_gen,) and np.all(np.isfinite(co['eps'])) and np.all(co['eps'] < 1e-5), case.name
        assert np.isfinite(co['first_bound']) and np.isfinite(co['second_bound']) and co['second_bound'] < 1e-5, case.name
        if case.n_gen:
            w32 = _softmax_fp32(co['S32']).astype(np.float64)
            assert np.all(np.abs(w32 / co['c_traj'][case.n_demo:] - 1.0) <= co['eps']), case.name
