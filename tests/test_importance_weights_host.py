"""CPU checks of the importance-weighted max-ent IRL loss (reference ac_irl.py:292-321 z_j, :404-406 the weighted second
term it leaves commented out): networks.maxent_irl_loss(log_z=...) in fp64 against the closed form and against the oracle's
backward pass driven by the weighted coefficients softmax(S + ln z); the three new C entry points are declared, bound and
exported under ABI 18; the classes take the keyword and default to off."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

from discrete_mean_field_game_amd.networks import RewardNet, maxent_irl_loss
from oracle import reward_net_oracle as RO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ('mfg_traj_log_z_pop', 'mfg_reward_net_train_step_z', 'mfg_reward_net_train_steps_pop_z')


def _case(reg, d=7, nd=2, ng=4, T=15, seed=0):
    torch.manual_seed(seed)
    net = RewardNet(d=d, reg=reg, n_fc3=5, n_fc4=3).double()
    with torch.no_grad():
        for p in net.parameters():
            p.add_(0.05 * torch.randn_like(p))
    rs = np.random.RandomState(seed + 1)
    ds, da = rs.dirichlet(np.ones(d), size=nd * T), rs.dirichlet(np.ones(d) * 0.5, size=(nd * T, d))
    gs, ga = rs.dirichlet(np.ones(d), size=ng * T), rs.dirichlet(np.ones(d) * 0.5, size=(ng * T, d))
    return net, rs, (ds, da, gs, ga)


def weighted_reference(prm, ds, da, gs, ga, n_div, ng, T, lz, l1l2=False, masks=None):
    """The weighted loss and gradient from the oracle's fp64 rewards: c = softmax(S + ln z), second = logsumexp(S + ln z) - ln M,
    then the oracle's own backward pass with those coefficients."""
    nd_t = ds.shape[0]
    r, _ = RO.forward_cache(prm, np.concatenate([ds, gs], 0), np.concatenate([da, ga], 0), masks)
    D = r[nd_t:].reshape(ng, T).sum(1) + np.asarray(lz, dtype=np.float64)
    e = np.exp(D - D.max())
    c = e / e.sum()
    second = float(D.max() + np.log(e.sum() / ng))
    dr = np.concatenate([np.full(nd_t, -1.0 / n_div), np.repeat(c, T)])[:, None]
    (_, first, _, reg), g, _ = RO.irl_loss_and_grad(prm, ds, da, gs, ga, n_div, ng, l1l2=l1l2, steps=T, masks=masks, dr=dr)
    return (first + second + reg, first, second, reg), RO.flatten_like_kernel(g), c, dr


@pytest.mark.parametrize('reg', ['none', 'l1l2'])
@pytest.mark.parametrize('offset,spread', [(0.0, 1.0), (-5700.0, 1.0), (-13300.0, 20.0)])
def test_weighted_loss_and_gradient_equal_the_closed_form_and_the_oracle(reg, offset, spread):
    net, rs, (ds, da, gs, ga) = _case(reg)
    ng, T = 4, 15
    lz = offset + spread * rs.randn(ng)
    (loss, first, second, _), ref, c, _ = weighted_reference(RO.params_from_torch(net), ds, da, gs, ga, 5, ng, T, lz,
                                                            l1l2=net.use_l1l2)
    tl, tf_, ts = maxent_irl_loss(net(torch.tensor(ds), torch.tensor(da)), net(torch.tensor(gs), torch.tensor(ga)), 5, ng,
                                  net.regularization() if net.use_l1l2 else None, log_z=torch.tensor(lz))
    tol = 1e-12 * max(1.0, abs(offset))
    grads = torch.autograd.grad(tl, list(net.parameters()))
    tl, tf_, ts = tl.detach(), tf_.detach(), ts.detach()
    assert abs(float(tf_) - first) < 1e-12 and abs(float(ts) - second) < tol and abs(float(tl) - loss) < tol
    got = np.concatenate([x.numpy().reshape(-1) for x in grads])
    assert np.max(np.abs(got - ref)) <= 1e-9 * max(1.0, np.abs(ref).max())
    assert 1.0 <= 1.0 / np.sum(c * c) <= ng


def test_no_weights_and_zero_weights_give_the_old_loss():
    net, rs, (ds, da, gs, ga) = _case('l1l2', seed=3)
    rd, rg = net(torch.tensor(ds), torch.tensor(da)), net(torch.tensor(gs), torch.tensor(ga))
    reg = net.regularization()
    first = -1.0 / 5 * rd.sum()
    second = torch.log(1.0 / 4 * torch.exp(rg.reshape(4, 15).sum(1)).sum())
    old = (first + second + reg, first, second)
    for a, b in zip(maxent_irl_loss(rd, rg, 5, 4, reg), old):                       # None: the expression it always was
        assert torch.equal(a, b)
    for a, b in zip(maxent_irl_loss(rd, rg, 5, 4, reg, log_z=None), old):
        assert torch.equal(a, b)
    for a, b in zip(maxent_irl_loss(rd, rg, 5, 4, reg, log_z=torch.zeros(4, dtype=torch.float64)), old):
        assert abs(a.item() - b.item()) <= 1e-14 * max(1.0, abs(b.item()))
    # a constant ln z shifts the second term and leaves the gradient alone
    g0 = torch.autograd.grad(old[0], list(net.parameters()), retain_graph=True)
    lc, _, sc = maxent_irl_loss(rd, rg, 5, 4, reg, log_z=torch.full((4,), -5700.0, dtype=torch.float64))
    assert abs(sc.item() - (second.item() - 5700.0)) <= 1e-11
    g1 = torch.autograd.grad(lc, list(net.parameters()))
    for x, y in zip(g0, g1):
        assert torch.allclose(x, y, rtol=1e-10, atol=1e-14)


def test_fp32_rewards_keep_their_dtype_and_the_fp64_weights():
    """fp32 rewards with fp64 ln z (the autograd fall-back of AC_IRL.update_reward): the weights are formed in fp64 -- an fp32
    ln z of 5.7e3 carries 5e-4 -- and the loss comes back in the rewards' dtype."""
    rs = np.random.RandomState(0)
    rg = torch.tensor(rs.randn(60).astype(np.float32) * 0.1, requires_grad=True)
    rd = torch.tensor(rs.randn(30).astype(np.float32) * 0.1)
    lz = -5700.0 + rs.randn(4)
    loss, _, second = maxent_irl_loss(rd, rg, 5, 4, log_z=torch.tensor(lz))
    assert loss.dtype == torch.float32 and second.dtype == torch.float32
    D = rg.detach().double().numpy().reshape(4, 15).sum(1) + lz
    c = np.exp(D - D.max()); c /= c.sum()
    g, = torch.autograd.grad(loss, rg)
    assert np.max(np.abs(g.numpy().reshape(4, 15) - c[:, None])) <= 4e-7      # (fp32 storage of c <= 1; an fp32 ln z: ~5e-4)
    assert abs(second.item() - (D.max() + np.log(np.exp(D - D.max()).sum() / 4))) <= 5.7e3 * 2.0 ** -23


def test_classes_accept_the_keyword_and_default_to_off():
    from discrete_mean_field_game_amd import irl_population
    from discrete_mean_field_game_amd.ac_irl import AC_IRL
    from discrete_mean_field_game_amd.reward_learning import RewardTrainer
    for fn in (AC_IRL.__init__, irl_population.AC_IRLPopulation.__init__, irl_population.gridsearch):
        p = inspect.signature(fn).parameters['importance_weights']
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is False, fn
    assert inspect.signature(RewardTrainer.step).parameters['gen_log_z'].default is None
    assert inspect.signature(maxent_irl_loss).parameters['log_z'].default is None
    for cls in (AC_IRL, irl_population.AC_IRLPopulation):
        assert callable(getattr(cls, 'importance_log_weights'))
    # the flag is a constructor argument and derived state: the checkpoint keeps its keys
    src = inspect.getsource(AC_IRL.state_dict)
    assert 'importance' not in src and '_lz' not in src


def test_new_entry_points_are_declared_bound_and_exported():
    from discrete_mean_field_game_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'mfg_hip.h')).read(), flags=re.S)
    handle = _lib.lib()
    for name in NEW_SYMBOLS:
        decl = re.search(r'\b%s\s*\(([^;]*)\)\s*;' % name, text)
        assert decl, name
        assert len(decl.group(1).split(',')) == len(_lib.SIGNATURES[name][1]), name
        assert getattr(handle, name) is not None
    # additions only: the weighted calls are the unweighted ones plus gen_log_z in front of the stream
    for name in ('mfg_reward_net_train_step', 'mfg_reward_net_train_steps_pop'):
        assert len(_lib.SIGNATURES[name + '_z'][1]) == len(_lib.SIGNATURES[name][1]) + 1
    assert handle.mfg_abi_version() == 18
