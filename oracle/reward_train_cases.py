"""Networks, trajectory stores and the batch-shape / reward-regime grid of the reward-network training-step tests.  TEST
INFRASTRUCTURE shared by tests/test_gpu_reward_train.py, tests/test_gpu_reward_train_shapes.py (GPU) and
tests/test_reward_learning.py (CPU: everything here runs on CPU tensors too, which is how the seeds below were chosen).

The grid walks the paths of rn_train_combine_body (csrc/mfg_reward_train.hip) that depend on the batch, not on the network:
  * N = (n_demo + n_gen) steps against the 152 column reads of one round (RT_CU x RT_WAVES), 256 (one r_mine slot) and 2048;
  * N n3 against the 2048 register-staged dz3 entries (RT_DZ x 256) and the tail loop behind them;
  * N (1 + n3) 4 B against the 60 KB of dynamic LDS;
  * the number of generated trajectories against the 64 lanes of the soft-max wave (1, 33, 63, 64, and 0);
  * the number of demonstration rewards against the 64 lanes of the first term's sum (0, < 64, > 64);
  * steps != 15 everywhere a transition index is split into (trajectory, step).
Every case must keep the oracle's `kink` (forward_cache) >= 1e-6: closer to a ReLU kink an fp32 evaluation may take the other
branch and no comparison means anything.  A clean draw is rare at 2048 samples x ~700 ReLU inputs (d = 15), so the cases of
1000 transitions and more run at d = 4 / 9; `seed` is the first network seed whose kink clears 3e-6 (found on the CPU with
`python -m oracle.reward_train_cases`, which prints the table)."""
from collections import namedtuple

import numpy as np
import torch

from oracle import reward_net_oracle as RO


def _net(d, reg, n3, n4, dev, k1=5, f2=2, k2=3, seed=0):
    from discrete_mean_field_game_amd.networks import RewardNet
    torch.manual_seed(seed)
    net = RewardNet(d=d, reg=reg, f1=1, k1=k1, f2=f2, k2=k2, n_fc3=n3, n_fc4=n4)
    with torch.no_grad():
        for p in net.parameters():
            p.add_(0.05 * torch.randn_like(p))          # biases away from zero, some negative weights
    return net.to(dev)


def _stores(d, n_demo, n_gen, dev, rs, T=15):
    """Two stores whose physical rows differ from the logical order (pushes with drops in between)."""
    from discrete_mean_field_game_amd.reward_learning import TrajectoryStore
    out = []
    for n in (n_demo, n_gen):
        st = TrajectoryStore(d, T, dev)
        junk = torch.as_tensor(rs.dirichlet(np.ones(d), size=(3, T)), dtype=torch.float32)
        junkP = torch.as_tensor(rs.dirichlet(np.ones(d), size=(3, T, d)), dtype=torch.float32)
        st.push(junk, junkP)
        s = torch.as_tensor(rs.dirichlet(np.ones(d) * 0.7, size=(n, T)), dtype=torch.float32)
        a = torch.as_tensor(rs.dirichlet(np.ones(d) * 0.5, size=(n, T, d)), dtype=torch.float32)
        st.push(s, a, drop=2)                            # logical: [junk2, new...]; rows of `new` reuse freed rows
        out.append(st)
    return out


def _batch_np(store, logical):
    s, a = store.gather(logical)
    d = store.d
    return s.reshape(-1, d).cpu().numpy().astype(np.float64), a.reshape(-1, d, d).cpu().numpy().astype(np.float64)


Case = namedtuple('Case', 'name family d n_demo n_gen steps n3 n4 reg gain seed')
DEMO_DIVISOR = 5                      # num_demo_samples of the reference (ac_irl.py:390), whatever the batch holds
REGS = ('none', 'l1l2', 'dropout_l1l2')

# (family, d, n_demo, n_gen, steps, n3, n4); reg alternates over REGS in this order
_SHAPES = [
    ('tiny', 15, 1, 1, 1, 8, 4),
    ('control', 21, 5, 5, 15, 8, 4),
    ('round', 15, 4, 4, 19, 8, 4),            # N = 152: the last batch one round of column reads serves
    ('round', 15, 9, 8, 9, 8, 4),             # N = 153: the first into the second round
    ('round', 15, 8, 8, 19, 8, 4),            # N = 304
    ('round', 21, 30, 31, 5, 8, 4),           # N = 305: the same edge one round later
    ('dz', 15, 8, 8, 16, 8, 4),               # N n3 = 2048 exactly (n3 = 8)
    ('dz', 15, 4, 4, 16, 16, 4),              # N n3 = 2048 exactly (n3 = 16)
    ('dz', 15, 21, 22, 6, 8, 4),              # N = 258, N n3 = 2064: 16 entries in the tail
    ('dz', 15, 5, 5, 13, 16, 8),              # N = 130, N n3 = 2080
    ('dz', 15, 6, 7, 11, 32, 8),              # n3 = 32: N n3 = 4576
    ('full', 9, 64, 64, 16, 6, 4),            # N = 2048: every r_mine slot
    ('full', 9, 64, 64, 15, 7, 4),            # N (1 + n3) 4 = 61440 B: the LDS limit exactly
    ('full', 4, 1, 1, 1024, 3, 2),            # one generated trajectory: its coefficient is 1 exactly
    ('lanes', 15, 3, 64, 7, 8, 4),
    ('lanes', 15, 64, 3, 7, 8, 4),
    ('lanes', 15, 2, 63, 5, 8, 4),
    ('lanes', 15, 2, 33, 5, 8, 4),
    ('empty', 15, 0, 6, 15, 8, 4),
    ('empty', 15, 6, 0, 15, 8, 4),
]
GAINS = (1e-3, 1.0, 8.0, 30.0)
_REGIMES = [('regime', 15, 5, 5, 15, 8, 4), ('regime', 9, 8, 8, 64, 8, 4)]

# network seeds: first seed >= 0 with kink >= 3e-6 on the CPU, keyed by (d, n_demo, n_gen, steps, n3, n4, reg)
_SEEDS = {
    (15, 1, 1, 1, 8, 4, 'none'): 0,    # kink 4.8e-04
    (21, 5, 5, 15, 8, 4, 'l1l2'): 0,    # kink 1.1e-05
    (15, 4, 4, 19, 8, 4, 'dropout_l1l2'): 0,    # kink 2.1e-05
    (15, 9, 8, 9, 8, 4, 'none'): 0,    # kink 3.5e-06
    (15, 8, 8, 19, 8, 4, 'l1l2'): 0,    # kink 1.7e-05
    (21, 30, 31, 5, 8, 4, 'dropout_l1l2'): 0,    # kink 5.3e-06
    (15, 8, 8, 16, 8, 4, 'none'): 3,    # kink 4.1e-06
    (15, 4, 4, 16, 16, 4, 'l1l2'): 0,    # kink 7.3e-06
    (15, 21, 22, 6, 8, 4, 'dropout_l1l2'): 0,    # kink 5.0e-06
    (15, 5, 5, 13, 16, 8, 'none'): 0,    # kink 6.6e-06
    (15, 6, 7, 11, 32, 8, 'l1l2'): 4,    # kink 2.1e-05
    (9, 64, 64, 16, 6, 4, 'dropout_l1l2'): 0,    # kink 6.3e-06
    (9, 64, 64, 15, 7, 4, 'none'): 1,    # kink 3.8e-06
    (4, 1, 1, 1024, 3, 2, 'l1l2'): 0,    # kink 5.6e-06
    (15, 3, 64, 7, 8, 4, 'dropout_l1l2'): 5,    # kink 1.2e-05
    (15, 64, 3, 7, 8, 4, 'none'): 5,    # kink 1.3e-05
    (15, 2, 63, 5, 8, 4, 'l1l2'): 0,    # kink 1.9e-05
    (15, 2, 33, 5, 8, 4, 'dropout_l1l2'): 0,    # kink 9.0e-06
    (15, 0, 6, 15, 8, 4, 'none'): 0,    # kink 2.9e-05
    (15, 6, 0, 15, 8, 4, 'l1l2'): 1,    # kink 2.8e-05
    (15, 5, 5, 15, 8, 4, 'none'): 0,    # kink 5.2e-06
    (15, 5, 5, 15, 8, 4, 'l1l2'): 0,    # kink 5.2e-06
    (15, 5, 5, 15, 8, 4, 'dropout_l1l2'): 0,    # kink 1.1e-05
    (9, 8, 8, 64, 8, 4, 'l1l2'): 0,    # kink 7.8e-06
    (9, 8, 8, 64, 8, 4, 'dropout_l1l2'): 0,    # kink 7.8e-06
    (9, 8, 8, 64, 8, 4, 'none'): 0,    # kink 7.8e-06
}


def _cases():
    out = []
    for i, (fam, d, nd, ng, T, n3, n4) in enumerate(_SHAPES):
        reg = REGS[i % 3]
        key = (d, nd, ng, T, n3, n4, reg)
        out.append(Case('%s-d%d-%dx%dx%d-n%d-%s' % (fam, d, nd, ng, T, n3, reg), fam, d, nd, ng, T, n3, n4, reg, 1.0, _SEEDS.get(key, 0)))
    for j, (fam, d, nd, ng, T, n3, n4) in enumerate(_REGIMES):
        for gi, gain in enumerate(GAINS):
            reg = REGS[(j + gi) % 3]
            key = (d, nd, ng, T, n3, n4, reg)
            out.append(Case('%s-d%d-%dx%dx%d-gain%g-%s' % (fam, d, nd, ng, T, gain, reg), fam, d, nd, ng, T, n3, n4, reg, gain,
                            _SEEDS.get(key, 0)))
    return out


CASES = _cases()


def dropout_seed(case):
    return 0xABCDEF0123 + 7 * case.steps + case.n_gen


def build(case, dev, dead_unit=None):
    """(net, demo store, gen store, logical demo indices, logical gen indices) of a case on device `dev` ('cpu' works).
    dead_unit: FC3 unit whose bias is set to -10, dead for every sample."""
    net = _net(case.d, case.reg, case.n3, case.n4, dev, seed=case.seed)
    with torch.no_grad():
        net.out.weight.mul_(case.gain)
        if dead_unit is not None:
            net.fc3.bias[dead_unit] = -10.0
    rs = np.random.RandomState(1000 * case.d + 10 * case.steps + case.n_demo)
    demo, gen = _stores(case.d, case.n_demo, case.n_gen, dev, rs, T=case.steps)
    # logical index 0 is a leftover of the first push; the batch is a permutation of the rest
    di = [int(i) + 1 for i in rs.permutation(case.n_demo)]
    gi = [int(i) + 1 for i in rs.permutation(case.n_gen)]
    return net, demo, gen, di, gi


def oracle_inputs(case, net, demo, gen, di, gi):
    """(params, demo states, demo actions, gen states, gen actions, masks) in the oracle's fp64 layouts."""
    ds, da = _batch_np(demo, di)
    gs, ga = _batch_np(gen, gi)
    N = (case.n_demo + case.n_gen) * case.steps
    masks = RO.dropout_masks(net.keep_prob, dropout_seed(case), 0, N, case.n3, case.n4) if net.use_dropout else None
    return RO.params_from_torch(net), ds, da, gs, ga, masks


def kink_of(case):
    net, demo, gen, di, gi = build(case, 'cpu')
    prm, ds, da, gs, ga, masks = oracle_inputs(case, net, demo, gen, di, gi)
    _, cache = RO.forward_cache(prm, np.concatenate([ds, gs], 0), np.concatenate([da, ga], 0), masks)
    return cache['kink']


if __name__ == '__main__':                    # the seed search: prints the _SEEDS table
    seen = {}
    for c in CASES:
        key = (c.d, c.n_demo, c.n_gen, c.steps, c.n3, c.n4, c.reg)
        if key in seen:
            continue
        best = (-1.0, 0)
        for seed in range(200):
            k = kink_of(c._replace(seed=seed))
            best = max(best, (k, seed))
            if k >= 3e-6:
                break
        seen[key] = best
        print('    %r: %d,    # kink %.1e' % (key, best[1], best[0]), flush=True)
