#!/usr/bin/env python3
"""GPU: the reward sensitivities of a sweep-sized IRL population -- AC_IRLPopulation.reward_sensitivity(), the mean of d r / d pi
and d r / d P (and of gradient x input) over the four reward sets, formed on the device by the reward input-gradient block
that rides on mfg_reward_net_forward_pop -- against what a user had to do before: the same four sets through
torch.autograd.grad on networks.RewardNet copies of the weights, learner by learner, on the same device.  27 learners (the
reference's 3 x 3 x 3 grid), d = 15, 20 training and 10 test demonstrations, batch 32.  Both sides run the same two generations
and evaluate every network with keep_prob = 1; both end in one host read of the means.

Timing: wall clock around whole calls, a warm-up of both, then --reps repetitions alternating the sides; median and spread
(min .. max).  The two sides' means are first compared (fp32 evaluations of the same function: they agree to ~1e-6 of the
largest entry, not bit for bit).  Kernel times: a `rocprofv3 --kernel-trace --stats` run of this script on its own.
python tools/reward_grad_probe.py [--reps 7] [--out FILE]     (default: profiles/reward_grad.txt)"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from discrete_mean_field_game_amd import irl_population as ip  # noqa: E402
from discrete_mean_field_game_amd import ops  # noqa: E402

D, T, BATCH, N_TRAIN, N_TEST = 15, 15, 32, 20, 10


def demos(n, seed):
    rs = np.random.RandomState(seed)
    return [[(rs.dirichlet(np.ones(D)), rs.dirichlet(np.ones(D), size=D)) for _ in range(T)] for _ in range(n)]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles',
                                                  'reward_grad.txt'), help='the table is also written to this file')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('reward_grad_probe needs a GPU')
    ops.init()
    dev = torch.device('cuda', torch.cuda.current_device())
    points = ip.gridsearch_points(('dropout', 'l1l2', 'dropout_l1l2'), range(4, 10, 2), range(4, 10, 2))
    K = len(points)
    rs = np.random.RandomState(3)
    table, table_test = rs.dirichlet(np.ones(D), size=20), rs.dirichlet(np.ones(D), size=10)
    pop = ip.AC_IRLPopulation(np.linspace(8.0, 9.0, K), 0.16, 1e4, D, batch=BATCH, reward_nets=ip.gridsearch_nets(points, D, 0),
                              seeds=list(range(K)), pi0=table, device=dev, demonstrations=demos(N_TRAIN, 5),
                              demonstrations_test=demos(N_TEST, 8), mixed_nets=True)
    pop.train(1, 0.9)
    tt_dev = torch.as_tensor(table_test.astype(np.float32), device=dev)
    n = N_TRAIN * T
    test_dev = (torch.from_numpy(pop._test_np[0]).reshape(-1, D).contiguous().to(dev),
                torch.from_numpy(pop._test_np[1]).reshape(-1, D, D).contiguous().to(dev))
    nets = []
    for k in range(K):
        net = pop.reward_net(k)
        net.use_dropout = False                      # keep_prob = 1, as reward_sensitivity(dropout=False)
        nets.append(net)

    def new_side():
        return pop.reward_sensitivity(pi0_test=table_test)

    def old_side(advance=True):
        prev = pop._ctx.bind_scoped()
        try:
            saved = (pop._rng_step, pop._gen_traj_counter)
            inputs = [tuple(t.expand(K, *t.shape) for t in pop._demo_store.gather_flat()),
                      tuple(t.expand(K, *t.shape) for t in test_dev)]
            for tab in (None, tt_dev):
                st, ac = pop._generate(N_TRAIN, mat_dev=tab)
                inputs.append((st[:, :, :T].reshape(K, n, D), ac.reshape(K, n, D, D)))
            if not advance:
                pop._rng_step, pop._gen_traj_counter = saved
        finally:
            pop._ctx.restore(prev)
        out = []
        for st, ac in inputs:
            for k in range(K):
                s = st[k].detach().clone().requires_grad_(True)
                a = ac[k].detach().clone().requires_grad_(True)
                gs, ga = torch.autograd.grad(nets[k](s, a).sum(), (s, a))
                gs, ga, sd, ad = gs.double(), ga.double(), s.detach().double(), a.detach().double()
                out.append(torch.cat([gs.mean(0).reshape(-1), (gs * sd).mean(0).reshape(-1), ga.mean(0).reshape(-1),
                                      (ga * ad).mean(0).reshape(-1)]))
        return torch.stack(out).cpu().numpy().reshape(4, K, -1)         # the one host read

    # the two sides on the same sets (the old side first, without moving the counters)
    ref = old_side(advance=False)
    got = new_side()
    new = np.concatenate([got.grad_state.reshape(K, 4, -1), got.gxi_state.reshape(K, 4, -1), got.grad_action.reshape(K, 4, -1),
                          got.gxi_action.reshape(K, 4, -1)], axis=2).transpose(1, 0, 2)
    gap = float(np.abs(new - ref).max() / np.abs(ref).max())

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    sides = {'new': new_side, 'old': old_side}
    for fn in sides.values():
        wall(fn), wall(fn)
    t = {name: [] for name in sides}
    for _ in range(args.reps):
        for name, fn in sides.items():
            t[name].append(wall(fn))
    cell = lambda v: '%9.3f (%9.3f .. %9.3f)' % (np.median(v), min(v), max(v))
    lines = ['reward_sensitivity(), K = %d learners, d = %d, %d / %d demonstrations (%d / %d transitions per set); ms per call, '
             'median (min .. max) of %d alternating repetitions' % (K, D, N_TRAIN, N_TEST, n, N_TEST * T, args.reps),
             '  input-gradient block on mfg_reward_net_forward_pop, means on the device : %s' % cell(t['new']),
             '  torch.autograd.grad on networks.RewardNet copies, learner by learner    : %s' % cell(t['old']),
             '  ratio old / new                                                         : %.2f'
             % (np.median(t['old']) / np.median(t['new'])),
             '  (both sides include the same two generations and end in one host read)',
             '  largest difference of the two sides\' means, relative to the largest entry: %.2e' % gap]
    print('\n'.join(lines), flush=True)
    with open(args.out, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
