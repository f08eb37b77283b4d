#!/usr/bin/env python3
"""GPU: the reward-distribution diagnostics of a sweep-sized IRL population -- AC_IRLPopulation.reward_distribution() +
action_heatmap(), reduced on the device -- against the same numbers computed per learner on the host with NumPy and SciPy from
downloaded rewards and actions (what a user had to do before: np.histogram, scipy.stats.gaussian_kde on 200 points, the three
JSDs, np.mean of the fp64 copy of the actions).  27 learners (the reference's 3 x 3 x 3 grid), d = 15, 20 training and 10 test
demonstrations, batch 32.  Both sides run the same generations and reward-network forwards; they differ in what follows.

Timing: wall clock around whole calls (both sides end in a host read), a warm-up of both, then --reps repetitions alternating
the sides; median and spread (min .. max).  The device statistics are first checked against the host's on the call's own
rewards.  Then mfg_row_distribution and mfg_action_mean_pop alone, device events around --iters back-to-back calls: the mean
action in GB/s of input read, next to the 6.0 TB/s the given-P step kernel reaches.
python tools/reward_dist_probe.py [--reps 7] [--iters 20] [--out FILE]     (default: profiles/reward_dist.txt)"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from discrete_mean_field_game_amd import irl_population as ip  # noqa: E402
from discrete_mean_field_game_amd import ops, reward_dist  # noqa: E402
from discrete_mean_field_game_amd.reward_learning import RN_SEED_OFFSET, philox_call_key  # noqa: E402

D, T, BATCH, N_TRAIN, N_TEST = 15, 15, 32, 20, 10
BINS, XMIN, XMAX, POINTS = 20, -0.1, 0.4, 200


def demos(n, seed):
    rs = np.random.RandomState(seed)
    return [[(rs.dirichlet(np.ones(D)), rs.dirichlet(np.ones(D), size=D)) for _ in range(T)] for _ in range(n)]


def host_statistics(rewards, actions, demo_actions):
    """Per learner on the host, from downloaded fp32 arrays: rewards four [K, N_s], actions [K, n, d, d], demo_actions [n, d, d]."""
    from scipy.stats import gaussian_kde
    K = rewards[0].shape[0]
    xs = np.linspace(XMIN, XMAX, POINTS)
    out = []
    demo_avg = np.mean(demo_actions.astype(np.float64), axis=0)
    for k in range(K):
        hist, dens = [], []
        for r in rewards:
            x = r[k].astype(np.float64)
            hist.append(np.histogram(x, BINS))
            dens.append(gaussian_kde(x)(xs))
        jsd = [reward_dist.host_jsd(hist[a][0], hist[b][0]) for a, b in reward_dist.JSD_PAIRS]
        gen_avg = np.mean(actions[k].astype(np.float64), axis=0)
        out.append((hist, dens, jsd, gen_avg, np.abs(demo_avg - gen_avg)))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles',
                                                  'reward_dist.txt'), help='the table is also written to this file')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('reward_dist_probe needs a GPU')
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

    def device_side():
        return pop.reward_distribution(pi0_test=table_test), pop.action_heatmap()

    def host_side():
        prev = pop._ctx.bind_scoped()
        try:
            active = list(range(K))
            inputs = [pop._demo_store.gather_flat(), pop._test_dev]
            for tab in (None, tt_dev):
                st, ac = pop._generate(N_TRAIN, mat_dev=tab)
                inputs.append((st[:, :, :T].reshape(K, n, D).contiguous(), ac.reshape(K, n, D, D)))
            _, heat_actions = pop._generate(N_TRAIN)
            rewards = []
            for st, ac in inputs:
                pop._calls_k[active] += 1
                keys = [philox_call_key(pop.seeds[k], RN_SEED_OFFSET, pop._calls_k[k]) for k in active]
                rewards.append(pop._forward(st, ac, active, keys))
            rewards = [r.cpu().numpy() for r in rewards]
            actions = heat_actions.reshape(K, n, D, D).cpu().numpy()
            demo_actions = inputs[0][1].cpu().numpy()
        finally:
            pop._ctx.restore(prev)
        return host_statistics(rewards, actions, demo_actions)

    # the device's statistics against the host's, on the call's own rewards
    got = pop.reward_distribution(pi0_test=table_test, want_rewards=True)
    ref = host_statistics(got.rewards, np.zeros((K, 1, D, D), np.float32), np.zeros((1, D, D), np.float32))
    for k in range(K):
        hist, dens, jsd = ref[k][:3]
        for s in range(4):
            assert np.array_equal(got.counts[k, s], hist[s][0]) and np.array_equal(got.edges[k, s], hist[s][1]), (k, s)
            np.testing.assert_allclose(got.density[k, s], dens[s], rtol=1e-11, atol=1e-300)
        assert np.array_equal(got.jsd[k], jsd)

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    sides = {'device': device_side, 'host': host_side}
    for fn in sides.values():
        wall(fn), wall(fn)
    t = {name: [] for name in sides}
    for _ in range(args.reps):
        for name, fn in sides.items():
            t[name].append(wall(fn))
    cell = lambda v: '%9.3f (%9.3f .. %9.3f)' % (np.median(v), min(v), max(v))
    lines = ['reward_distribution() + action_heatmap(), K = %d learners, d = %d, %d / %d demonstrations (%d / %d transitions per '
             'set), %d bins, %d KDE points; ms per call pair, median (min .. max) of %d alternating repetitions'
             % (K, D, N_TRAIN, N_TEST, n, N_TEST * T, BINS, POINTS, args.reps),
             '  reduced on the device, one host read per call : %s' % cell(t['device']),
             '  downloaded, NumPy + SciPy per learner         : %s' % cell(t['host']),
             '  ratio host / device                           : %.2f' % (np.median(t['host']) / np.median(t['device'])),
             '  (both sides include the same three generations and four population forwards)', '']

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        fn()
        a.record()
        for _ in range(args.iters):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / args.iters

    lines.append('mfg_row_distribution alone (one launch), %d bins; ms per call, median (min .. max) of %d x %d calls'
                 % (BINS, args.reps, args.iters))
    for R, N, G in ((K, n, POINTS), (K, n, 0), (K, 70001, POINTS), (K, 70001, 0)):
        v = torch.tanh(0.3 * torch.randn(R, N, device=dev))
        out = ops.row_distribution(v, bins=BINS, G=G, x_lo=XMIN, x_hi=XMAX)
        ts = [timed(lambda: ops.row_distribution(v, bins=BINS, G=G, x_lo=XMIN, x_hi=XMAX, out=out)) for _ in range(args.reps)]
        lines.append('  R = %3d, N = %6d, G = %3d : %s' % (R, N, G, cell(ts)))
    lines += ['', 'mfg_action_mean_pop alone (two launches); ms per call, median (min .. max) of %d x %d calls, and GB/s of input '
              'read (the given-P step kernel: 6.0 TB/s)' % (args.reps, args.iters)]
    for Kk, N, d in ((K, n, D), (K, 30000, D), (8, 4096, 64)):
        a = torch.rand(Kk, N, d, d, device=dev)
        out = ops.action_mean_pop(a)
        ts = [timed(lambda: ops.action_mean_pop(a, out=out)) for _ in range(args.reps)]
        nbytes = Kk * N * d * d * 4
        lines.append('  K = %3d, N = %6d, d = %2d (%7.1f MB) : %s  %8.1f GB/s' % (Kk, N, d, nbytes / 1e6, cell(ts),
                                                                                nbytes / (np.median(ts) * 1e-3) / 1e9))
    print('\n'.join(lines), flush=True)
    with open(args.out, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
