#!/usr/bin/env python3
"""GPU: the reference's sweep gridsearch.py:8-31 (reg x n_fc3 x n_fc4 = 27 points) as ONE mixed AC_IRLPopulation against 27
sequential AC_IRL learners of the same settings, wall-clock (both sides read the host at every reward_iteration check):
  * reward_iteration(100, stop_criteria=-1): 100 update_reward steps + 10 checks of every point;
  * one outer iteration: outerloop(1, max_reward_iterations=100, max_forward_episodes=E, final_training=False).
With --uniform the 27 networks all have the reference's default shape (dropout_l1l2, 8, 4) and the population is built twice,
with and without the geometry table: what the table itself costs.
python tools/irl_pop_mixed_probe.py [--batch 4096] [--d 21,15] [--episodes 200] [--repeat 3] [--modes step,rollout]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from discrete_mean_field_game_amd import irl_population as ip  # noqa: E402
from discrete_mean_field_game_amd import ops  # noqa: E402

GRID = (('dropout', 'l1l2', 'dropout_l1l2'), range(4, 10, 2), range(4, 10, 2))


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def make(mode, d, points, B, dev, mixed=True):
    nets = [n.to(dev) for n in ip.gridsearch_nets(points, d)]
    K = len(points)
    rs = np.random.RandomState(1)
    demos = [[(rs.dirichlet(np.ones(d)), rs.dirichlet(np.ones(d), size=d)) for _ in range(15)] for _ in range(20)]
    mat = rs.dirichlet(np.ones(d), size=64)
    return ip.AC_IRLPopulation([6.5] * K, 0.0, 1e4, d, batch=B, reward_nets=nets, seeds=np.arange(K), pi0=mat,
                               update_every=mode, device=dev, demonstrations=demos, lr_reward=1e-4, mixed_nets=mixed)


def probe(mode, d, points, B, E, repeat, dev, sequential=True, mixed=True, tag='mixed'):
    rows = []
    K = len(points)
    for _ in range(repeat):
        pop = make(mode, d, points, B, dev, mixed)
        pop._gen_store.push(*pop._generate(50))
        singles = [pop.learner(k) for k in range(K)] if sequential else []
        pop.reward_iteration(10, -1, 10)                      # warm-up (allocations, first launches)
        for ac in singles:
            ac.reward_iteration(10, -1, 10)
        t_pop = wall(lambda: pop.reward_iteration(100, -1, 10))
        t_seq = wall(lambda: [ac.reward_iteration(100, -1, 10) for ac in singles])
        pop2 = make(mode, d, points, B, dev, mixed)
        singles2 = [pop2.learner(k) for k in range(K)] if sequential else []
        o_pop = wall(lambda: pop2.outerloop(1, 5, 100, E, final_training=False))
        o_seq = wall(lambda: [ac.outerloop(1, 5, 100, E, final_training=False) for ac in singles2])
        rows.append((t_pop, t_seq, o_pop, o_seq))
    t_pop, t_seq, o_pop, o_seq = np.median(np.array(rows), axis=0)
    if sequential:
        print('%-7s d=%2d K=%2d Bk=%5d %-8s reward_iteration(100): population %.1f ms, %d sequential %.1f ms, gain %.2fx   '
              'one outer iteration (%d forward episodes): population %.1f ms, sequential %.1f ms, gain %.2fx   (median of %d)'
              % (mode, d, K, B, tag, t_pop, K, t_seq, t_seq / t_pop, E, o_pop, o_seq, o_seq / o_pop, repeat), flush=True)
    else:
        print('%-7s d=%2d K=%2d Bk=%5d %-8s reward_iteration(100): population %.1f ms   one outer iteration (%d forward '
              'episodes): population %.1f ms   (median of %d)' % (mode, d, K, B, tag, t_pop, E, o_pop, repeat), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=4096)
    ap.add_argument('--d', default='21,15')
    ap.add_argument('--episodes', type=int, default=200)
    ap.add_argument('--repeat', type=int, default=3)
    ap.add_argument('--modes', default='step,rollout')
    ap.add_argument('--uniform', action='store_true', help='27 default-shaped networks, with and without the geometry table')
    ap.add_argument('--K', type=int, default=27, help='--uniform: population size')
    args = ap.parse_args()
    ops.init()
    dev = torch.device('cuda', 0)
    for d in [int(x) for x in args.d.split(',')]:
        for mode in args.modes.split(','):
            if args.uniform:
                points = [('dropout_l1l2', 8, 4)] * args.K
                probe(mode, d, points, args.batch, args.episodes, args.repeat, dev, False, True, 'table')
                probe(mode, d, points, args.batch, args.episodes, args.repeat, dev, False, False, 'shared')
            else:
                probe(mode, d, ip.gridsearch_points(*GRID), args.batch, args.episodes, args.repeat, dev)


if __name__ == '__main__':
    main()
