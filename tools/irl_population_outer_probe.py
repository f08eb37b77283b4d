#!/usr/bin/env python3
"""GPU: the reward half of an AC_IRLPopulation (per-learner reward networks) against K sequential AC_IRL learners of the
same settings, wall-clock (both sides read the host at every reward_iteration check):
  * reward_iteration(100, stop_criteria=-1): 100 update_reward steps + 10 checks of every learner;
  * one outer iteration: outerloop(1, max_reward_iterations=100, max_forward_episodes=E, final_training=False) -- D_samp
    generation, reward_iteration (stop 1e-4, its own stop per learner) and the forward solve.
python tools/irl_population_outer_probe.py [--K 16] [--batch 4096] [--d 21] [--episodes 200] [--repeat 3]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from discrete_mean_field_game_amd import ops  # noqa: E402
from discrete_mean_field_game_amd.networks import RewardNet  # noqa: E402
from discrete_mean_field_game_amd.irl_population import AC_IRLPopulation  # noqa: E402


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def make(mode, d, K, B, dev):
    torch.manual_seed(0)
    nets = [RewardNet(d=d).to(dev) for _ in range(K)]
    rs = np.random.RandomState(1)
    demos = [[(rs.dirichlet(np.ones(d)), rs.dirichlet(np.ones(d), size=d)) for _ in range(15)] for _ in range(20)]
    mat = rs.dirichlet(np.ones(d), size=64)
    return AC_IRLPopulation(np.linspace(8.4, 8.9, K), 0.0, 1e4, d, batch=B, reward_nets=nets, seeds=np.arange(K), pi0=mat,
                            update_every=mode, device=dev, demonstrations=demos, lr_reward=1e-4)


def probe(mode, d, K, B, E, repeat, dev):
    rows = []
    for _ in range(repeat):
        pop = make(mode, d, K, B, dev)
        pop._gen_store.push(*pop._generate(50))
        singles = [pop.learner(k) for k in range(K)]
        pop.reward_iteration(10, -1, 10)                      # warm-up (allocations, first launches)
        for ac in singles:
            ac.reward_iteration(10, -1, 10)
        t_pop = wall(lambda: pop.reward_iteration(100, -1, 10))
        t_seq = wall(lambda: [ac.reward_iteration(100, -1, 10) for ac in singles])
        pop2 = make(mode, d, K, B, dev)
        singles2 = [pop2.learner(k) for k in range(K)]
        o_pop = wall(lambda: pop2.outerloop(1, 5, 100, E, final_training=False))
        o_seq = wall(lambda: [ac.outerloop(1, 5, 100, E, final_training=False) for ac in singles2])
        rows.append((t_pop, t_seq, o_pop, o_seq))
    t_pop, t_seq, o_pop, o_seq = np.median(np.array(rows), axis=0)
    print('%-7s d=%2d K=%2d Bk=%5d  reward_iteration(100): population %.1f ms, %d sequential %.1f ms, gain %.2fx   '
          'one outer iteration (%d forward episodes): population %.1f ms, sequential %.1f ms, gain %.2fx   (median of %d)'
          % (mode, d, K, B, t_pop, K, t_seq, t_seq / t_pop, E, o_pop, o_seq, o_seq / o_pop, repeat), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--K', type=int, default=16)
    ap.add_argument('--batch', type=int, default=4096)
    ap.add_argument('--d', type=int, default=21)
    ap.add_argument('--episodes', type=int, default=200)
    ap.add_argument('--repeat', type=int, default=3)
    ap.add_argument('--modes', default='step,rollout')
    args = ap.parse_args()
    ops.init()
    dev = torch.device('cuda', 0)
    for mode in args.modes.split(','):
        probe(mode, args.d, args.K, args.batch, args.episodes, args.repeat, dev)


if __name__ == '__main__':
    main()
