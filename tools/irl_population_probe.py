#!/usr/bin/env python3
"""GPU: a population of K IRL forward learners (ops.train_episodes_irl_pop / train_rollouts_irl_pop, per-learner reward
networks) against K sequential single-learner native IRL calls (ops.train_episode_irl with the device start draw /
ops.train_rollout_irl) of the same shapes: event-timed ms per episode (all K learners) and aggregate env-steps/s.
python tools/irl_population_probe.py [--episodes 10] [--warmup 3] [--quick]"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from discrete_mean_field_game_amd import ops  # noqa: E402
from discrete_mean_field_game_amd.networks import RewardNet  # noqa: E402
from discrete_mean_field_game_amd.irl_population import AC_IRLPopulation  # noqa: E402


def timed(fn, E, warmup):
    fn(warmup)
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    fn(E)
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / E


def probe(mode, d, K, B, T, E, warmup, dev):
    torch.manual_seed(0)
    nets = [RewardNet(d=d).to(dev) for _ in range(K)]
    mat = np.random.RandomState(0).dirichlet(np.ones(d), size=64)
    pop = AC_IRLPopulation(np.full(K, 8.64), 0.0, 1e4, d, batch=B, reward_nets=nets, seeds=np.arange(K), w0=np.zeros(ops.num_features(d)),
                           pi0=mat, update_every=mode, device=dev)
    b = pop._buffers()
    lr0 = torch.zeros(K, dtype=torch.float64, device=dev)
    mat_dev = pop._mat_pi0_dev

    def run_pop(n):
        if mode == 'step':
            ops.train_episodes_irl_pop(mat_dev, b['pi'], T, n, 1, 1, pop._theta, pop._shifts_dev, pop._alphas_dev, pop._w, 1.0,
                                       lr0, lr0, pop._seeds_dev, pop._net_struct, 1, pop._rn_seeds_dev, 0, b['G'], b['ws'],
                                       b['run'])
        else:
            ops.train_rollouts_irl_pop(mat_dev, T, n, 1, 1, pop._theta, pop._shifts_dev, pop._alphas_dev, pop._w, 1.0, lr0, lr0,
                                       pop._seeds_dev, pop._net_struct, 1, pop._rn_seeds_dev, 0, b['G'], b['ws'], b['run'])

    # the single calls: learner k's slices of the same buffers, its own network, the workspace AC_IRL allocates
    ws1 = [ops.workspace(B if mode == 'step' else B * T, d, dev) for _ in range(K)]
    r = b['run']

    def run_seq(n):
        for _ in range(n):
            for k in range(K):
                th = pop._theta[k:k + 1]
                if mode == 'step':
                    bufs = dict(scratch=r['scratch'][k], P=r['P'][k], reward=r['reward'][k], delta=r['delta'][k], g=r['g'][k])
                    ops.train_episode_irl(b['pi'][k], T, th, 0.0, 1e4, pop._w[k], 1.0, 0.0, 0.0, nets[k], b['G'][k], ws1[k], bufs,
                                          seed=k, rn_seed=k + 0x5EED, mat_pi0=mat_dev)
                else:
                    bufs = dict(pi_traj=r['pi_traj'][k], pi_last=r['pi_last'][k], P=r['P'][k], reward=r['reward'][k].view(-1),
                                delta=r['delta'][k].view(-1), g=r['g'][k].view(-1))
                    ops.train_rollout_irl(mat_dev, None, T, th, 0.0, 1e4, pop._w[k], 1.0, 0.0, 0.0, nets[k], b['G'][k], ws1[k],
                                          bufs, seed=k, rn_key=k + 0x5EED)
    t_pop, t_seq = timed(run_pop, E, warmup), timed(run_seq, E, warmup)
    steps = K * B * T
    print('%-7s d=%2d K=%2d Bk=%5d  population %.4f ms/episode %.3e env-steps/s   sequential %.4f ms/episode %.3e env-steps/s'
          '   gain %.2fx' % (mode, d, K, B, t_pop, steps / t_pop * 1e3, t_seq, steps / t_seq * 1e3, t_seq / t_pop), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--episodes', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--quick', action='store_true', help='only d = 21, K = 16, Bk = 4 096 (for a kernel-trace run)')
    args = ap.parse_args()
    ops.init()
    dev = torch.device('cuda', 0)
    shapes = [(21, 16, 4096)] if args.quick else [(21, 16, 4096), (21, 16, 1024), (21, 4, 4096), (15, 16, 4096)]
    for mode in ('step', 'rollout'):
        for d, K, B in shapes:
            probe(mode, d, K, B, 15, args.episodes, args.warmup, dev)


if __name__ == '__main__':
    main()
