#!/usr/bin/env python3
"""GPU: a population of K learners (ops.train_episodes_pop / train_rollouts_pop) against K sequential single-learner calls
(ops.train_episodes / train_rollouts) of the same shapes: event-timed ms per episode (all K learners) and aggregate
env-steps/s.  python tools/population_probe.py [--episodes 20] [--warmup 5]"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from discrete_mean_field_game_amd import ops, _lib as L  # noqa: E402


def bufs_for(mode, K, B, d, T, dev):
    z = lambda *s, dt=torch.float64: torch.zeros(*s, dtype=dt, device=dev)
    if mode == 'step':
        return dict(scratch=z(K, B, d, dt=torch.float32), reward=z(K, B, dt=torch.float32), delta=z(K, B), g=z(K, B))
    return dict(pi_traj=z(K, B, T + 1, d, dt=torch.float32), reward=z(K, B, T, dt=torch.float32), delta=z(K, B, T), g=z(K, B, T))


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
    F = d * (d + 1) // 2 + d + 1
    rs = np.random.RandomState(0)
    mat = torch.as_tensor(rs.dirichlet(np.ones(d), size=64).astype(np.float32), device=dev)
    sb = (int(L.lib().mfg_workspace_bytes(B * T, d)) + 255) // 256 * 256
    th, w = torch.full((K,), 8.86349, dtype=torch.float64, device=dev), torch.zeros(K, F, dtype=torch.float64, device=dev)
    G, ws = torch.zeros(K, F + 3, dtype=torch.float64, device=dev), torch.zeros(K, sb // 8, dtype=torch.float64, device=dev)
    v = lambda x: torch.full((K,), x, dtype=torch.float64, device=dev)
    seeds = torch.arange(K, dtype=torch.int64, device=dev)
    b = bufs_for(mode, K, B, d, T, dev)
    pi = torch.zeros(K, B, d, dtype=torch.float32, device=dev)

    def pop(n):
        if mode == 'step':
            ops.train_episodes_pop(mat, pi, T, n, 0, 1, th, v(0.16), v(12000.0), w, 1.0, v(0.0), v(0.0), seeds, G, ws, b)
        else:
            ops.train_rollouts_pop(mat, T, n, 0, 1, th, v(0.16), v(12000.0), w, 1.0, G, ws, b, v(0.0), v(0.0), seeds)

    def seq(n):
        for _ in range(n):
            for k in range(K):
                if mode == 'step':
                    ops.train_episodes(mat, pi[k], T, 1, 0, 1, th[k:k + 1], 0.16, 12000.0, w[k], 1.0, 0.0, 0.0, G[k], ws[k],
                                       dict(scratch=b['scratch'][k], reward=b['reward'][k], delta=b['delta'][k], g=b['g'][k]),
                                       seed=k)
                else:
                    ops.train_rollouts(mat, T, 1, 0, 1, th[k:k + 1], 0.16, 12000.0, w[k], 1.0, G[k], ws[k],
                                       dict(pi_traj=b['pi_traj'][k], reward=b['reward'][k], delta=b['delta'][k], g=b['g'][k]),
                                       0.0, 0.0, seed=k)
    t_pop, t_seq = timed(pop, E, warmup), timed(seq, E, warmup)
    steps = K * B * T
    print('%-7s d=%2d K=%2d Bk=%5d  population %.4f ms/episode %.3e env-steps/s   sequential %.4f ms/episode %.3e env-steps/s'
          '   gain %.2fx' % (mode, d, K, B, t_pop, steps / t_pop * 1e3, t_seq, steps / t_seq * 1e3, t_seq / t_pop), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--episodes', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--quick', action='store_true', help='only d = 21, K = 16, Bk = 4 096 (for a kernel-trace run)')
    args = ap.parse_args()
    ops.init()
    dev = torch.device('cuda', 0)
    shapes = [(21, 16, 4096)] if args.quick else [(21, K, B) for K in (1, 4, 16) for B in (1024, 4096)] + [(15, 16, 4096)]
    for mode in ('step', 'rollout'):
        for d, K, B in shapes:
            probe(mode, d, K, B, 15, args.episodes, args.warmup, dev)


if __name__ == '__main__':
    main()
