#!/usr/bin/env python3
"""GPU: the population selection step against the point-by-point paths, wall-clock with the device synchronised (both sides read
the test files, evaluate on the device, copy the metrics to the host and append their CSV lines):
  * population.gridsearch (one mfg_evaluate_pop call per GRID_CHUNK points) against actor_critic.gridsearch (one rollout, one
    JSD and the torch reductions per point) on grids of 8, 125 and 1 000 points (8 000 for the population path only);
  * ActorCriticPopulation.evaluate at K learners against K sequential learner(k).evaluate calls.
N synthetic test files of 16 rows each; every number is the median of --repeat runs after a warm-up run.
python tools/eval_pop_probe.py [--d 21,15] [--files 5] [--repeat 3]"""
import argparse
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from discrete_mean_field_game_amd import ops, population  # noqa: E402
from discrete_mean_field_game_amd.mfg_ac2 import actor_critic  # noqa: E402
from discrete_mean_field_game_amd.population import ActorCriticPopulation  # noqa: E402

INDIR = 'test_normalized_round2'


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def median(fn, repeat):
    fn()                                  # warm-up (allocations, first launches, occupancy queries)
    return float(np.median([wall(fn) for _ in range(repeat)]))


def grid(n):
    return np.linspace(6.0, 10.0, n).tolist(), np.linspace(0.1, 0.5, n).tolist(), np.linspace(8000.0, 14000.0, n).tolist()


def probe_grid(d, side, repeat, with_seq, dev):
    th, sh, al = grid(side)
    npts = side ** 3
    t_pop = median(lambda: population.gridsearch(th, sh, al, INDIR, 'pop.csv', d=d, device=dev), repeat)
    line = 'gridsearch d=%2d points=%5d  population %9.2f ms' % (d, npts, t_pop)
    if with_seq:
        ac = actor_critic(d=d, pi0=np.full((1, d), 1.0 / d), seed=0, verbose=0, device=dev)
        t_seq = median(lambda: ac.gridsearch(th, sh, al, INDIR, 'seq.csv'), repeat)
        line += '   actor_critic.gridsearch %9.2f ms   gain %6.1fx' % (t_seq, t_seq / t_pop)
    else:
        line += '   actor_critic.gridsearch  not run'
    print(line, flush=True)


def probe_evaluate(d, K, repeat, dev):
    rs = np.random.RandomState(3)
    pop = ActorCriticPopulation(np.linspace(6.0, 10.0, K), 0.3, 1e4, d, batch=2, seeds=np.arange(K), pi0=rs.dirichlet(np.ones(d),
                                size=16), w0=np.zeros(d * (d + 1) // 2 + d + 1), device=dev)
    learners = [pop.learner(k) for k in range(K)]
    th = pop.thetas
    t_pop = median(lambda: pop.evaluate(outfile='pop.csv'), repeat)
    t_seq = median(lambda: [ac.evaluate(float(th[k]), 0.3, 1e4, d, outfile='seq.csv') for k, ac in enumerate(learners)], repeat)
    print('evaluate   d=%2d K=%5d       population %9.2f ms   %d x learner(k).evaluate %9.2f ms   gain %6.1fx'
          % (d, K, t_pop, K, t_seq, t_seq / t_pop), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--d', default='21,15')
    ap.add_argument('--files', type=int, default=5)
    ap.add_argument('--repeat', type=int, default=3)
    ap.add_argument('--sides', default='2,5,10,20')        # grid points = side^3
    ap.add_argument('--seq-max', type=int, default=1000)   # largest grid the point-by-point path is timed on
    ap.add_argument('--K', default='16,256')
    args = ap.parse_args()
    ops.init()
    dev = torch.device('cuda', 0)
    home = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        os.makedirs(INDIR)
        for d in [int(v) for v in args.d.split(',')]:
            for f in os.listdir(INDIR):
                os.remove(os.path.join(INDIR, f))
            rs = np.random.RandomState(d)
            for j in range(args.files):
                np.savetxt('%s/trend_distribution_day%d.csv' % (INDIR, 22 + j), rs.dirichlet(np.ones(d), size=16), fmt='%.3e',
                           delimiter=' ')
            for side in [int(v) for v in args.sides.split(',')]:
                probe_grid(d, side, args.repeat, side ** 3 <= args.seq_max, dev)
            for K in [int(v) for v in args.K.split(',')]:
                probe_evaluate(d, K, args.repeat, dev)
        os.chdir(home)       # (out of the directory before it goes: a profiler writes its output relative to the cwd at exit)


if __name__ == '__main__':
    main()
