#!/usr/bin/env python3
"""GPU: ActorCriticPopulation.train() in step mode through the resident kernel (resident=True: one workgroup per learner,
ceil(episodes / 64) launches) against the per-step launches (resident=False: 1 + 2 T launches per episode), the same
population, alternating in one process.  Per shape: median / min / max ms per episode of each side over the repetitions, the
ratio of the medians and a verdict -- `resident` or `per-step` when the slower side's fastest repetition is still slower than
the faster side's slowest one (the difference exceeds the spread between repetitions of the same side), `tie` otherwise.
population.resident_rule follows this table.

    python tools/pop_resident_probe.py [--reps 5] [--out profiles/pop_resident_ab.txt]

train() ends with a device synchronisation (it reads the returns back), so the host clock around it times the work.  Learning
rates are 0: the parameters stay at the reference point however many episodes are timed."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from discrete_mean_field_game_amd import ActorCriticPopulation, ops  # noqa: E402

SHAPES = {21: (12, 48, 96, 192, 768), 15: (16, 64, 256, 1024)}
KS = (16, 256, 512, 4096)
T = 15


def population(K, d, Bk, resident, precision, table):
    return ActorCriticPopulation(np.full(K, 8.86349), 0.16, 12000, d, batch=Bk, seeds=np.arange(K), w0=np.zeros(d * (d + 1) // 2 + d + 1),
                                 pi0=table, resident=resident, precision=precision, episode_steps=T)


def ms_per_episode(pop, E):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    pop.train(E, constant=1, lr_critic=0.0, lr_actor=0.0)
    return (time.perf_counter() - t0) * 1e3 / E


def probe(K, d, Bk, precision, reps, target_ms, out):
    table = np.random.RandomState(0).dirichlet(np.ones(d), size=64)
    sides = {'resident': population(K, d, Bk, True, precision, table), 'per-step': population(K, d, Bk, False, precision, table)}
    # warm-up (code objects, buffers), then the episodes per timed call: enough work for `target_ms` on the faster side
    est = {name: min(ms_per_episode(p, 2), ms_per_episode(p, 2)) for name, p in sides.items()}
    E = int(min(64, max(4, np.ceil(target_ms / min(est.values())))))
    for p in sides.values():
        ms_per_episode(p, E)
    t = {name: [] for name in sides}
    for _ in range(reps):
        for name, p in sides.items():      # alternating
            t[name].append(ms_per_episode(p, E))
    r, s = np.array(t['resident']), np.array(t['per-step'])
    verdict = 'resident' if r.max() < s.min() else ('per-step' if s.max() < r.min() else 'tie')
    line = ('%-5s d=%2d K=%4d Bk=%4d E=%2d  resident %9.4f [%9.4f .. %9.4f]  per-step %9.4f [%9.4f .. %9.4f] ms/episode  '
            'per-step / resident %6.2fx  %s' % (precision, d, K, Bk, E, np.median(r), r.min(), r.max(), np.median(s), s.min(),
                                                s.max(), np.median(s) / np.median(r), verdict))
    print(line, flush=True)
    if out:
        out.write(line + '\n')
        out.flush()
    del sides
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--target-ms', type=float, default=60.0, help='work per timed train() call on the faster side')
    ap.add_argument('--out', default=None)
    ap.add_argument('--quick', action='store_true', help='K = 16 and 512 at the smallest and largest Bk only')
    args = ap.parse_args()
    ops.init()
    out = open(args.out, 'w') if args.out else None
    head = ('# ActorCriticPopulation.train(), update_every=\'step\', T = %d, %d alternating repetitions per side; ms per episode of '
            'all K learners: median [min .. max]' % (T, args.reps))
    print(head, flush=True)
    if out:
        out.write(head + '\n')
    for d, batches in SHAPES.items():
        for K in ((16, 512) if args.quick else KS):
            for Bk in ((batches[0], batches[-1]) if args.quick else batches):
                probe(K, d, Bk, 'mixed', args.reps, args.target_ms, out)
    # strict precision (its resident kernels keep spilled registers in scratch, docs/KERNELS.md): two shapes for the record
    for K, Bk in ((256, 12), (256, 192)):
        probe(K, 21, Bk, 'f64', args.reps, args.target_ms, out)
    if out:
        out.close()


if __name__ == '__main__':
    main()
