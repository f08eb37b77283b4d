#!/usr/bin/env python3
"""GPU: the forecast scores (ops.forecast_score: CRPS, rank counts, energy score, per-hour means) against what the project
offered before them: the members of ops.forecast_pop(want_traj=True) scored by torch on the device -- torch.sort plus a weighted
sum for CRPS, comparisons for the counts, torch.cdist (fp64, its default mode, which goes through a matrix product from 26
members on: ||x||^2 + ||y||^2 - 2 x.y, hence a difference of 1e-8 for near-equal members; the mode that follows the definition,
compute_mode='donot_use_mm_for_euclid_dist', fails to launch from R = 256 on at this shape) for the energy score.  K = 16 policies, N = 6 start states, H = 16 hours, d = 21, mixed precision, R
members per start state: the forecast's own benchmark shape.  Both sides score the SAME members (one forecast_pop call per R,
outside the timing); their outputs are compared first.

Timing: device events around --iters back-to-back calls (no host synchronisation inside), five repetitions per side,
alternating the sides, after a warm-up of both at every shape; the table holds each side's median and spread (min .. max) per
call.  The variants without the energy score are timed too.  A torch side that runs out of memory is recorded as such.
python tools/forecast_score_probe.py [--R 64,256,1024] [--iters 10] [--out profiles/forecast_score_ab.txt]"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from discrete_mean_field_game_amd import ops  # noqa: E402

K, N, H, D = 16, 6, 16, 21


def timed(fn, iters):
    """ms per call: device events around `iters` calls."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--R', default='64,256,1024')
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=None, help='also write the table to this file')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('forecast_score_probe needs a GPU')
    ops.init()
    dev = torch.device('cuda', torch.cuda.current_device())
    rs = np.random.RandomState(0)
    emp = np.array([[[float('%.3e' % v) for v in row] for row in rs.dirichlet(np.ones(D), size=H)] for _ in range(N)])
    e64 = torch.as_tensor(emp, device=dev)
    e32 = torch.as_tensor(emp.astype(np.float32), device=dev)
    start32 = e32[:, 0].contiguous()
    f = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=dev)
    th, sh, al = f(np.linspace(6.0, 10.0, K)), f(np.full(K, 0.3)), f(np.full(K, 1e4))
    sd = torch.arange(K, dtype=torch.int64, device=dev)
    lines = ['forecast scores of given members, K = %d, N = %d, H = %d, d = %d (members: mixed precision); ms per call, median '
             '(min .. max) of %d alternating repetitions of %d calls' % (K, N, H, D, args.reps, args.iters),
             '%6s  %-28s  %-28s  %7s  %-28s  %-28s  %7s' % ('R', 'forecast_score', 'torch (sort, cdist)', 'ratio',
                                                            'forecast_score, no energy', 'torch, no energy', 'ratio')]
    for R in [int(r) for r in args.R.split(',')]:
        traj = ops.forecast_pop(start32, th, sh, al, sd, H, repeats=R, want_traj=True)['traj']
        ws = ops.forecast_score_workspace(N, H, D, K, R, dev)
        wts = (2.0 * torch.arange(R, dtype=torch.float64, device=dev) - R + 1.0).view(1, R, 1, 1, 1)

        def new(want_energy=True):
            return ops.forecast_score(traj, e32, e64, N, R, want_energy=want_energy, ws=ws)

        def old(want_energy=True):
            m32 = traj.view(K, R, N, H, D)
            m = m32.double()
            crps = (m - e64).abs().mean(1) - (wts * torch.sort(m, dim=1).values).sum(1) / float(R * R)
            less = (m32 < e32).sum(1, dtype=torch.int32)
            equal = (m32 == e32).sum(1, dtype=torch.int32)
            energy = None
            if want_energy:
                x = m.permute(0, 2, 3, 1, 4).reshape(K * N * H, R, D)
                first = (x - e64.reshape(1, N * H, 1, D).expand(K, N * H, 1, D).reshape(K * N * H, 1, D)).norm(dim=-1).mean(1)
                pairs = torch.cdist(x, x).sum((1, 2))
                energy = (first - pairs / float(2 * R * R)).view(K, N, H)
            return crps, less, equal, energy

        a = new()
        torch.cuda.synchronize()
        try:
            b = old()
            torch.cuda.synchronize()
            oom = False
        except torch.cuda.OutOfMemoryError:
            b, oom = old(False), True
            torch.cuda.synchronize()
        assert torch.equal(a['less'], b[1]) and torch.equal(a['equal'], b[2])
        assert float((a['crps'] - b[0]).abs().max()) <= 1e-12
        if not oom:
            assert float((a['energy'] - b[3]).abs().max()) <= 1e-6
        sides = {'new': new, 'old': old, 'new_lean': lambda: new(False), 'old_lean': lambda: old(False)}
        if oom:
            del sides['old']
        for fn in sides.values():                    # warm-up at this shape
            timed(fn, 2)
        t = {k: [] for k in sides}
        for _ in range(args.reps):
            for k, fn in sides.items():
                t[k].append(timed(fn, args.iters))
        cell = lambda v: '%8.4f (%8.4f .. %8.4f)' % (np.median(v), min(v), max(v))
        old_cell = 'out of memory' if oom else cell(t['old'])
        ratio = '      -' if oom else '%7.2f' % (np.median(t['old']) / np.median(t['new']))
        line = '%6d  %-28s  %-28s  %s  %-28s  %-28s  %7.2f' % (R, cell(t['new']), old_cell, ratio, cell(t['new_lean']),
                                                               cell(t['old_lean']),
                                                               np.median(t['old_lean']) / np.median(t['new_lean']))
        print(line, flush=True)
        lines.append(line)
        del traj
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
