#!/usr/bin/env python3
"""GPU: the ensemble forecast (ops.forecast_pop, three ranks, held-out rows given) against the composition the project offered
before it: ops.evaluate_pop(want_traj=True) plus torch.sort / mean / std over the member axis on the device.  K = 16 policies,
N = 6 start states, H = 16 hours, d = 21, mixed precision, R members per start state.

Timing: device events around --iters back-to-back calls (no host synchronisation inside), five repetitions per side,
alternating the sides, after a warm-up of both at every shape; the table holds each side's median and spread (min .. max) per
call.  Two more columns time forecast_pop without ranks (no LDS sort) and without held-out rows (no curves launch): the
differences to the full call say what the sort and the curves cost.  The outputs of the two sides are compared first: the order
statistics bit for bit, mean / std within 2 R 2^-53.
python tools/forecast_probe.py [--R 64,256,1024] [--iters 20] [--out profiles/forecast_ab.txt]"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from discrete_mean_field_game_amd import ops, population  # noqa: E402

K, N, H, D = 16, 6, 16, 21
PROBS = (0.05, 0.5, 0.95)


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
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=None, help='also write the table to this file')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('forecast_probe needs a GPU')
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
    lines = ['ensemble forecast, K = %d, N = %d, H = %d, d = %d, mixed precision, three ranks; ms per call, median (min .. max) of '
             '%d alternating repetitions of %d calls' % (K, N, H, D, args.reps, args.iters),
             '%6s  %-28s  %-28s  %7s  %-28s  %-28s' % ('R', 'forecast_pop', 'evaluate_pop + torch', 'ratio', 'forecast_pop, no ranks',
                                                        'forecast_pop, no held-out rows')]
    for R in [int(r) for r in args.R.split(',')]:
        ranks = population.forecast_ranks(PROBS, R)
        ws_f = ops.forecast_pop_workspace(N, H, D, K, R, False, dev)
        ws_e = ops.evaluate_pop_workspace(N, H, D, K, R, True, dev)
        idx = torch.as_tensor(ranks, device=dev)

        def new(ranks=ranks, held_out=True):
            return ops.forecast_pop(start32, th, sh, al, sd, H, repeats=R, ranks=ranks, ws=ws_f,
                                    emp32=e32 if held_out else None, emp64=e64 if held_out else None)

        def old():
            metrics, traj = ops.evaluate_pop(e32, e64, th, sh, al, sd, repeats=R, want_traj=True, ws=ws_e)
            m = traj.view(K, R, N, H, D)
            q = torch.sort(m, dim=1).values.index_select(1, idx)
            m64 = m.double()
            return metrics, m64.mean(1), m64.std(1, unbiased=False), q

        a, b = new(), old()
        torch.cuda.synchronize()
        assert torch.equal(a['quant'].permute(0, 3, 1, 2, 4), b[3])
        tol = 2.0 * R * 2.0 ** -53
        assert float((a['mean'] - b[1]).abs().max()) <= tol
        assert float((a['std'] - b[2]).abs().max()) <= 1e-9          # (torch's std: an order and a formula of its own)
        sides = {'new': new, 'old': old, 'noranks': lambda: new(ranks=()), 'noemp': lambda: new(held_out=False)}
        for fn in sides.values():                    # warm-up at this shape
            timed(fn, 3)
        t = {k: [] for k in sides}
        for _ in range(args.reps):
            for k, fn in sides.items():
                t[k].append(timed(fn, args.iters))
        cell = lambda v: '%8.4f (%8.4f .. %8.4f)' % (np.median(v), min(v), max(v))
        line = '%6d  %-28s  %-28s  %7.2f  %-28s  %-28s' % (R, cell(t['new']), cell(t['old']), np.median(t['old']) / np.median(t['new']),
                                                          cell(t['noranks']), cell(t['noemp']))
        print(line, flush=True)
        lines.append(line)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
