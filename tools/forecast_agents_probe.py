#!/usr/bin/env python3
"""GPU: the finite-population forecast (ops.forecast_agents_pop) at the ensemble forecast's benchmark shape -- K = 16 policies,
N = 6 start states, H = 16 hours, d = 21, R = 256 members per start state, mixed precision, three ranks, held-out rows -- for
populations of A agents per member.

Per A: the whole call; its H - 1 launches of the agents kernel alone (ops.agents_step_pop on the call's own counts and actions,
step by step), hence the agent-steps per second of the kernel and the share of everything else in the call (the H - 1 sampling
launches over all K N R members, row 0, the reductions); and a plain-torch formulation of one step on the same device with the
same number of uniform draws: the agents of (member, topic) are a segment of one long vector, torch.rand gives each its
uniform, one torch.searchsorted over the concatenated row cdfs (row r shifted by r, in fp64) places it, scatter_add counts.
torch needs the draws in memory, so it runs on as many members as fit --torch-draws draws and is reported per agent-step.
The mean-field call (ops.forecast_pop) at the same shape is timed for scale.

Timing: device events around --iters back-to-back calls, --reps repetitions, the sides alternating, after a warm-up of each;
median (min .. max).  python tools/forecast_agents_probe.py [--A 1000,10000,100000,1000000] [--out profiles/forecast_agents.txt]

The share of the sampling launches themselves: --trace N runs nothing but N calls per A (after one warm-up call), for a kernel
trace from outside -- rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o p -- python tools/forecast_agents_probe.py
--A 1000 --trace 10 -- whose per-kernel totals (k_eval_rollout_pop, k_agents_step, k_agents_init, k_forecast_reduce,
k_forecast_curves) are recorded below the table in profiles/forecast_agents.txt."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from discrete_mean_field_game_amd import ops, population  # noqa: E402

K, N, H, D, R = 16, 6, 16, 21, 256
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


def torch_step(counts, P):
    """One step of the members counts [M, d] (int64) under the actions P [M, d, d] in plain torch: counts' [M, d]."""
    M, d = counts.shape
    cdf = P.double().cumsum(-1)
    cdf = cdf / cdf[..., -1:]
    rows = torch.arange(M * d, device=counts.device)
    seq = (cdf.view(M * d, d) + rows[:, None].double()).view(-1)     # row r's cdf in (r, r + 1]: one ascending sequence
    row_of = torch.repeat_interleave(rows, counts.view(-1))          # agent -> its (member, topic) row
    u = torch.rand(row_of.shape[0], dtype=torch.float64, device=counts.device)
    col = torch.searchsorted(seq, u + row_of.double(), right=True) - row_of * d
    col.clamp_(max=d - 1)
    out = torch.zeros(M * d, dtype=torch.int64, device=counts.device)
    out.scatter_add_(0, (row_of // d) * d + col, torch.ones_like(col))
    return out.view(M, d)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--A', default='1000,10000,100000,1000000')
    ap.add_argument('--budget-ms', type=float, default=400.0, help='device time one timed repetition may take (sets the iterations)')
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--torch-draws', type=int, default=1 << 25)
    ap.add_argument('--out', default=None, help='also write the table to this file')
    ap.add_argument('--trace', type=int, default=0, help='only this many forecast_agents_pop calls per A (for a kernel trace)')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('forecast_agents_probe needs a GPU')
    ops.init()
    dev = torch.device('cuda', torch.cuda.current_device())
    rs = np.random.RandomState(0)
    emp = np.array([[[float('%.3e' % v) for v in row] for row in rs.dirichlet(np.ones(D), size=H)] for _ in range(N)])
    e64 = torch.as_tensor(emp, device=dev)
    e32 = torch.as_tensor(emp.astype(np.float32), device=dev)
    f = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=dev)
    th, sh, al = f(np.linspace(6.0, 10.0, K)), f(np.full(K, 0.3)), f(np.full(K, 1e4))
    sd = torch.arange(K, dtype=torch.int64, device=dev)
    ranks = population.forecast_ranks(PROBS, R)
    NR, T = N * R, H - 1
    if args.trace:
        for A in [int(a) for a in args.A.split(',')]:
            counts0 = torch.as_tensor(population.apportion(emp[:, 0], A), device=dev)
            ws = ops.forecast_agents_pop_workspace(N, H, D, K, R, False, False, dev)
            for _ in range(args.trace + 1):
                ops.forecast_agents_pop(counts0, A, th, sh, al, sd, H, repeats=R, ranks=ranks, emp32=e32, emp64=e64, ws=ws)
            torch.cuda.synchronize()
        return
    ws_m =ops.forecast_pop_workspace(N, H, D, K, R, False, dev)
    mean_field = lambda: ops.forecast_pop(e32[:, 0].contiguous(), th, sh, al, sd, H, repeats=R, ranks=ranks, ws=ws_m, emp32=e32, emp64=e64)
    timed(mean_field, 3)
    t_mf = [timed(mean_field, 20) for _ in range(args.reps)]
    cell = lambda v: '%9.3f (%9.3f .. %9.3f)' % (np.median(v), min(v), max(v))
    lines = ['finite-population forecast, K = %d, N = %d, H = %d, d = %d, R = %d (%d members, %d steps), mixed precision, three ranks, '
             'held-out rows; ms, median (min .. max) of %d alternating repetitions' % (K, N, H, D, R, K * NR, T, args.reps),
             'mean-field call (ops.forecast_pop) at this shape: %s ms' % cell(t_mf),
             '%8s  %-33s  %-33s  %13s  %10s  %-33s  %13s  %8s' % ('A', 'forecast_agents_pop, ms per call', 'its %d agents launches alone' % T,
                                                                 'agent-steps/s', 'rest share', 'torch, ms per step of its members',
                                                                 'agent-steps/s', 'ratio')]
    for A in [int(a) for a in args.A.split(',')]:
        counts0 = torch.as_tensor(population.apportion(emp[:, 0], A), device=dev)
        ws = ops.forecast_agents_pop_workspace(N, H, D, K, R, False, False, dev)
        call = lambda: ops.forecast_agents_pop(counts0, A, th, sh, al, sd, H, repeats=R, ranks=ranks, emp32=e32, emp64=e64, ws=ws)
        got = ops.forecast_agents_pop(counts0, A, th, sh, al, sd, H, repeats=R, want_counts=True, want_actions=True)
        cs = [got['counts'][:, :, t].contiguous() for t in range(T)]
        Ps = [got['actions'][:, :, t].contiguous() for t in range(T)]
        assert bool((got['counts'].sum(-1) == A).all())
        del got

        def steps():
            for t in range(T):
                ops.agents_step_pop(cs[t], Ps[t], A, sd, step=t, want_pi=False)

        assert torch.equal(ops.agents_step_pop(cs[0], Ps[0], A, sd, step=0, want_pi=False)[0], cs[1])
        Mt = max(1, min(K * NR, args.torch_draws // A))
        tc, tP = cs[0].view(K * NR, D)[:Mt].long().contiguous(), Ps[0].view(K * NR, D, D)[:Mt].contiguous()
        assert bool((torch_step(tc, tP).sum(-1) == A).all())
        tstep = lambda: torch_step(tc, tP)
        sides = {'call': call, 'steps': steps, 'torch': tstep}
        iters = {}
        for k, fn in sides.items():                  # warm-up, and the iterations the budget allows
            timed(fn, 1)
            iters[k] = int(max(1, min(20, args.budget_ms / max(timed(fn, 1), 1e-3))))
        t = {k: [] for k in sides}
        for _ in range(args.reps):
            for k, fn in sides.items():
                t[k].append(timed(fn, iters[k]))
        work = float(K * NR) * A * T
        ours = work / (np.median(t['steps']) * 1e-3)
        theirs = float(Mt) * A / (np.median(t['torch']) * 1e-3)
        line = '%8d  %-33s  %-33s  %13.3e  %9.1f%%  %-33s  %13.3e  %8.1f' % (
            A, cell(t['call']), cell(t['steps']), ours, 100.0 * (1.0 - np.median(t['steps']) / np.median(t['call'])),
            cell(t['torch']) + ' [%d]' % Mt, theirs, ours / theirs)
        print(line, flush=True)
        lines.append(line)
        del cs, Ps
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
