#!/usr/bin/env python3
"""GPU: the backward-equation check of the reference sweep's shape (mfg_synthetic.py:902-925: K = 200 learners, 26 start rows,
d = 21, 16 hours, one rollout per start row, mixed precision).

(a) the full call: one population.consistency call (context, uploads, three launches, one read-back) against 200 sequential
    mfg_synthetic.actor_critic.evaluate_synthetic_JSD(1, 26) calls (generate_trajectory, mfg_backward_value, NumPy mean / std;
    that class is the parent commit's, unchanged).  Host wall clock around calls that end in a read-back; the population side
    is the median of --calls calls, the class side the median over --rounds rounds of the sum of its 200 calls.
(b) the backward kernel alone, over those 5 200 trajectories' actions [200, 26, 15, 21, 21]: mfg_consistency_given without V
    and with V (the new scan AND the per-group reduction: two launches) against mfg_backward_value (one launch, V always).
    Device events around --iters back-to-back calls, --reps alternating repetitions after a warm-up; median (min .. max).
The two sides' per-hour values are compared first (l1 rtol 1e-12, jsd rtol 1e-10).
python tools/consistency_probe.py [--calls 20] [--rounds 5] [--iters 20] [--out profiles/consistency_pop.txt]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from discrete_mean_field_game_amd import _lib as L, ops, population  # noqa: E402
from discrete_mean_field_game_amd.mfg_synthetic import actor_critic as SAC  # noqa: E402

K, N, H, D = 200, 26, 16, 21
ALPHA = 10000.0


def timed(fn, iters):
    """ms per call: device events around `iters` calls."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles',
                                                  'consistency_pop.txt'), help='the file the lines are written to')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('consistency_probe needs a GPU')
    ops.init()
    dev = torch.device('cuda', torch.cuda.current_device())
    rs = np.random.RandomState(0)
    pi0 = np.array([[float('%.3e' % v) for v in row] for row in rs.dirichlet(np.ones(D), size=N)])
    points = [(shift, theta) for shift in np.arange(0, 0.04, 0.02) for theta in np.arange(0, 5.0, 0.05)]
    sh, th = np.array([p[0] for p in points]), np.array([p[1] for p in points])
    cell = lambda v: '%9.4f (%9.4f .. %9.4f)' % (np.median(v), min(v), max(v))
    lines = ['backward-equation check, K = %d, %d start rows, d = %d, %d hours, R = 1, mixed precision; ms' % (K, N, D, H)]

    # ---- (a) the full call
    new_call = lambda: population.consistency(th, sh, ALPHA, pi0, d=D, seed=0, hours=H)
    learners = [SAC(float(th[k]), float(sh[k]), ALPHA, D, pi0=pi0, seed=0, verbose=0) for k in range(K)]

    def old_round():
        out = []
        for ac in learners:
            ac._rng_step = 0
            out.append(ac.evaluate_synthetic_JSD(1, N))
        return np.array(out)

    got, want = new_call(), old_round()
    assert np.allclose(got.jsd_mean, want[:, 0], rtol=1e-9) and np.allclose(got.jsd_std, want[:, 1], rtol=1e-6, atol=1e-12)
    wall(new_call)
    t_new = [wall(new_call) for _ in range(args.calls)]
    t_old = [wall(old_round) for _ in range(args.rounds)]
    line = '(a) full call: population.consistency %s [%d calls]; 200 x actor_critic.evaluate_synthetic_JSD(1, 26) %s [%d rounds]; ' \
           'ratio %.1f' % (cell(t_new), args.calls, cell(t_old), args.rounds, np.median(t_old) / np.median(t_new))
    print(line, flush=True)
    lines.append(line)

    # ---- (b) the backward kernel alone, on the actions of the K policies
    f = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=dev)
    out = ops.consistency_pop(torch.as_tensor(pi0.astype(np.float32), device=dev), f(th), f(sh), f(np.full(K, ALPHA)),
                              torch.zeros(K, dtype=torch.int64, device=dev), H, want_actions=True, want_steps=True)
    P = out['actions']
    B, T = K * N, H - 1
    V = torch.empty(B, T + 1, D, dtype=torch.float64, device=dev)
    l1 = torch.empty(B, T, dtype=torch.float64, device=dev)
    js = torch.empty(B, T, dtype=torch.float64, device=dev)
    metrics = torch.empty(K, 4, dtype=torch.float64, device=dev)
    steps = torch.empty(K, N, T, 2, dtype=torch.float64, device=dev)
    h = L.lib()
    st = lambda: torch.cuda.current_stream().cuda_stream

    def old():
        L.check(h.mfg_backward_value(P.data_ptr(), B, T, D, V.data_ptr(), l1.data_ptr(), js.data_ptr(), st()), 'mfg_backward_value')

    def new(with_V=False):
        L.check(h.mfg_consistency_given(P.data_ptr(), K, N, T, D, metrics.data_ptr(), steps.data_ptr(),
                                        V.data_ptr() if with_V else None, None, 0, st()), 'mfg_consistency_given')

    old(), new()
    torch.cuda.synchronize()
    assert torch.allclose(steps[..., 0].reshape(B, T), l1, rtol=1e-12, atol=0) and torch.allclose(steps[..., 1].reshape(B, T), js,
                                                                                                   rtol=1e-10, atol=0)
    sides = {'new': new, 'new_V': lambda: new(True), 'old': old}
    for fn in sides.values():
        timed(fn, 3)
    t = {k: [] for k in sides}
    for _ in range(args.reps):
        for k, fn in sides.items():
            t[k].append(timed(fn, args.iters))
    line = '(b) backward kernel, %d trajectories: mfg_consistency_given (scan + reduction) without V %s, with V %s; ' \
           'mfg_backward_value %s; ratio %.2f [%d repetitions of %d calls]' % (
               B, cell(t['new']), cell(t['new_V']), cell(t['old']), np.median(t['old']) / np.median(t['new']), args.reps, args.iters)
    print(line, flush=True)
    lines.append(line)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
