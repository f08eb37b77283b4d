#!/usr/bin/env python3
"""GPU: what held-out validation inside a population training call (train(..., validate=Validation(...))) costs, and what
the host loop it replaces costs.  ActorCriticPopulation, K learners x Bk trajectories at d, T steps, E episodes per call,
event-timed around the calls (each call's one synchronisation included), alternating rounds:
  (a) plain     train(E)                                   no validation block: the launches of the parent
  (b) validate  train(E, validate=Validation(period=P))    E / P checks enqueued by the call itself
  (c) loop      E / P times [train(P), evaluate (ops.evaluate_pop, with --score + ops.forecast_score), copy to host]
for repeats in --repeats, with and without the proper scores.  lr = 0: theta stays put, every call does the same work.
python tools/pop_validate_probe.py [--K 16] [--batch 4096] [--d 21] [--T 15] [--episodes 64] [--period 8] [--files 5]
                                   [--rows 16] [--repeats 1 16] [--rounds 5] [--out profiles/pop_validate.txt]"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from discrete_mean_field_game_amd import ActorCriticPopulation, ops  # noqa: E402
from discrete_mean_field_game_amd.population import Validation  # noqa: E402


def event_ms(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--K', type=int, default=16)
    ap.add_argument('--batch', type=int, default=4096)
    ap.add_argument('--d', type=int, default=21)
    ap.add_argument('--T', type=int, default=15)
    ap.add_argument('--episodes', type=int, default=64)
    ap.add_argument('--period', type=int, default=8)
    ap.add_argument('--files', type=int, default=5)
    ap.add_argument('--rows', type=int, default=16)
    ap.add_argument('--repeats', type=int, nargs='+', default=[1, 16])
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    K, B, d, T, E, P = a.K, a.batch, a.d, a.T, a.episodes, a.period
    rs = np.random.RandomState(0)
    table = rs.dirichlet(np.ones(d), size=64)
    emp = rs.dirichlet(np.ones(d), size=(a.files, a.rows))
    dev = torch.device('cuda:0')
    emp64 = torch.as_tensor(emp, dtype=torch.float64, device=dev)
    emp32 = torch.as_tensor(emp.astype(np.float32), device=dev)
    lr = dict(lr_critic=0.0, lr_actor=0.0)
    lines = ['pop_validate_probe: %s, ActorCriticPopulation d=%d K=%d Bk=%d T=%d E=%d period=%d (%d checks), held-out %d files x %d '
             'rows, %d alternating rounds, ms per call (medians; all rounds in brackets)'
             % (torch.cuda.get_device_name(0), d, K, B, T, E, P, E // P, a.files, a.rows, a.rounds)]
    print(lines[0], flush=True)
    for mode in ('rollout', 'step'):
        for R in a.repeats:
            for score in (False, True):
                pop = ActorCriticPopulation([8.86349] * K, 0.16, 12000.0, d, batch=B, pi0=table, update_every=mode, episode_steps=T)
                val = Validation(emp=emp, period=P, repeats=R, score=score, metric='crps' if score else 'JSD_mean')

                def loop():
                    for _ in range(E // P):
                        pop.train(P, **lr)
                        m, traj = ops.evaluate_pop(emp32, emp64, pop._theta, pop._shifts_dev, pop._alphas_dev, pop._seeds_dev,
                                                   first_step=0, repeats=R, precision=pop.precision, want_traj=True)
                        if score:
                            s = ops.forecast_score(traj, emp32, emp64, a.files, R)['summary'].cpu()
                        m.cpu()
                runs = {'plain': lambda: pop.train(E, **lr), 'validate': lambda: pop.train(E, validate=val, **lr), 'loop': loop}
                for fn in runs.values():
                    fn()
                ms = {n: [] for n in runs}
                for _ in range(a.rounds):
                    for n, fn in runs.items():
                        ms[n].append(event_ms(fn))
                assert np.array_equal(pop.validation.checks, [E // P] * K)
                med = {n: float(np.median(v)) for n, v in ms.items()}
                f = lambda v: ' '.join('%.2f' % x for x in v)
                lines.append('%-7s repeats=%-3d score=%d  (a) plain %.2f [%s]  (b) validate %.2f [%s]  (c) loop %.2f [%s]'
                             % (mode, R, score, med['plain'], f(ms['plain']), med['validate'], f(ms['validate']), med['loop'],
                                f(ms['loop'])))
                lines.append('        (b) - (a) = %+.3f ms per check (%+.1f %% of the call);  (c) - (b) = %+.3f ms per check, (c) / (b) = %.2f'
                             % ((med['validate'] - med['plain']) / (E // P), 100.0 * (med['validate'] - med['plain']) / med['plain'],
                                (med['loop'] - med['validate']) / (E // P), med['loop'] / med['validate']))
                print('\n'.join(lines[-2:]), flush=True)
    if a.out:
        with open(a.out, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
