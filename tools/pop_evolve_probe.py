#!/usr/bin/env python3
"""GPU: what population-based training inside a population training call (train(..., validate=V, evolve=Evolution(...))) costs,
and what the host loop it replaces costs.  ActorCriticPopulation, rollout mode, K learners x Bk trajectories at d, T steps, E
episodes per call with a held-out check and an exploit / explore step every `period` episodes; wall clock around the calls (each
call's one synchronisation included), alternating rounds, in one process:
  (a) validate  train(E, validate=V)                     the checks alone
  (b) evolve    train(E, validate=V, evolve=Evolution)   checks and steps enqueued by the call itself
  (c) loop      E / period times [train(period), ops.evaluate_pop, metrics to the host, the NumPy step of
                tests/pop_evolve_ref.py, theta / w / rates back to the device]
(b) and (c) start from the same learners and must end on the same bits: the probe checks it after every round.
python tools/pop_evolve_probe.py [--shapes 16x4096 1024x256] [--d 21] [--T 15] [--episodes 64] [--period 8] [--files 5]
                                 [--rows 16] [--rounds 5] [--out profiles/pop_evolve.txt]

The time of a step itself: --trace N runs nothing but N evolved calls per shape (after one warm-up call), for a kernel trace
from outside -- rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o p -- python tools/pop_evolve_probe.py --trace 3 --
whose per-kernel averages (k_pop_evolve_rank, k_pop_evolve_apply) are recorded below the table in profiles/pop_evolve.txt."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import pop_evolve_ref as R  # noqa: E402
from discrete_mean_field_game_amd import ActorCriticPopulation, ops  # noqa: E402
from discrete_mean_field_game_amd.population import Evolution, Validation  # noqa: E402

SEED, COLUMN = 12345, 6       # JSD_mean


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', nargs='+', default=['16x4096', '1024x256'], help='K x Bk')
    ap.add_argument('--d', type=int, default=21)
    ap.add_argument('--T', type=int, default=15)
    ap.add_argument('--episodes', type=int, default=64)
    ap.add_argument('--period', type=int, default=8)
    ap.add_argument('--files', type=int, default=5)
    ap.add_argument('--rows', type=int, default=16)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--trace', type=int, default=0)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    d, T, E, P = a.d, a.T, a.episodes, a.period
    rs = np.random.RandomState(0)
    table = rs.dirichlet(np.ones(d), size=64)
    emp = rs.dirichlet(np.ones(d), size=(a.files, a.rows))
    dev = torch.device('cuda:0')
    emp64 = torch.as_tensor(emp, dtype=torch.float64, device=dev)
    emp32 = torch.as_tensor(emp.astype(np.float32), device=dev)
    lines = ['pop_evolve_probe: %s, ActorCriticPopulation rollout mode d=%d T=%d E=%d period=%d (%d checks, a step after each, '
             'top = bottom = 25 %%), held-out %d files x %d rows, repeats 1, %d alternating rounds, ms per call (medians; all rounds '
             'in brackets)' % (torch.cuda.get_device_name(0), d, T, E, P, E // P, a.files, a.rows, a.rounds)]
    print(lines[0], flush=True)
    for shape in a.shapes:
        K, B = (int(x) for x in shape.split('x'))
        w0 = np.random.RandomState(1).randn(K, ops.num_features(d)) * 0.1     # (the same start for the three populations)
        make = lambda: ActorCriticPopulation(np.linspace(8.2, 9.0, K), 0.16, 12000.0, d, batch=B, w0=w0, pi0=table,
                                             update_every='rollout', episode_steps=T)
        val = Validation(emp=emp, period=P, repeats=1, metric='JSD_mean')
        evo = Evolution(every=1, top=0.25, bottom=0.25, seed=SEED)
        n_top, n_bottom = evo.counts(K)
        rates = {n: [np.full(K, 0.1), np.full(K, 0.001)] for n in ('evolve', 'loop')}
        pops = {'validate': make(), 'evolve': make(), 'loop': make()}

        def evolve():
            pop = pops['evolve']
            pop.train(E, lr_critic=rates['evolve'][0], lr_actor=rates['evolve'][1], validate=val, evolve=evo)
            rates['evolve'] = [pop.evolution.lr_critic, pop.evolution.lr_actor]

        def loop():
            pop = pops['loop']
            lrc, lra = rates['loop']
            first_step = pop._rng_step
            pop._rng_step += a.rows - 1                  # (the checks' Philox steps, as the validated call reserves them)
            active = np.ones(K, bool)
            for c in range(E // P):
                pop.train(P, lr_critic=lrc, lr_actor=lra, first_episode=c * P)
                m = ops.evaluate_pop(emp32, emp64, pop._theta, pop._shifts_dev, pop._alphas_dev, pop._seeds_dev,
                                     first_step=first_step, repeats=1, precision=pop.precision).cpu().numpy()
                out = R.step(m[:, COLUMN], active, pop.thetas, pop.w, lrc, lra, s=c, seed=SEED, n_top=n_top, n_bottom=n_bottom,
                             factors=evo.factors, lr_critic_bounds=evo.lr_critic_bounds, lr_actor_bounds=evo.lr_actor_bounds)
                lrc, lra = out['lr_critic'], out['lr_actor']
                pop._theta.copy_(torch.as_tensor(out['theta'], device=dev))
                pop._w.copy_(torch.as_tensor(out['w'], device=dev))
            rates['loop'] = [lrc, lra]

        def same():
            return (np.array_equal(pops['evolve'].thetas, pops['loop'].thetas) and np.array_equal(pops['evolve'].w, pops['loop'].w)
                    and np.array_equal(rates['evolve'][0], rates['loop'][0]) and np.array_equal(rates['evolve'][1], rates['loop'][1]))
        if a.trace:
            evolve()
            for _ in range(a.trace):
                evolve()
            torch.cuda.synchronize()
            print('traced %d evolved calls at K=%d Bk=%d: %d steps each' % (a.trace, K, B, E // P), flush=True)
            continue
        runs = {'validate': lambda: pops['validate'].train(E, lr_critic=0.1, lr_actor=0.001, validate=val), 'evolve': evolve,
                'loop': loop}
        for fn in runs.values():
            fn()
        assert same(), 'the evolved call and the host loop differ'
        ms = {n: [] for n in runs}
        for _ in range(a.rounds):
            for n, fn in runs.items():
                ms[n].append(wall_ms(fn))
            assert same(), 'the evolved call and the host loop differ'
        replaced = int((pops['evolve'].evolution.parent != np.arange(K)[:, None]).sum())
        med = {n: float(np.median(v)) for n, v in ms.items()}
        f = lambda v: ' '.join('%.2f' % x for x in v)
        lines.append('K=%-5d Bk=%-5d (a) validate %.2f [%s]  (b) evolve %.2f [%s]  (c) loop %.2f [%s]'
                     % (K, B, med['validate'], f(ms['validate']), med['evolve'], f(ms['evolve']), med['loop'], f(ms['loop'])))
        lines.append('        (b) - (a) = %+.3f ms per step;  (c) - (b) = %+.3f ms per step, (c) / (b) = %.3f;  %d learners replaced '
                     'in the last call; (b) and (c) end on the same bits'
                     % ((med['evolve'] - med['validate']) / (E // P), (med['loop'] - med['evolve']) / (E // P),
                        med['loop'] / med['evolve'], replaced))
        print('\n'.join(lines[-2:]), flush=True)
    if a.out and not a.trace:
        with open(a.out, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
