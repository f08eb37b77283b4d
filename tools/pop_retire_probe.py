#!/usr/bin/env python3
"""GPU: what the population control block (train(..., stop_criteria=, isolate=)) costs and gains.  Per class and update mode,
K learners x Bk trajectories at d, E episodes per call, event-timed around train() (the call's one synchronisation included):
  plain      train(E)                         no control block: the launches of the parent
  control    train(E, isolate=True)           a block, nobody retires: + one k_pop_retire launch per episode (and one per call)
  stop       train(E, stop_criteria=c)        `--stop` of the K learners stop after episode 1 (a criterion above any step)
python tools/pop_retire_probe.py [--K 16] [--batch 4096] [--d 21] [--episodes 20] [--stop 12] [--rounds 5] [--no-irl]"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from discrete_mean_field_game_amd import ActorCriticPopulation  # noqa: E402
from discrete_mean_field_game_amd.irl_population import AC_IRLPopulation  # noqa: E402
from discrete_mean_field_game_amd.networks import RewardNet  # noqa: E402


def timed(fn, rounds):
    fn()
    out = []
    for _ in range(rounds):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        out.append(s.elapsed_time(e))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--K', type=int, default=16)
    ap.add_argument('--batch', type=int, default=4096)
    ap.add_argument('--d', type=int, default=21)
    ap.add_argument('--episodes', type=int, default=20)
    ap.add_argument('--stop', type=int, default=12)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--no-irl', action='store_true')
    a = ap.parse_args()
    K, B, d, E = a.K, a.batch, a.d, a.episodes
    table = np.random.RandomState(0).dirichlet(np.ones(d), size=64)
    crit = np.array([1e9] * a.stop + [-1.0] * (K - a.stop))
    classes = [('ActorCriticPopulation', lambda mode: ActorCriticPopulation([8.86349] * K, 0.16, 12000.0, d, batch=B, pi0=table,
                                                                            update_every=mode))]
    if not a.no_irl:
        torch.manual_seed(0)
        nets = [RewardNet(d=d, n_fc3=8, n_fc4=4) for _ in range(K)]
        classes.append(('AC_IRLPopulation', lambda mode: AC_IRLPopulation([8.86349] * K, 0.16, 1e4, d, batch=B, reward_nets=nets,
                                                                          pi0=table, update_every=mode)))
    for name, make in classes:
        for mode in ('step', 'rollout'):
            pop = make(mode)
            # lr 0: theta stays put, every call does the same work (a learner with a criterion of 1e9 still stops after episode 1)
            lr = dict(lr_critic=0.0, lr_actor=0.0)
            plain = timed(lambda: pop.train(E, **lr), a.rounds)
            ctl = timed(lambda: pop.train(E, isolate=True, **lr), a.rounds)
            stop = timed(lambda: pop.train(E, stop_criteria=crit, **lr), a.rounds)
            assert int((pop.learner_state == 1).sum()) == a.stop and list(pop.episodes_run[:a.stop]) == [1] * a.stop
            f = lambda v: ' '.join('%.3f' % x for x in v)
            m = lambda v: float(np.median(v))
            print('%-22s %-7s d=%d K=%d Bk=%d E=%d  ms per call: plain [%s] control [%s] stop %d/%d [%s]' % (
                name, mode, d, K, B, E, f(plain), f(ctl), a.stop, K, f(stop)), flush=True)
            print('%-22s %-7s   medians: plain %.3f  control %.3f (%+.4f ms per episode)  stop %.3f (%.2fx plain)' % (
                name, mode, m(plain), m(ctl), (m(ctl) - m(plain)) / E, m(stop), m(plain) / m(stop)), flush=True)


if __name__ == '__main__':
    main()
