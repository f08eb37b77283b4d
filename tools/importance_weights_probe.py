#!/usr/bin/env python3
"""GPU: what the importance weights of the max-ent IRL loss cost (one process per variant, one JSON line each).
  reward_iteration(100) of AC_IRL and of a K-learner AC_IRLPopulation at d = 15 with `rows` trajectories in D_samp, host clock
  around a device synchronise, `reps` repeats after two warm-up calls; with --variant on also with ln z made stale before
  every call (one refresh per reward_iteration, as outerloop causes); the duration of one mfg_traj_log_z_pop refresh at
  50 rows x 10 policies for K = 1 and K (device events); a hash of the trained parameters (same seeds: equal hashes = equal bits).
--variant parent runs a tree without the keyword (put that tree first on PYTHONPATH); off / on pass importance_weights.
python tools/importance_weights_probe.py --variant off|on|parent [--reps 8] [--rows 4096] [--K 16]"""
import argparse
import hashlib
import json
import os
import random
import sys
import time

import numpy as np
import torch

if not os.environ.get('PYTHONPATH'):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ap = argparse.ArgumentParser()
ap.add_argument('--variant', required=True, choices=['parent', 'off', 'on'])
ap.add_argument('--reps', type=int, default=8)
ap.add_argument('--rows', type=int, default=4096)
ap.add_argument('--K', type=int, default=16)
a = ap.parse_args()

import discrete_mean_field_game_amd as pkg
from discrete_mean_field_game_amd.ac_irl import AC_IRL
from discrete_mean_field_game_amd.irl_population import AC_IRLPopulation
from discrete_mean_field_game_amd.networks import RewardNet
from discrete_mean_field_game_amd import ops

dev = torch.device('cuda:0')
d, T = 15, 15
rs = np.random.RandomState(4)
table = rs.dirichlet(np.ones(d), size=20)
demos = [[(rs.dirichlet(np.ones(d)), rs.dirichlet(np.ones(d), size=d)) for _ in range(T)] for _ in range(20)]
kw = {} if a.variant == 'parent' else {'importance_weights': a.variant == 'on'}
out = {'variant': a.variant, 'package': pkg.__file__, 'rows': a.rows, 'K': a.K}


def timed(fn, reps, before=None):
    ts = []
    for _ in range(reps):
        if before:
            before()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return [round(t, 3) for t in ts]


def sha(t):
    return hashlib.sha1(t.detach().cpu().numpy().tobytes()).hexdigest()[:16]


# ---- single learner
np.random.seed(1); torch.manual_seed(1); random.seed(0)
ac = AC_IRL(d=d, pi0=table, demonstrations=demos, batch=32, seed=5, verbose=0, device=dev, **kw)
ac.list_policies = [float(x) for x in np.linspace(7.9, 9.0, ac.num_policies)]
ac._gen_store.push(*ac._generate_device(a.rows))
run = lambda: ac.reward_iteration(100, -1, 10)
timed(run, 2)                                    # warm-up: code objects, workspaces, the first ln z fill
out['single_ms'] = timed(run, a.reps)
if a.variant == 'on':
    def stale():
        ac._lz_key = None
    out['single_refresh_each_call_ms'] = timed(run, a.reps, before=stale)
out['single_params_sha'] = sha(ac._trainer.flat)
out['single_loss'] = ac.loss_val

# ---- population
torch.manual_seed(2)
nets = [RewardNet(d=d, reg='dropout_l1l2', n_fc3=8, n_fc4=4).to(dev) for _ in range(a.K)]
pop = AC_IRLPopulation(np.linspace(8.0, 9.0, a.K), 0.0, 1e4, d, batch=32, reward_nets=nets, seeds=list(range(11, 11 + a.K)),
                       pi0=table, demonstrations=demos, **kw)
pop.list_policies = [[float(x) for x in np.linspace(7.9, 9.0, pop.num_policies) + 0.01 * k] for k in range(a.K)]
pop._gen_store.push(*pop._generate(a.rows))
runp = lambda: pop.reward_iteration(100, -1, 10)
timed(runp, 2)
out['pop_ms'] = timed(runp, a.reps)
if a.variant == 'on':
    def stalep():
        pop._lz_key = None
    out['pop_refresh_each_call_ms'] = timed(runp, a.reps, before=stalep)
out['pop_params_sha'] = sha(pop._flat)

# ---- one refresh of the log weights at 50 rows x 10 policies (device events)
if a.variant != 'parent':
    for K in (1, a.K):
        st = pop._gen_store
        state, action = st.state[:K].contiguous(), st.action[:K].contiguous()
        th = torch.as_tensor(np.linspace(7.9, 9.0, 10)[None].repeat(K, 0).copy(), device=dev)
        sh = torch.zeros(K, dtype=torch.float64, device=dev)
        rows = list(range(50))
        lz = torch.empty(K, state.shape[1], dtype=torch.float64, device=dev)
        scratch = torch.empty(64, dtype=torch.int32, device=dev)
        call = lambda: ops.traj_log_z_pop(state, action, rows, th, sh, float(np.log(20)), out=lz, scratch=scratch)
        for _ in range(3):
            call()
        ev = []
        for _ in range(20):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); call(); e1.record(); e1.synchronize()
            ev.append(round(e0.elapsed_time(e1) * 1e3, 1))
        out['refresh_50x10_K%d_us' % K] = ev
    lzs = ac.importance_log_weights()
    w = np.exp(lzs[:8] - lzs[:8].max()); w /= w.sum()
    out['single_lz_range'] = [float(lzs.min()), float(lzs.max())]
    out['single_ess_first8'] = float(1 / np.sum(w * w))
print(json.dumps(out))
