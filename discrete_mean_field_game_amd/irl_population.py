"""A population of K independent max-ent IRL forward learners trained in the launches of one (mfg_train_episodes_irl_pop /
mfg_train_rollouts_irl_pop, include/mfg_hip.h).

The forward solve of the reference's IRL loop (AC_IRL.train, ac_irl.py:634-732) is what an outer iteration spends its time
on, and the sweep driver runs one learner after another.  AC_IRLPopulation holds K learners, each with its own theta, critic
weights w, shift, alpha_scale, learning rates, Philox seed, `batch` trajectories and reward network (or one network shared by
all), and trains them in lock-step: after the same train() calls learner k holds exactly (bit for bit) what
`AC_IRL(theta_k, shift_k, alpha_k, d, seed=seed_k, batch=batch, update_every=...)` with the same w and network holds after
`train(E, stop_criteria=-1)`.

Early stop: train(E, stop_criteria=c) (a scalar or [K]) gives learner k, bit for bit, what AC_IRL.train(E, stop_criteria=c_k)
gives -- theta, w, episodes_run[k], the list_policies FIFO, and the episode returns up to episodes_run[k] (0 beyond).  The
learners' activity states live on the device (the population control block, mfg_ctx_set_pop_control): a learner that has
converged leaves every later launch of the call at once and the host reads nothing back inside the call.  The shared Philox
step and the per-learner reward-call counters still advance by the full E for every learner (deterministic, no read-back), so
a LATER call of a learner that stopped early corresponds to an AC_IRL whose _rng_step and _reward_calls were set to these
values, not to one that simply went on.  isolate=True, learner_state, episodes_run, learner_status and clear_status(k) are
those of ActorCriticPopulation (population.py): a diverged learner is frozen and skipped -- by evaluate (NaN rows, no CSV
line), update_reward, reward_iteration, test_reward_network, the D_samp generation and outerloop -- instead of stopping the
sweep.

Scope: one GPU, start states drawn on the device (batch >= 2), Philox sampling, the matrix-core reward-network kernel's
geometry (d = 15 / 21, n_fc3 <= 16).

With per-learner networks and `demonstrations`, the population also runs the reward half of the IRL loop: update_reward,
reward_iteration and outerloop give learner k exactly what AC_IRL's methods give with learner k's settings, its lr_reward
and the module `random` stream seeded with host_seeds[k] (each learner draws its batches from its own random.Random; the
module stream is never touched).  Early stopping in reward_iteration is decided per learner, so the reward-call, reward-train,
Adam-step and reward-update counters are per-learner arrays; the Philox step and the D_samp trajectory counter stay shared.
The reward updates of all learners run in the two launches per update of mfg_reward_net_train_steps_pop, each
reward_iteration check is one population forward (mfg_reward_net_forward_pop) over the demonstrations and one over the
learners' D_samp, plus one host read.  D_samp is generated as AC_IRL._generate_device does, one draw + one rollout launch per
learner.  Out of scope: CSV / checkpoint files, a population state_dict, multi-GPU and eval-set overrides.

importance_weights=True: every learner trains on the loss as the reference wrote it (ac_irl.py:404-405, commented out there),
each generated trajectory weighted by z_j = [1/k sum_k q_k(tau_j)]^-1 over the learner's own policy FIFO (calc_z, :292-379).  The
population keeps ln z [K, capacity] in fp64 beside the stacked D_samp, refreshes it with ONE mfg_traj_log_z_pop launch when
D_samp or a FIFO changed (once per outer iteration) and hands it to mfg_reward_net_train_steps_pop_z; learner k still equals
AC_IRL(..., importance_weights=True) with its settings bit for bit.  Off (the default) no `_z` symbol is called.

Mixed populations (mixed_nets=True): the learners' networks may differ in n_fc3, n_fc4 and regulariser -- the three axes of
the reference's sweep gridsearch.py:8-31.  Each learner's parameters are one flat row of a [K, stride] buffer in its OWN layout
(mfg_reward_net_param_offsets of its geometry; stride = the longest row rounded up to PARAM_ALIGN, tails zero and never
written), the Adam moments likewise, and a geometry table (mfg_rn_geom_t, one 16-byte entry per learner, host and device)
tells the kernels of the population calls which shape a learner's blocks run.  Learner k still gives exactly what AC_IRL
gives with learner k's shape and regulariser.  test_reward_network() is AC_IRL.test_reward_network for every learner, and
gridsearch() below runs the reference's sweep as one such population.

The instance owns one ops.Context; its sticky status word is shared by the K learners (as for ActorCriticPopulation; with
isolate=True a diverged learner is booked to its own word instead).
"""
from __future__ import annotations

import copy
import os
import random

import numpy as np
import torch

from . import _lib as L
from . import ops
from .ac_irl import AC_IRL
from .mfg_ac2 import EPISODE_STEPS
from .networks import RewardNet
from .population import _Population, _with_ctx, broadcast
from .reward_learning import (RN_SEED_OFFSET, RT_SEED_OFFSET, RewardTrainer, StackedTrajectoryStore, TrajectoryStore,
                              batch_fits, draw_batches, philox_call_key)      # (the rules shared with AC_IRL)

# the tensors of mfg_reward_net_t, in the order of the struct, and the module parameter each one comes from
NET_TENSORS = (('conv1_w', 'conv1.weight'), ('conv1_b', 'conv1.bias'), ('conv2_w', 'conv2.weight'), ('conv2_b', 'conv2.bias'),
               ('fc3_w', 'fc3.weight'), ('fc3_b', 'fc3.bias'), ('fc4_w', 'fc4.weight'), ('fc4_b', 'fc4.bias'),
               ('out_w', 'out.weight'), ('out_b', 'out.bias'))
NUM_DEMO_SAMPLES = NUM_GEN_SAMPLES = 5     # AC_IRL.num_demo_samples / num_gen_samples
PARAM_ALIGN = 64             # floats: one learner's flat parameter row is padded to this (keeps every fc3_w 8-byte aligned)


def check_demonstrations(demonstrations, d):
    """The demonstrations as float32 arrays (states [n, 15, d], actions [n, 15, d, d]); ValueError when missing or ragged."""
    if demonstrations is None or len(demonstrations) == 0:
        raise ValueError('the reward half of the IRL loop needs demonstrations (a list of trajectories of %d (state, action) '
                         'pairs)' % EPISODE_STEPS)
    for tr in demonstrations:
        if len(tr) != EPISODE_STEPS:
            raise ValueError('ragged demonstrations: every trajectory needs %d (state, action) pairs, got %d'
                             % (EPISODE_STEPS, len(tr)))
    s = np.array([[np.asarray(p[0], dtype=np.float32)[:d] for p in tr] for tr in demonstrations], dtype=np.float32)
    a = np.array([[np.asarray(p[1], dtype=np.float32)[:d, :d] for p in tr] for tr in demonstrations], dtype=np.float32)
    if s.shape[2] != d or a.shape[2:] != (d, d):
        raise ValueError('demonstrations: states of %d entries / actions of %d x %d expected' % (d, d, d))
    return s, a


def _check_common(K, d, batch, update_every, precision):
    """The checks check_args and check_args_mixed share, ahead of those on the networks."""
    if K < 1 or K > L.POP_MAX_K:
        raise ValueError('population size %d outside [1, %d]' % (K, L.POP_MAX_K))
    if d not in ops.IRL_POP_D:
        raise ValueError('d=%d: IRL populations cover d = 15 / 21 (the matrix-core reward-network kernel)' % d)
    if batch < 2:
        raise ValueError('batch=%d: a population draws its start states on the device, which AC_IRL does from batch 2 on'
                         % batch)
    if update_every not in ('step', 'rollout'):
        raise ValueError("update_every must be 'step' or 'rollout'")
    if precision not in ('mixed', 'f64'):
        raise ValueError("precision must be 'mixed' or 'f64'")


def _check_nets(nets, d, geometry):
    """... and behind them: RewardNet modules of the population's d; returns what `geometry` (ops.irl_pop_net_geometry /
    ops.irl_pop_net_geometries) gives behind d."""
    if not all(isinstance(n, RewardNet) for n in nets):
        raise ValueError('reward_nets: expected networks.RewardNet modules')
    nd, *rest = geometry(nets)
    if nd != d:
        raise ValueError('reward network d=%d, population d=%d' % (nd, d))
    return rest


def check_args(K, d, batch, update_every, precision, reward_nets):
    """Validation of the constructor's arguments (no GPU needed); returns the networks as a list (1 = shared)."""
    _check_common(K, d, batch, update_every, precision)
    nets = [reward_nets] if isinstance(reward_nets, torch.nn.Module) else list(reward_nets)
    if len(nets) not in (1, K):
        raise ValueError('reward_nets: one network (shared) or %d (one per learner), got %d' % (K, len(nets)))
    _check_nets(nets, d, ops.irl_pop_net_geometry)
    return nets


def check_args_mixed(K, d, batch, update_every, precision, reward_nets):
    """check_args for a population with per-learner network shapes (mixed_nets=True): one network per learner, each inside the
    matrix-core kernel's limits, d / k1 / f2 / k2 shared.  Returns (networks, [(n3, n4, keep_prob, l1l2), ...])."""
    _check_common(K, d, batch, update_every, precision)
    if isinstance(reward_nets, torch.nn.Module):
        raise ValueError('mixed_nets: one network per learner is needed, got one shared network')
    nets = list(reward_nets)
    if len(nets) != K:
        raise ValueError('mixed_nets: one network per learner is needed (%d), got %d' % (K, len(nets)))
    geoms, = _check_nets(nets, d, ops.irl_pop_net_geometries)
    return nets, geoms


def net_row_offsets(d, n3, n4):
    """The 11 offsets (ten tensors of NET_TENSORS and the parameter count) of one learner's flat row."""
    import ctypes as C
    offs = (C.c_int64 * 11)()
    L.check(L.lib().mfg_reward_net_param_offsets(int(d), 5, 2, 3, int(n3), int(n4), offs), 'mfg_reward_net_param_offsets')
    return [int(o) for o in offs]


class AC_IRLPopulation(_Population):
    _WITH_P = True

    def __init__(self, thetas, shifts=0.0, alpha_scales=1e4, d=15, *, batch, reward_nets, seeds=None, w0=None, pi0=None,
                 path_to_dir=None, update_every='step', precision='mixed', device=None, verbose=0, demonstrations=None,
                 lr_reward=1e-4, num_policies=10, host_seeds=None, mixed_nets=False, demonstrations_test=None,
                 importance_weights=False):
        th = np.asarray(thetas, dtype=np.float64).reshape(-1)
        K = th.shape[0]
        geoms = None
        if mixed_nets:
            nets, geoms = check_args_mixed(K, int(d), int(batch), update_every, precision, reward_nets)
        else:
            nets = check_args(K, int(d), int(batch), update_every, precision, reward_nets)
        self.mixed_nets = bool(mixed_nets)
        self._geom = None                      # (host table, device copy) of a mixed population (None: no table)
        test_np = check_demonstrations(demonstrations_test, int(d)) if demonstrations_test else None
        lr_reward = broadcast('lr_reward', lr_reward, K)
        if int(num_policies) < 1:
            raise ValueError('num_policies < 1')
        demo_np = check_demonstrations(demonstrations, int(d)) if demonstrations is not None else None
        super().__init__(th, d, batch, EPISODE_STEPS, shifts, alpha_scales, seeds, w0, pi0, path_to_dir, update_every, precision,
                         device, verbose)
        dev = self.device
        self._rn_seeds_dev = torch.as_tensor((self.seeds + np.uint64(RN_SEED_OFFSET)).view(np.int64), device=dev)
        # the networks: owned copies, one stacked fp32 tensor per parameter ([1, ...] when shared); per-learner networks live
        # in one flat buffer [K, ld] (the reward trainer's parameter layout, rows padded to PARAM_ALIGN floats) and the
        # stacked tensors are views into it
        self._templates = [copy.deepcopy(n).to('cpu') for n in nets]
        self.per_learner_net = len(nets) > 1 or bool(mixed_nets)      # (a mixed population of one learner owns its network)
        self._net_params = {}
        self._flat = None
        self._net_stride = 0
        n0 = nets[0]
        self._rn_dims = (n0.d, n0.conv1.kernel_size[0], n0.conv2.out_channels, n0.conv2.kernel_size[0], n0.fc3.out_features,
                         n0.fc4.out_features)
        if mixed_nets:
            self._rn_dims = self._rn_dims[:4] + (max(g[0] for g in geoms), max(g[1] for g in geoms))    # the largest learner
        with torch.no_grad():
            if mixed_nets:
                # learner k's row in ITS layout; the tail of a row beyond its own parameter count stays zero
                rows = [net_row_offsets(d, g[0], g[1]) for g in geoms]
                self._row_offsets = rows
                self._net_stride = (max(r[10] for r in rows) + PARAM_ALIGN - 1) // PARAM_ALIGN * PARAM_ALIGN
                self._flat = torch.zeros(K, self._net_stride, dtype=torch.float32, device=dev)
                self._net_views = []
                for k, n in enumerate(nets):
                    views = {}
                    for i, (field, pname) in enumerate(NET_TENSORS):
                        par = n.get_parameter(pname).detach()
                        view = self._flat[k, rows[k][i]:rows[k][i + 1]].view(*par.shape)
                        view.copy_(par.to(device=dev, dtype=torch.float32))
                        views[field] = view
                    self._net_views.append(views)
                self._geom = ops.rn_geom_table(geoms, dev)
            elif self.per_learner_net:
                import ctypes as C
                offs = (C.c_int64 * 11)()
                L.check(L.lib().mfg_reward_net_param_offsets(*self._rn_dims, offs), 'mfg_reward_net_param_offsets')
                npar = int(offs[10])
                self._net_stride = (npar + PARAM_ALIGN - 1) // PARAM_ALIGN * PARAM_ALIGN
                self._flat = torch.zeros(K, self._net_stride, dtype=torch.float32, device=dev)
                for i, (field, pname) in enumerate(NET_TENSORS):
                    shape = tuple(n0.get_parameter(pname).shape)
                    view = self._flat[:, int(offs[i]):int(offs[i + 1])].view(K, *shape)
                    view.copy_(torch.stack([n.get_parameter(pname).detach().to(device=dev, dtype=torch.float32) for n in nets]))
                    self._net_params[field] = view
            else:
                for field, pname in NET_TENSORS:
                    ts = [n.get_parameter(pname).detach().to(device=dev, dtype=torch.float32) for n in nets]
                    self._net_params[field] = torch.stack(ts).contiguous()
        st = L.RewardNetStruct()
        st.k1, st.f2, st.k2 = nets[0].conv1.kernel_size[0], nets[0].conv2.out_channels, nets[0].conv2.kernel_size[0]
        if mixed_nets:      # conv1_w = the base of row 0 is what the calls read with a table; n3 / n4: the largest
            st.n3, st.n4 = self._rn_dims[4], self._rn_dims[5]
            for field, _ in NET_TENSORS:
                setattr(st, field, self._flat.data_ptr())
            st.keep_prob = 1.0
        else:
            _, _, _, keep = ops.irl_pop_net_geometry(nets)
            st.n3, st.n4 = nets[0].fc3.out_features, nets[0].fc4.out_features
            for field, _ in NET_TENSORS:
                setattr(st, field, self._net_params[field].data_ptr())
            st.keep_prob = keep
        self._net_struct = st
        # AC_IRL's reward-call counters (dropout keys), one per learner: reward_iteration's checks stop per learner
        self._calls_k = np.zeros(K, dtype=np.int64)
        # the reward half of the IRL loop (AC_IRL.update_reward / reward_iteration / outerloop)
        self.lr_reward = lr_reward
        self.num_policies = int(num_policies)
        self.host_seeds = broadcast('host_seeds', self.seeds.astype(np.int64) if host_seeds is None else host_seeds, K, np.int64)
        self._random = [random.Random(int(h)) for h in self.host_seeds]
        self.theta_initial = th.copy()
        self.list_policies = [[float(t)] * self.num_policies for t in th]
        self.reward_update_count = np.zeros(K, dtype=np.int64)
        self._reward_train_calls = np.zeros(K, dtype=np.int64)
        self._adam_step = np.zeros(K, dtype=np.int64)
        self._gen_traj_counter = 1 << 40                   # AC_IRL._gen_offset's first id, shared
        self._demo_store = TrajectoryStore(self.d, EPISODE_STEPS, dev)
        self._demo_np = demo_np
        if demo_np is not None:
            self._demo_store.push(torch.from_numpy(demo_np[0]), torch.from_numpy(demo_np[1]))
        self._test_np = test_np                # the test demonstrations of test_reward_network (None: no test set)
        self._test_dev = None
        self._gen_store = StackedTrajectoryStore(K, self.d, EPISODE_STEPS, dev)
        self._adam_m = self._adam_v = None
        if self.per_learner_net:
            self._adam_m = torch.zeros_like(self._flat)
            self._adam_v = torch.zeros_like(self._flat)
        self._rt_stats = torch.zeros(K, 4, dtype=torch.float32, device=dev)
        self._rt_ws = self._rt_plan_dev = self._fw_scratch = None
        # AC_IRL(importance_weights=True) for every learner: ln z [K, capacity] of the learners' D_samp (see _gen_log_z)
        self.importance_weights = bool(importance_weights)
        self._lz = self._lz_key = None

    # ------------------------------------------------------------------ state
    @property
    def _reward_calls(self):
        """The learners' reward-call count: an int while they agree (train() alone), else the per-learner array [K]."""
        c = self._calls_k
        return int(c[0]) if np.all(c == c[0]) else c.copy()

    def reward_net(self, k):
        """Learner k's reward network as a networks.RewardNet (a copy, on the population's device)."""
        if not 0 <= k < self.K:
            raise IndexError('learner %d of %d' % (k, self.K))
        j = k if self.per_learner_net else 0
        net = copy.deepcopy(self._templates[j])
        with torch.no_grad():
            for field, pname in NET_TENSORS:
                src = self._net_views[j][field] if self.mixed_nets else self._net_params[field][j]
                net.get_parameter(pname).copy_(src.cpu())
        return net.to(self.device)

    # ------------------------------------------------------------------ training
    @_with_ctx
    def train(self, num_episodes, gamma=1, constant=False, lr_critic=0.1, lr_actor=0.001, *, first_episode=0, stop_criteria=-1,
              isolate=False, validate=None):
        """`num_episodes` episodes of every learner: AC_IRL.train(num_episodes, stop_criteria[k], ...) under each learner's
        reward network (episodes numbered first_episode + 1 ... in the learning-rate schedule, as there).  lr_critic /
        lr_actor: scalars or [K].  Returns a NumPy array [K, num_episodes] of the per-episode returns as AC_IRL.train books
        them: step mode the sum of the T updates' mean rewards, rollout mode T x the update's mean reward per transition.
        stop_criteria (a scalar or [K]; the default -1: none, unlike AC_IRL.train's 0.01): learner k leaves the call after the
        first episode with |theta - prev_theta| < stop_criteria[k] (ac_irl.py:726) and holds what AC_IRL.train holds then;
        episodes_run[k] says when, its returns are 0 beyond.  The Philox step and the reward-call counters advance by the full
        num_episodes all the same: a later call of learner k corresponds to an AC_IRL whose _rng_step and _reward_calls were
        set to the population's values.  isolate=True: a learner that diverges is frozen instead of raising for everybody
        (ActorCriticPopulation.train).  isolate=False with a criterion (or after an uncleared failure): the diverged learner is
        frozen all the same, the context's status word stays 0, the others finish the call, and train() raises afterwards.
        validate (a population.Validation; None: nothing changes): held-out checks on the device every validate.period
        episodes, as ActorCriticPopulation.train; the results land on self.validation."""
        T = self.episode_steps

        def run(b, lrc, lra, acc):
            common = dict(first_step=self._rng_step, reward_acc=acc, precision=self.precision, net_stride=self._net_stride,
                          geom=self._geom)
            calls = torch.as_tensor(self._calls_k, device=self.device)      # per-learner reward-call counters
            if self.update_every == 'step':
                ops.train_episodes_irl_pop(self._mat_pi0_dev, b['pi'], T, int(num_episodes), first_episode + 1, constant,
                                           self._theta, self._shifts_dev, self._alphas_dev, self._w, gamma, lrc, lra,
                                           self._seeds_dev, self._net_struct, self.per_learner_net, self._rn_seeds_dev, calls,
                                           b['G'], b['ws'], b['run'], **common)
                self._calls_k += int(num_episodes) * T
            else:
                ops.train_rollouts_irl_pop(self._mat_pi0_dev, T, int(num_episodes), first_episode + 1, constant, self._theta,
                                           self._shifts_dev, self._alphas_dev, self._w, gamma, lrc, lra, self._seeds_dev,
                                           self._net_struct, self.per_learner_net, self._rn_seeds_dev, calls, b['G'],
                                           b['ws'], b['run'], **common)
                self._calls_k += int(num_episodes)
        out = self._train(num_episodes, lr_critic, lr_actor, run, stop_criteria, isolate, validate)
        if out.shape[1]:
            for k, t in enumerate(self.thetas):         # AC_IRL.train records the policy (list_policies FIFO)
                if self._act.state[k] != 2:            # (a failed learner has no policy to record)
                    self.list_policies[k] = (self.list_policies[k] + [float(t)])[1:]
        return out * T if self.update_every == 'rollout' else out

    @_with_ctx
    def evaluate(self, episode_length=16, indir='test_normalized_round2', outfile='eval_mfg_round2/validation.csv', write_header=0,
                 *, repeats=1):
        """ActorCriticPopulation.evaluate with the defaults of AC_IRL.evaluate (ac_irl.py:1495-1571: the population's d,
        validation.csv): learner k gets what learner(k).evaluate(thetas[k], shifts[k], alpha_scales[k], d, ...) gives."""
        return self._evaluate(episode_length, indir, outfile, write_header, repeats)

    def learner(self, k):
        """An AC_IRL holding learner k's theta, w, reward network, Philox position and reward-call counter and, for the reward
        half of the loop, the demonstrations, D_samp, the reward trainer's Adam state, lr_reward, the policy FIFO and the
        reward-update counters.  Its construction leaves the global np.random stream (and torch's CPU generator) as they were;
        the module `random` stream is set to learner k's (AC_IRL.update_reward draws its batches from it)."""
        ac = super().learner(k)
        ac._reward_calls = int(self._calls_k[k])
        ac.lr_reward = float(self.lr_reward[k])
        ac.num_policies = self.num_policies
        ac.theta_initial = float(self.theta_initial[k])
        ac.list_policies = list(self.list_policies[k])
        ac.reward_update_count = int(self.reward_update_count[k])
        ac._reward_train_calls = int(self._reward_train_calls[k])
        ac._gen_traj_counter = self._gen_traj_counter
        if self._demo_np is not None:
            ac.list_demonstrations = [[(s_.astype(np.float64), a_.astype(np.float64)) for s_, a_ in zip(st, at)]
                                      for st, at in zip(*self._demo_np)]
        if self._test_np is not None:
            ac.list_demonstrations_test = [[(s_.astype(np.float64), a_.astype(np.float64)) for s_, a_ in zip(st, at)]
                                           for st, at in zip(*self._test_np)]
        if len(self._gen_store):
            ac._gen_store.push(*self._gen_store.gather(k=k))
        if self.per_learner_net and ac._trainer is not None:
            ac.lr_reward = float(self.lr_reward[k])
            ac._trainer.lr = float(self.lr_reward[k])
            npar = ac._trainer.flat.numel()
            ac._trainer.load_state_dict({'m': self._adam_m[k, :npar], 'v': self._adam_v[k, :npar],
                                         'step': int(self._adam_step[k]), 'stats': self._rt_stats[k]})
        ac._stats_host = None
        # the module `random` stream now continues learner k's (AC_IRL.update_reward draws from it)
        random.setstate(self._random[k].getstate())
        return ac

    def _new_learner(self, k):
        net = self.reward_net(k)
        with torch.random.fork_rng(devices=[]):
            ac = AC_IRL(float(self.thetas[k]), float(self.shifts[k]), float(self.alpha_scales[k]), self.d,
                        lr_reward=float(self.lr_reward[k]), num_policies=self.num_policies, reg=net.reg, n_fc3=net.fc3.out_features, n_fc4=net.fc4.out_features, pi0=self.mat_pi0,
                        demonstrations=[], batch=self.batch, seed=int(self.seeds[k]), update_every=self.update_every,
                        precision=self.precision, device=self.device, verbose=self.verbose,
                        importance_weights=self.importance_weights)
        ac.reward_net = net
        ac.create_training_method()
        return ac

    def host_random_state(self, k):
        """Learner k's random.Random state (the stream its update_reward batches are drawn from)."""
        return self._random[k].getstate()

    # ------------------------------------------------------------------ reward learning (AC_IRL.update_reward ...)
    def _check_reward_learning(self):
        if not self.per_learner_net:
            raise ValueError('reward learning needs one reward network per learner (a shared network cannot take K updates)')
        if self._demo_np is None:
            raise ValueError('reward learning needs demonstrations (constructor argument demonstrations=...)')
        nd = min(len(self._demo_store), NUM_DEMO_SAMPLES)
        ng = min(len(self._gen_store), NUM_GEN_SAMPLES)
        if not batch_fits(nd, ng, self._rn_dims[4]):
            raise ValueError('update_reward batch of %d + %d trajectories is outside the HIP training step\'s limits' % (nd, ng))
        return nd, ng

    def _gen_log_z(self):
        """AC_IRL._gen_log_z for the population: ln z [K, capacity] (fp64, device) of every learner's D_samp rows under its own
        policy FIFO (list_policies[k], uploaded as [K, num_policies]) and shift, ONE mfg_traj_log_z_pop launch per refresh;
        recomputed only when D_samp, a FIFO, the shifts or the start table changed.  The launch covers all K learners: a failed
        learner's row is computed from its unused store rows and never read (its updates are skipped)."""
        st = self._gen_store
        pol = np.ascontiguousarray(self.list_policies, dtype=np.float64).reshape(self.K, self.num_policies)
        nss = int(self.mat_pi0.shape[0])
        key = (st.version, st.capacity, pol.tobytes(), np.asarray(self.shifts, dtype=np.float64).tobytes(), nss)
        if self._lz is None or key != self._lz_key:
            lz = torch.full((self.K, st.capacity), float('nan'), dtype=torch.float64, device=self.device)
            if st.rows:
                ops.traj_log_z_pop(st.state, st.action, st.rows, torch.as_tensor(pol, device=self.device),
                                   torch.as_tensor(np.asarray(self.shifts, dtype=np.float64), device=self.device),
                                   float(np.log(nss)), out=lz)
            self._lz, self._lz_key = lz, key
        return self._lz

    @_with_ctx
    def importance_log_weights(self):
        """ln z [K, len(D_samp)] of the learners' D_samp in logical order (AC_IRL.importance_log_weights per learner)."""
        lz = self._gen_log_z()
        idx = torch.as_tensor(self._gen_store.rows, dtype=torch.int64, device=self.device)
        return lz.index_select(1, idx).cpu().numpy()

    def _train_rewards(self, active, n_updates):
        """n_updates update_reward calls of the learners `active` (store sizes fixed): the batches drawn from each learner's
        random.Random in AC_IRL.update_reward's order, then ONE mfg_reward_net_train_steps_pop call."""
        nd, ng = self._check_reward_learning()
        n_active = len(active)
        if n_updates < 1 or n_active == 0:
            return
        plan = ops.rn_train_plan(n_updates * n_active).reshape(n_updates, n_active)     # update-major, as the C call reads it
        nd_all, ng_all = len(self._demo_store), len(self._gen_store)
        drow = np.asarray(self._demo_store.rows, dtype=np.int32)
        grow = np.asarray(self._gen_store.rows, dtype=np.int32)
        for s_, k in enumerate(active):           # (column-wise: the host side is one random.sample pair per update)
            batches = draw_batches(self._random[k], nd_all, ng_all, n_updates)
            c0 = int(self._reward_train_calls[k])
            col = plan[:, s_]
            col['learner'] = k
            col['key'] = [philox_call_key(self.seeds[k], RT_SEED_OFFSET, c0 + 1 + u) for u in range(n_updates)]
            col['lr'] = float(self.lr_reward[k])
            col['adam_step'] = int(self._adam_step[k]) + 1 + np.arange(n_updates)
            col['demo_rows'][:, :nd] = drow[np.array([b[0] for b in batches], dtype=np.int64).reshape(n_updates, nd)]
            col['gen_rows'][:, :ng] = grow[np.array([b[1] for b in batches], dtype=np.int64).reshape(n_updates, ng)]
            self._reward_train_calls[k] += n_updates
            self._adam_step[k] += n_updates
        plan = plan.reshape(-1)
        net = self._templates[0]
        need_ws = (int(L.lib().mfg_reward_net_train_workspace_bytes(*self._rn_dims, (nd + ng) * EPISODE_STEPS)) + 255) // 256 * 256
        need_ws *= n_active
        if self._rt_ws is None or self._rt_ws.numel() * 4 < need_ws:
            self._rt_ws = torch.empty((need_ws + 3) // 4, dtype=torch.float32, device=self.device)
        if self._rt_plan_dev is None or self._rt_plan_dev.numel() < plan.nbytes:
            self._rt_plan_dev = torch.empty(plan.nbytes, dtype=torch.uint8, device=self.device)
        ds, da = self._demo_store.state, self._demo_store.action
        gs, ga = self._gen_store.state, self._gen_store.action
        keep = float(net.keep_prob) if net.use_dropout else 1.0
        ops.reward_net_train_steps_pop(self._flat, self._adam_m, self._adam_v, self._net_stride, self.K, self._rn_dims, (ds, da),
                                       (gs, ga), plan, n_updates, n_active, nd, ng, EPISODE_STEPS, NUM_DEMO_SAMPLES, keep,
                                       net.use_l1l2, self._rt_stats, self._rt_ws, self._rt_plan_dev,
                                       RewardTrainer.BETA1, RewardTrainer.BETA2, RewardTrainer.EPS, geom=self._geom,
                                       gen_log_z=self._gen_log_z() if self.importance_weights else None)

    @_with_ctx
    def update_reward(self, learners=None):
        """One AC_IRL.update_reward of every learner (or of the listed ones): two launches for all of them."""
        active = self._healthy() if learners is None else [int(k) for k in learners if self._act.state[int(k)] != 2]
        self._train_rewards(active, 1)

    def _forward(self, st, ac, active, keys, out=None):
        """One population forward of the learners `active` under `keys` (shared [N, ...] or per-learner [K, N, ...] inputs);
        out: an fp32 [K, N] tensor to fill (rows of other learners are left as they are)."""
        if self._fw_scratch is None:
            self._fw_scratch = torch.empty(2 * self.K, dtype=torch.float64, device=self.device)
        return ops.reward_net_forward_pop(self._net_struct, True, self.K, st, ac, active, keys, out=out,
                                          net_stride=self._net_stride, scratch=self._fw_scratch, geom=self._geom)

    def _reward_averages(self, active):
        """AC_IRL._eval_reward_averages of the learners `active`: one population forward over the demonstrations, one over
        the learners' D_samp, ONE host read; sums as there (r.double().sum() on a contiguous row).  [n_active, 2]."""
        K = self.K
        ds, da = self._demo_store.gather_flat()
        gs, ga = self._gen_store.gather_flat()
        nd, ng = ds.shape[0], gs.shape[1]
        sums = []
        outs = []
        for n, (st, ac) in ((nd, (ds, da)), (ng, (gs, ga))):
            if n == 0:
                outs.append(None)
                continue
            self._calls_k[active] += 1
            keys = [philox_call_key(self.seeds[k], RN_SEED_OFFSET, self._calls_k[k]) for k in active]
            outs.append(self._forward(st, ac, active, keys))
        zero = torch.zeros((), dtype=torch.float64, device=self.device)
        for r in outs:
            for k in active:
                sums.append(r[k].double().sum() if r is not None else zero)
        host = torch.stack(sums).cpu().numpy().reshape(2, len(active))
        avg = np.full((len(active), 2), np.nan)
        if nd:
            avg[:, 0] = [float(v) / nd for v in host[0]]
        if ng:
            avg[:, 1] = [float(v) / ng for v in host[1]]
        return avg

    @_with_ctx
    def reward_iteration(self, max_iterations=500, stop_criteria=0.01, iter_check=10):
        """AC_IRL.reward_iteration for every learner, each stopping on its own.  Between two checks every batch is known in
        advance (the stores do not change), so one native call runs up to `iter_check` updates of all running learners.
        Returns (iterations [K] at which each learner left, averages [K, 2] of its last check: demo / generated; NaN where
        there was none)."""
        K = self.K
        self._check_reward_learning()
        max_iterations, iter_check = int(max_iterations), int(iter_check)
        if iter_check < 1:
            raise ValueError('iter_check < 1')
        prev = np.full(K, -100.0)
        its = np.zeros(K, dtype=np.int64)
        last = np.full((K, 2), np.nan)
        active = self._healthy()                  # (failed learners take no part: iterations 0, NaN averages)
        it = 0
        while it < max_iterations and active:
            u = min(iter_check - it % iter_check, max_iterations - it)
            self.reward_update_count[active] += u
            self._train_rewards(active, u)
            it += u
            its[active] = it
            if it % iter_check:
                continue
            avg = self._reward_averages(active)
            still = []
            for i, k in enumerate(active):
                demo_avg, gen_avg = avg[i]
                last[k] = avg[i]
                if np.isnan(demo_avg) or np.isnan(gen_avg):
                    continue
                if stop_criteria != -1 and abs(demo_avg - prev[k]) < stop_criteria:
                    continue
                prev[k] = demo_avg
                still.append(k)
            active = still
        return its, last

    @_with_ctx
    def test_reward_network(self):
        """AC_IRL.test_reward_network (ac_irl.py:1008-1046) for every learner: D_samp is replaced by len(demonstrations) fresh
        trajectories per learner, then one population forward over the training demonstrations, one over D_samp and one over
        the test demonstrations (constructor argument demonstrations_test).  Returns a NumPy array [K, 3]:
        (reward_demo_avg_train, reward_demo_avg_test, reward_gen_avg) per learner, NaN in the second column without a test set.
        The reward-call counters advance as AC_IRL's do (one per forward)."""
        if not self.per_learner_net:
            raise ValueError('test_reward_network needs one reward network per learner')
        K = self.K
        active = self._healthy()                  # (failed learners: NaN rows)
        num_demos = len(self._demo_store)
        self._gen_store.clear()
        if num_demos:
            self._gen_store.push(*self._generate(num_demos))
        out = np.full((K, 3), np.nan)
        if not active:
            return out
        avg = self._reward_averages(active)
        out[active, 0] = avg[:, 0]
        out[active, 2] = avg[:, 1]
        if self._test_np is not None:
            if self._test_dev is None:
                d = self.d
                self._test_dev = (torch.from_numpy(self._test_np[0]).reshape(-1, d).contiguous().to(self.device),
                                  torch.from_numpy(self._test_np[1]).reshape(-1, d, d).contiguous().to(self.device))
            ts, ta = self._test_dev
            self._calls_k[active] += 1
            keys = [philox_call_key(self.seeds[k], RN_SEED_OFFSET, self._calls_k[k]) for k in active]
            r = self._forward(ts, ta, active, keys)
            host = torch.stack([r[k].double().sum() for k in active]).cpu().numpy()
            out[active, 1] = [float(v) / ts.shape[0] for v in host]
        if self.verbose:
            for k in active:
                print('learner %d: Avg reward demo train %f | Avg reward demo test %f | Avg reward gen %f' % ((k,) + tuple(out[k])))
        return out

    def _given_thetas(self, thetas):
        """`thetas` ([K] or a scalar; None: the learners' own) as a [K] fp64 device array, for a generation only."""
        if thetas is None:
            return None
        return torch.as_tensor(broadcast('thetas', thetas, self.K), device=self.device)

    def _nan_rows(self, active, *shape):
        """An fp32 device tensor [K, *shape]: NaN in the rows of the learners outside `active`."""
        t = torch.empty(self.K, *shape, dtype=torch.float32, device=self.device)
        if len(active) < self.K:
            t.fill_(float('nan'))
        return t

    @_with_ctx
    def reward_distribution(self, *, thetas=None, pi0_test=None, num_bins=20, xmin=-0.1, xmax=0.4, num_points=200,
                            hist_range=None, want_rewards=False):
        """The numbers of plot_reward_distribution (ac_irl.py:1046-1123) for every learner, reduced on the device: the reward of
        every transition of the training demonstrations, of the test demonstrations (constructor argument
        demonstrations_test), of len(demonstrations) trajectories generated from the train start table and of as many from the
        start table `pi0_test` [n, d]; per set the histogram (np.histogram with `num_bins` bins), the moments and the Gaussian
        KDE on linspace(xmin, xmax, num_points); and the three JSDs between the histograms.  Returns a
        reward_dist.RewardDistribution (leading K).  Four population forwards (the demonstrations shared by all learners),
        four mfg_row_distribution launches, ONE host read (a second for the rewards with want_rewards).
        hist_range=None gives every set its own min..max as plt.hist does -- the JSDs then compare histograms over different
        supports, as the reference's do; (lo, hi) gives all sets that range, values outside it are dropped.
        thetas=None generates under the learners' current policies; a [K] array (or scalar) is used for the two generations
        only: unlike the reference, which assigns self.theta = theta_good, no learner's theta is changed.  D_samp is not
        touched.  The counters advance as the calls the method stands for: the reward-call counters by one per forward (four,
        three or two: a missing set has none) in the order of `sets`, the Philox step by 15 and the trajectory counter by
        len(demonstrations) per generation.  Without demonstrations_test / pi0_test the set is NaN with status -1, and so are
        its JSDs.  Failed learners generate nothing and give NaN rows (status _lib.DIST_NONFINITE)."""
        from . import reward_dist
        if not self.per_learner_net:
            raise ValueError('reward_distribution needs one reward network per learner')
        if self._demo_np is None:
            raise ValueError('reward_distribution needs demonstrations (constructor argument demonstrations=...)')
        K, T, d = self.K, EPISODE_STEPS, self.d
        num_demos = len(self._demo_store)
        ops.check_row_distribution_args(K, num_demos * T, num_demos * T, num_bins, hist_range, num_points, xmin, xmax)
        th = self._given_thetas(thetas)
        test_table = None
        if pi0_test is not None:
            test_table = torch.as_tensor(np.ascontiguousarray(np.asarray(pi0_test, dtype=np.float64)[:, :d], dtype=np.float32),
                                         device=self.device)
        active = self._healthy()
        inputs = [self._demo_store.gather_flat(), None, None, None]
        if self._test_np is not None:
            if self._test_dev is None:
                self._test_dev = (torch.from_numpy(self._test_np[0]).reshape(-1, d).contiguous().to(self.device),
                                  torch.from_numpy(self._test_np[1]).reshape(-1, d, d).contiguous().to(self.device))
            inputs[1] = self._test_dev
        for s, table in ((2, self._mat_pi0_dev), (3, test_table)):
            if table is None:
                continue
            st, ac = self._generate(num_demos, mat_dev=table, theta=th)
            inputs[s] = (st[:, :, :T].reshape(K, num_demos * T, d).contiguous(), ac.reshape(K, num_demos * T, d, d))
        rewards = [None] * 4
        for s, inp in enumerate(inputs):
            if inp is None:
                continue
            st, ac = inp
            rewards[s] = self._nan_rows(active, st.shape[-2])
            if active:
                self._calls_k[active] += 1
                keys = [philox_call_key(self.seeds[k], RN_SEED_OFFSET, self._calls_k[k]) for k in active]
                self._forward(st, ac, active, keys, out=rewards[s])
        return reward_dist.summarise(rewards, K, self.device, num_bins, xmin, xmax, num_points, hist_range, want_rewards)

    @_with_ctx
    def action_heatmap(self, *, thetas=None):
        """The numbers of plot_action_heatmap (ac_irl.py:1276-1289) for every learner: (demo_avg [d,d], gen_avg [K,d,d], diff
        [K,d,d]) -- the mean demonstrated action matrix, each learner's mean action over len(demonstrations) freshly generated
        trajectories, and |demo_avg - gen_avg|, fp64 means formed on the device (mfg_action_mean_pop, K = 1 for the
        demonstrations), one host read.  thetas: as for reward_distribution (used for the generation only).  The Philox step
        advances by 15 and the trajectory counter by len(demonstrations); D_samp is not touched; failed learners give NaN
        rows."""
        if self._demo_np is None:
            raise ValueError('action_heatmap needs demonstrations (constructor argument demonstrations=...)')
        K, T, d = self.K, EPISODE_STEPS, self.d
        num_demos = len(self._demo_store)
        active = self._healthy()
        _, da = self._demo_store.gather_flat()
        _, ac = self._generate(num_demos, theta=self._given_thetas(thetas))
        both = torch.empty(K + 1, d, d, dtype=torch.float64, device=self.device)
        ops.action_mean_pop(da, out=both[:1])
        ops.action_mean_pop(ac.reshape(K, num_demos * T, d, d), out=both[1:])
        host = both.cpu().numpy()
        demo_avg, gen_avg = host[0], host[1:].copy()
        failed = [k for k in range(K) if k not in active]
        gen_avg[failed] = np.nan
        return demo_avg, gen_avg, np.abs(demo_avg[None] - gen_avg)

    def _sub_population(self, first, count, dropout):
        """(net struct, geometry table) of the learners [first, first + count) as a population of their own: the struct's
        pointers moved to row `first` of the flat buffer, the table's rows sliced.  dropout=False: keep_prob = 1 in a COPY
        of the struct / the table (no learner's network changes)."""
        import ctypes as C
        st = L.RewardNetStruct.from_buffer_copy(self._net_struct)
        shift = 4 * self._net_stride * first
        for field, _ in NET_TENSORS:
            setattr(st, field, getattr(st, field) + shift)
        geom = self._geom
        if geom is not None:
            host, dev = geom
            host = host[first:first + count].copy()
            if not dropout:
                host['keep_prob'] = 1.0
                dev = torch.from_numpy(host.view(np.uint8).copy()).to(self.device)
            else:
                dev = dev[16 * first:16 * (first + count)]
            geom = (host, dev)
        elif not dropout:
            st.keep_prob = 1.0
        return st, geom

    def _forward_input_grad(self, st, ac, active, keys, reward, bufs, dropout, budget, cache):
        """_forward with a reward input-gradient block bound (ops.reward_input_grad_pop), the learners in chunks whose
        workspace stays within `budget` bytes (population.consistency_chunks; None: its default).  cache: a dict that lives
        as long as one reward_sensitivity call -- the chunks' structs / tables and ONE workspace, grown to the largest need."""
        from .population import consistency_chunks
        K, d = self.K, self.d
        N = int(st.shape[-2])
        if self._fw_scratch is None:
            self._fw_scratch = torch.empty(2 * K, dtype=torch.float64, device=self.device)
        key_of = dict(zip(active, keys))
        for first, count in consistency_chunks(K, ops.rn_input_grad_workspace_bytes(1, N, d), budget):
            mine = [k for k in active if first <= k < first + count]
            if not mine:
                continue
            if (first, count) not in cache:
                cache[first, count] = self._sub_population(first, count, dropout)
            struct, geom = cache[first, count]
            need = ops.rn_input_grad_workspace_bytes(count, N, d)
            if cache.get('ws') is None or cache['ws'].numel() * 8 < need:
                cache['ws'] = torch.empty((need + 7) // 8, dtype=torch.float64, device=self.device)
            cut = (lambda t: t) if st.dim() == 2 else (lambda t: t[first:first + count])
            ops.reward_input_grad_pop(struct, True, count, cut(st), cut(ac), [k - first for k in mine], [key_of[k] for k in mine],
                                      out=reward[first:first + count], net_stride=self._net_stride, scratch=self._fw_scratch,
                                      geom=geom, want=tuple(bufs), bufs={n: t[first:first + count] for n, t in bufs.items()},
                                      workspace=cache['ws'])

    @_with_ctx
    def reward_sensitivity(self, *, thetas=None, pi0_test=None, dropout=False, want_samples=False, budget=None):
        """What the learned rewards reward, locally: the derivative of every learner's reward with respect to its inputs, d r /
        d pi [d] and d r / d P [d,d], on every transition of the four sets of reward_distribution (training demonstrations,
        test demonstrations, len(demonstrations) trajectories generated from the train start table and as many from
        `pi0_test`), averaged per set on the device, next to the mean of gradient x input.  Returns a
        reward_dist.RewardSensitivity (leading K).  The same two generations and one population forward per set as
        reward_distribution, each forward with a reward input-gradient block bound (include/mfg_hip.h,
        mfg_ctx_set_rn_input_grad); ONE host read for the means.
        dropout=False evaluates every network with keep_prob = 1 (through a copy of the geometry table / the struct: no
        learner's network changes); dropout=True with the learners' own keep_prob under the calls' keys.  Either way the
        Philox step, the trajectory counter and the reward-call counters advance exactly as reward_distribution advances them
        for the same sets.  thetas: for the two generations only, no theta changes; D_samp is not touched.  want_samples: the
        per-sample gradients too.  budget: bytes of workspace of one call; more learners go in chunks (None:
        population.CONSISTENCY_BUDGET).  A missing set is NaN with status -1; failed learners give NaN rows."""
        from . import reward_dist
        if not self.per_learner_net:
            raise ValueError('reward_sensitivity needs one reward network per learner')
        if self._demo_np is None:
            raise ValueError('reward_sensitivity needs demonstrations (constructor argument demonstrations=...)')
        from .population import consistency_chunks
        K, T, d = self.K, EPISODE_STEPS, self.d
        num_demos = len(self._demo_store)
        th = self._given_thetas(thetas)
        test_table = None
        if pi0_test is not None:
            test_table = torch.as_tensor(np.ascontiguousarray(np.asarray(pi0_test, dtype=np.float64)[:, :d], dtype=np.float32),
                                         device=self.device)
        active = self._healthy()
        inputs = [self._demo_store.gather_flat(), None, None, None]
        if self._test_np is not None:
            if self._test_dev is None:
                self._test_dev = (torch.from_numpy(self._test_np[0]).reshape(-1, d).contiguous().to(self.device),
                                  torch.from_numpy(self._test_np[1]).reshape(-1, d, d).contiguous().to(self.device))
            inputs[1] = self._test_dev
        for n in {num_demos * T} | ({int(inputs[1][0].shape[0])} if inputs[1] is not None else set()):
            consistency_chunks(K, ops.rn_input_grad_workspace_bytes(1, n, d), budget)     # (refused before anything runs)
        for s, table in ((2, self._mat_pi0_dev), (3, test_table)):
            if table is None:
                continue
            st, ac = self._generate(num_demos, mat_dev=table, theta=th)
            inputs[s] = (st[:, :, :T].reshape(K, num_demos * T, d).contiguous(), ac.reshape(K, num_demos * T, d, d))

        cache = {}

        def run(s, st, ac, reward, bufs):
            self._calls_k[active] += 1
            keys = [philox_call_key(self.seeds[k], RN_SEED_OFFSET, self._calls_k[k]) for k in active]
            self._forward_input_grad(st, ac, active, keys, reward, bufs, dropout, budget, cache)
        return reward_dist.sensitivity(inputs, K, d, active, self.device, run, want_samples)

    @_with_ctx
    def reward_heatmap(self, *, theta=8.64, states=None, actions=None):
        """The numbers of plot_reward_heatmap (ac_irl.py:1378-1443) for every learner: the reward of three prototype states x
        three prototype actions.  Returns (rewards [K,3,3] fp32, rewards[k,i,j] = r_k(state i, action j); states [3,d];
        actions [K,3,d,d]).  Default states: the first row of the start table; weight 2^(d-i) on topic i, normalised in fp32;
        uniform.  Default actions: action 1 of learner k is the first action of ONE trajectory generated from the one-row
        start table [state 2] under (theta, shift_k, alpha_scale_k) -- mass moves to more popular topics; the Philox step
        advances by 15 and the trajectory counter by 1 --, action 2 is uniform, action 3 is action 1 with every row reversed.
        The nine pairs of every learner go through ONE population forward, dropout as the learner's network has it (the
        reference's quirk); the reward-call counters advance by one.  Unlike the reference, no learner's theta is assigned.
        states [3,d] / actions [3,d,d] or [K,3,d,d]: given ones; given actions skip the generation.  Failed learners: NaN."""
        from . import reward_dist
        if not self.per_learner_net:
            raise ValueError('reward_heatmap needs one reward network per learner')
        K, d = self.K, self.d
        active = self._healthy()
        protos = reward_dist.heatmap_states(self.mat_pi0, d)
        if states is None:
            states = protos
        if actions is None:
            table = torch.as_tensor(protos[1:2].copy(), device=self.device)
            _, ac = self._generate(1, mat_dev=table, theta=self._given_thetas(theta))
            actions = reward_dist.heatmap_actions(ac[:, 0, 0].cpu().numpy())
        st9, ac9, states, actions = reward_dist.heatmap_pairs(states, actions, K, d)
        out = self._nan_rows(active, 9)
        if active:
            self._calls_k[active] += 1
            keys = [philox_call_key(self.seeds[k], RN_SEED_OFFSET, self._calls_k[k]) for k in active]
            self._forward(torch.as_tensor(st9, device=self.device), torch.as_tensor(ac9, device=self.device), active, keys, out=out)
        failed = [k for k in range(K) if k not in active]
        actions = actions.copy()
        actions[failed] = np.nan
        return out.cpu().numpy().reshape(K, 3, 3), states, actions

    def _generate(self, n, mat_dev=None, theta=None):
        """AC_IRL._generate_device(n) of every learner (its seed, theta, shift, alpha_scale; shared Philox step and
        trajectory ids): K draw + rollout launch pairs.  Returns (pi_traj [K,n,16,d], P [K,n,15,d,d]).  mat_dev: another
        start table [num_start, d] fp32 on the device (default: the train table); theta: another [K] fp64 device array of
        policies to roll (default: the learners' own)."""
        K, T, d = self.K, EPISODE_STEPS, self.d
        mat_dev = self._mat_pi0_dev if mat_dev is None else mat_dev
        theta = self._theta if theta is None else theta
        off = self._gen_traj_counter
        self._gen_traj_counter = off + n
        live = self._healthy()                     # (a failed learner rolls nothing: its rows stay zero and are never read)
        new = torch.empty if len(live) == K else torch.zeros
        states = new(K, n, T + 1, d, dtype=torch.float32, device=self.device)
        actions = new(K, n, T, d, d, dtype=torch.float32, device=self.device)
        for k in live:
            seed = int(self.seeds[k])
            _, pi0 = ops.draw_start(mat_dev, n, seed, self._rng_step, off)
            ops.rollout(pi0, T, theta[k:k + 1], float(self.shifts[k]), float(self.alpha_scales[k]), seed=seed,
                        first_step=self._rng_step, traj_offset=off, td=False, write_P=True, precision=self.precision,
                        out={'pi_traj': states[k], 'P': actions[k]})
        self._rng_step += T
        return states, actions

    @_with_ctx
    def outerloop(self, num_iterations=20, num_gen_from_policy=5, max_reward_iterations=100, max_forward_episodes=200, gamma=1,
                  constant=False, lr_critic=0.1, lr_actor=0.001, *, final_training=True, isolate=False):
        """AC_IRL.outerloop for every learner: alternate reward_iteration (stop criterion 1e-4, a check every 10 updates) and
        forward solves from theta_initial, D_samp refreshed as a FIFO; closes with a 2000-episode forward solve unless
        final_training=False.  lr_critic / lr_actor: scalars or [K].  Returns the thetas [K].
        isolate=True: the learners' range is checked on the device before the first D_samp generation and every forward solve
        runs with train(..., isolate=True), so a learner that is or goes out of range is frozen and skipped while the loop
        completes for the others."""
        nd = min(len(self._demo_store), NUM_DEMO_SAMPLES)
        self._check_reward_learning()
        if not batch_fits(nd, min(int(num_gen_from_policy) * self.num_policies, NUM_GEN_SAMPLES), self._rn_dims[4]):
            raise ValueError('update_reward batch outside the HIP training step\'s limits')
        num_gen_from_policy = int(num_gen_from_policy)
        if isolate:
            self.train(0, isolate=True)            # (no episode: the control block's check alone, before anything samples)
        self._gen_store.clear()
        self._gen_store.push(*self._generate(num_gen_from_policy * self.num_policies))
        self.reward_update_count[:] = 0
        th0 = torch.as_tensor(self.theta_initial, device=self.device)
        for _ in range(int(num_iterations)):
            self._gen_store.push(*self._generate(num_gen_from_policy), drop=num_gen_from_policy)
            self.reward_iteration(max_iterations=max_reward_iterations, stop_criteria=0.0001, iter_check=10)
            self._theta.copy_(th0)
            self.train(max_forward_episodes, gamma, constant, lr_critic, lr_actor, isolate=isolate)
        if final_training:
            self._theta.copy_(th0)
            self.train(2000, gamma, constant, lr_critic, lr_actor, isolate=isolate)
        return self.thetas


# ---------------------------------------------------------------------- the reference's sweep (gridsearch.py:8-31)
GRIDSEARCH_HEADER = 'reg,n_fc3,n_fc4,reward_demo_avg_train,reward_demo_avg_test,reward_gen_avg,theta\n'
GRIDSEARCH_LINE = '%s,%d,%d,%f,%f,%f,%f\n'


def gridsearch_points(list_reg, list_nfc3, list_nfc4):
    """The sweep's points (reg, n_fc3, n_fc4) in the reference's loop order: reg outermost, n_fc4 innermost."""
    return [(str(reg), int(n3), int(n4)) for reg in list_reg for n3 in list_nfc3 for n4 in list_nfc4]


def gridsearch_nets(points, d, net_seed=0):
    """Network p of the sweep: RewardNet(d, reg, n_fc3, n_fc4) initialised under torch.manual_seed(net_seed + p); the caller's
    torch generator is left as it was."""
    nets = []
    with torch.random.fork_rng(devices=[]):
        for p, (reg, n3, n4) in enumerate(points):
            torch.manual_seed(int(net_seed) + p)
            nets.append(RewardNet(d, reg, n_fc3=n3, n_fc4=n4))
    return nets


def gridsearch(list_reg=('dropout', 'l1l2', 'dropout_l1l2'), list_nfc3=range(4, 10, 2), list_nfc4=range(4, 10, 2), *,
               demonstrations, demonstrations_test=None, theta=6.5, shift=0, alpha_scale=1e4, d=15, batch, seed=0,
               net_seed=0, outfile='results/reward_gridsearch.csv', outerloop_kwargs=None, update_every='step',
               precision='mixed', pi0=None, device=None, verbose=0, return_population=False, importance_weights=False):
    """The reference's sweep gridsearch.py:8-31 -- for every (reg, n_fc3, n_fc4): AC_IRL(theta, reg=..., n_fc3=..., n_fc4=...),
    outerloop(), test_reward_network(), one CSV line -- as ONE mixed population: point p is learner p, with the network of
    gridsearch_nets, Philox seed and host seed `seed + p`.  Runs outerloop(**outerloop_kwargs) and test_reward_network() once
    for all points and appends the reference's lines ('%s,%d,%d,%f,%f,%f,%f', theta = the point's final theta) to `outfile`
    (None: no file; its header is written when the file is created).  Returns the rows [(reg, n_fc3, n_fc4, train, test, gen,
    theta), ...] in the reference's order, and the population as well with return_population=True.
    importance_weights: every point trains on the importance-weighted loss (AC_IRL(importance_weights=True))."""
    points = gridsearch_points(list_reg, list_nfc3, list_nfc4)
    if not points:
        raise ValueError('gridsearch: empty grid')
    K = len(points)
    nets = gridsearch_nets(points, int(d), net_seed)
    seeds = [int(seed) + p for p in range(K)]
    pop = AC_IRLPopulation([float(theta)] * K, shift, alpha_scale, d, batch=batch, reward_nets=nets, seeds=seeds, pi0=pi0,
                           update_every=update_every, precision=precision, device=device, verbose=verbose,
                           demonstrations=demonstrations, demonstrations_test=demonstrations_test, host_seeds=seeds,
                           mixed_nets=True, importance_weights=importance_weights)
    thetas = np.asarray(pop.outerloop(**dict(outerloop_kwargs or {})), dtype=np.float64).reshape(-1)
    avgs = np.asarray(pop.test_reward_network(), dtype=np.float64)
    rows = [(reg, n3, n4, float(avgs[p, 0]), float(avgs[p, 1]), float(avgs[p, 2]), float(thetas[p]))
            for p, (reg, n3, n4) in enumerate(points)]
    if outfile is not None:
        folder = os.path.dirname(outfile)
        if folder:
            os.makedirs(folder, exist_ok=True)
        new = not os.path.exists(outfile)
        with open(outfile, 'a') as f:
            if new:
                f.write(GRIDSEARCH_HEADER)
            for row in rows:
                f.write(GRIDSEARCH_LINE % row)
    return (rows, pop) if return_population else rows
