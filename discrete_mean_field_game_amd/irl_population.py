"""A population of K independent max-ent IRL forward learners trained in the launches of one (mfg_train_episodes_irl_pop /
mfg_train_rollouts_irl_pop, include/mfg_hip.h).

The forward solve of the reference's IRL loop (AC_IRL.train, ac_irl.py:634-732) is what an outer iteration spends its time
on, and the sweep driver runs one learner after another.  AC_IRLPopulation holds K learners, each with its own theta, critic
weights w, shift, alpha_scale, learning rates, Philox seed, `batch` trajectories and reward network (or one network shared by
all), and trains them in lock-step: after the same train() calls learner k holds exactly (bit for bit) what
`AC_IRL(theta_k, shift_k, alpha_k, d, seed=seed_k, batch=batch, update_every=...)` with the same w and network holds after
`train(E, stop_criteria=-1)`.

Scope: one GPU, start states drawn on the device (batch >= 2), Philox sampling, the matrix-core reward-network kernel's
geometry (d = 15 / 21, n_fc3 <= 16), no early stop.  Training the reward networks stays with AC_IRL.

The instance owns one ops.Context; its sticky status word is shared by the K learners (as for ActorCriticPopulation).
"""
from __future__ import annotations

import copy

import numpy as np
import torch

from . import _lib as L
from . import ops
from .ac_irl import AC_IRL
from .mfg_ac2 import EPISODE_STEPS, actor_critic
from .networks import RewardNet
from .population import _with_ctx, broadcast, resolve_start_table

# the tensors of mfg_reward_net_t, in the order of the struct, and the module parameter each one comes from
NET_TENSORS = (('conv1_w', 'conv1.weight'), ('conv1_b', 'conv1.bias'), ('conv2_w', 'conv2.weight'), ('conv2_b', 'conv2.bias'),
               ('fc3_w', 'fc3.weight'), ('fc3_b', 'fc3.bias'), ('fc4_w', 'fc4.weight'), ('fc4_b', 'fc4.bias'),
               ('out_w', 'out.weight'), ('out_b', 'out.bias'))
RN_SEED_OFFSET = 0x5EED      # AC_IRL's dropout key: (seed + 0x5EED) ^ (call x 0x9E3779B97F4A7C15), ac_irl.py reward()


def check_args(K, d, batch, update_every, precision, reward_nets):
    """Validation of the constructor's arguments (no GPU needed); returns the networks as a list (1 = shared)."""
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
    nets = [reward_nets] if isinstance(reward_nets, torch.nn.Module) else list(reward_nets)
    if len(nets) not in (1, K):
        raise ValueError('reward_nets: one network (shared) or %d (one per learner), got %d' % (K, len(nets)))
    if not all(isinstance(n, RewardNet) for n in nets):
        raise ValueError('reward_nets: expected networks.RewardNet modules')
    nd, _, _, _ = ops.irl_pop_net_geometry(nets)
    if nd != d:
        raise ValueError('reward network d=%d, population d=%d' % (nd, d))
    return nets


class AC_IRLPopulation:

    def __init__(self, thetas, shifts=0.0, alpha_scales=1e4, d=15, *, batch, reward_nets, seeds=None, w0=None, pi0=None,
                 path_to_dir=None, update_every='step', precision='mixed', device=None, verbose=0):
        th = np.asarray(thetas, dtype=np.float64).reshape(-1)
        K = th.shape[0]
        nets = check_args(K, int(d), int(batch), update_every, precision, reward_nets)
        if not torch.cuda.is_available():
            raise L.MfgError('AC_IRLPopulation needs a ROCm GPU: the HIP hot path has no CPU fallback')
        L.lib()
        ops.init()
        self.device = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
        self._ctx = ops.Context(self.device)
        self.d, self.batch, self.episode_steps = int(d), int(batch), EPISODE_STEPS
        self.update_every, self.precision, self.verbose = update_every, precision, verbose
        F = ops.num_features(self.d)
        self.shifts = broadcast('shifts', shifts, K)
        self.alpha_scales = broadcast('alpha_scales', alpha_scales, K)
        self.seeds = broadcast('seeds', np.arange(K) if seeds is None else seeds, K, np.uint64)
        dev = self.device
        self._theta = torch.as_tensor(th.copy(), device=dev)
        if w0 is None:
            w = np.stack([np.asarray(actor_critic.init_w(None, self.d), dtype=np.float64).reshape(-1) for _ in range(K)])
        else:
            w = np.asarray(w0, dtype=np.float64)
            w = np.broadcast_to(w.reshape(1, -1), (K, F)) if w.size == F else w.reshape(K, F)
        self._w = torch.as_tensor(np.array(w, dtype=np.float64), device=dev)   # (a copy: w may be a read-only broadcast view)
        self.mat_pi0 = resolve_start_table(self.d, pi0, path_to_dir)
        self._mat_pi0_dev = torch.as_tensor(np.ascontiguousarray(self.mat_pi0, dtype=np.float32), device=dev)
        self._seeds_dev = torch.as_tensor(self.seeds.view(np.int64), device=dev)
        self._rn_seeds_dev = torch.as_tensor((self.seeds + np.uint64(RN_SEED_OFFSET)).view(np.int64), device=dev)
        self._shifts_dev = torch.as_tensor(self.shifts, device=dev)
        self._alphas_dev = torch.as_tensor(self.alpha_scales, device=dev)
        # the networks: owned copies, one stacked fp32 tensor per parameter ([1, ...] when shared)
        self._templates = [copy.deepcopy(n).to('cpu') for n in nets]
        self.per_learner_net = len(nets) > 1
        self._net_params = {}
        with torch.no_grad():
            for field, pname in NET_TENSORS:
                ts = [n.get_parameter(pname).detach().to(device=dev, dtype=torch.float32) for n in nets]
                self._net_params[field] = torch.stack(ts).contiguous()
        _, _, _, keep = ops.irl_pop_net_geometry(nets)
        st = L.RewardNetStruct()
        st.k1, st.f2, st.k2 = nets[0].conv1.kernel_size[0], nets[0].conv2.out_channels, nets[0].conv2.kernel_size[0]
        st.n3, st.n4 = nets[0].fc3.out_features, nets[0].fc4.out_features
        for field, _ in NET_TENSORS:
            setattr(st, field, self._net_params[field].data_ptr())
        st.keep_prob = keep
        self._net_struct = st
        self._rng_step = 0       # Philox step counter, shared by the learners (they advance in lock-step)
        self._reward_calls = 0   # AC_IRL's reward-call counter (dropout keys), shared likewise
        self._bufs = None

    # ------------------------------------------------------------------ state
    @property
    def K(self):
        return int(self._theta.shape[0])

    @property
    def thetas(self):
        return self._theta.cpu().numpy().copy()

    @property
    def w(self):
        return self._w.cpu().numpy().copy()

    def reward_net(self, k):
        """Learner k's reward network as a networks.RewardNet (a copy, on the population's device)."""
        if not 0 <= k < self.K:
            raise IndexError('learner %d of %d' % (k, self.K))
        j = k if self.per_learner_net else 0
        net = copy.deepcopy(self._templates[j])
        with torch.no_grad():
            for field, pname in NET_TENSORS:
                net.get_parameter(pname).copy_(self._net_params[field][j].cpu())
        return net.to(self.device)

    def _buffers(self):
        K, B, d, T = self.K, self.batch, self.d, self.episode_steps
        if self._bufs is None:
            dev, F = self.device, ops.num_features(d)
            sb = ops.irl_pop_workspace_slice(B, d, T)
            b = {'G': torch.zeros(K, F + 3, dtype=torch.float64, device=dev),
                 'ws': torch.zeros(K, sb // 8, dtype=torch.float64, device=dev)}
            if self.update_every == 'step':
                b['pi'] = torch.empty(K, B, d, dtype=torch.float32, device=dev)
                b['run'] = {'scratch': torch.empty(K, B, d, dtype=torch.float32, device=dev),
                            'P': torch.empty(K, B, d, d, dtype=torch.float32, device=dev),
                            'reward': torch.empty(K, B, dtype=torch.float32, device=dev),
                            'delta': torch.empty(K, B, dtype=torch.float64, device=dev),
                            'g': torch.empty(K, B, dtype=torch.float64, device=dev)}
            else:
                b['run'] = {'pi_traj': torch.empty(K, B, T + 1, d, dtype=torch.float32, device=dev),
                            'pi_last': torch.empty(K, B, d, dtype=torch.float32, device=dev),
                            'P': torch.empty(K, B, T, d, d, dtype=torch.float32, device=dev),
                            'reward': torch.empty(K, B, T, dtype=torch.float32, device=dev),
                            'delta': torch.empty(K, B, T, dtype=torch.float64, device=dev),
                            'g': torch.empty(K, B, T, dtype=torch.float64, device=dev)}
            self._bufs = b
        return self._bufs

    # ------------------------------------------------------------------ training
    @_with_ctx
    def train(self, num_episodes, gamma=1, constant=False, lr_critic=0.1, lr_actor=0.001, *, first_episode=0):
        """`num_episodes` episodes of every learner: AC_IRL.train(num_episodes, stop_criteria=-1, ...) under each learner's
        reward network (episodes numbered first_episode + 1 ... in the learning-rate schedule, as there).  lr_critic /
        lr_actor: scalars or [K].  Returns a NumPy array [K, num_episodes] of the per-episode returns as AC_IRL.train books
        them: step mode the sum of the T updates' mean rewards, rollout mode T x the update's mean reward per transition."""
        K, T = self.K, self.episode_steps
        num_episodes = int(num_episodes)
        if num_episodes < 0:
            raise ValueError('num_episodes < 0')
        if num_episodes == 0:
            return np.zeros((K, 0))
        lrc = torch.as_tensor(broadcast('lr_critic', lr_critic, K), device=self.device)
        lra = torch.as_tensor(broadcast('lr_actor', lr_actor, K), device=self.device)
        acc = torch.zeros(K, num_episodes, dtype=torch.float64, device=self.device)
        b = self._buffers()
        common = dict(first_step=self._rng_step, reward_acc=acc, precision=self.precision)
        if self.update_every == 'step':
            ops.train_episodes_irl_pop(self._mat_pi0_dev, b['pi'], T, num_episodes, first_episode + 1, constant, self._theta,
                                       self._shifts_dev, self._alphas_dev, self._w, gamma, lrc, lra, self._seeds_dev,
                                       self._net_struct, self.per_learner_net, self._rn_seeds_dev, self._reward_calls, b['G'],
                                       b['ws'], b['run'], **common)
            self._reward_calls += num_episodes * T
        else:
            ops.train_rollouts_irl_pop(self._mat_pi0_dev, T, num_episodes, first_episode + 1, constant, self._theta,
                                       self._shifts_dev, self._alphas_dev, self._w, gamma, lrc, lra, self._seeds_dev,
                                       self._net_struct, self.per_learner_net, self._rn_seeds_dev, self._reward_calls, b['G'],
                                       b['ws'], b['run'], **common)
            self._reward_calls += num_episodes
        self._rng_step += num_episodes * T
        out = acc.cpu().numpy()
        if self.update_every == 'rollout':
            out = out * T
        if self.precision == 'mixed' and self._ctx.status(synchronize=True):
            raise L.MfgError('a mixed-precision sampling launch of this population ran with |theta| (1/2 + |shift|) > 86 '
                             '(or theta not finite): its outputs are NaN; use precision=\'f64\', then clear_status()')
        return out

    def status(self, synchronize=True) -> int:
        """Bits of this population's status word (0 = healthy), shared by its K learners."""
        return self._ctx.status(synchronize)

    def clear_status(self):
        self._ctx.clear_status()

    def learner(self, k):
        """An AC_IRL holding learner k's theta, w, reward network, Philox position and reward-call counter.  Its
        construction leaves the global np.random stream (and torch's CPU generator) as they were."""
        if not 0 <= k < self.K:
            raise IndexError('learner %d of %d' % (k, self.K))
        net = self.reward_net(k)
        state = np.random.get_state()
        try:
            with torch.random.fork_rng(devices=[]):
                ac = AC_IRL(float(self.thetas[k]), float(self.shifts[k]), float(self.alpha_scales[k]), self.d,
                            reg=net.reg, n_fc3=net.fc3.out_features, n_fc4=net.fc4.out_features, pi0=self.mat_pi0,
                            demonstrations=[], batch=self.batch, seed=int(self.seeds[k]), update_every=self.update_every,
                            precision=self.precision, device=self.device, verbose=self.verbose)
        finally:
            np.random.set_state(state)
        ac.reward_net = net
        ac.create_training_method()
        ac.w = self.w[k]
        ac.theta = np.array([self.thetas[k]]) if self._rng_step else float(self.thetas[k])
        ac._rng_step = self._rng_step
        ac._reward_calls = self._reward_calls
        return ac
