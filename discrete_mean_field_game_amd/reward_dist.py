"""The numbers behind the reference's reward-distribution figures (plot_reward_distribution and its two siblings,
ac_irl.py:1046-1263), shared by AC_IRL.reward_distribution and AC_IRLPopulation.reward_distribution: the histogram and the
Gaussian KDE of four reward sets per learner, reduced on the device (ops.row_distribution, one launch per set for all
learners), ONE host read, and the three JSDs between the histograms on the host.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import ops

SETS = ('demo_train', 'demo_test', 'gen_train', 'gen_test')
# the reference's three JSDs, in its order (ac_irl.py:1121-1123): demo train / demo test, demo train / generated from train
# start states, demo test / generated from test start states
JSD_PAIRS = ((0, 1), (0, 2), (1, 3))
STATUS_MISSING = -1           # status of a set that was not given (no test demonstrations / no test start table)


@dataclass
class RewardDistribution:
    """K learners' reward distributions over the four sets of `sets` (AC_IRL.reward_distribution: without the leading K).
    moments [K,4,6]: values kept by the histogram, min, max, mean, variance (ddof 1), KDE bandwidth variance; counts
    [K,4,bins] int64 and edges [K,4,bins+1]: np.histogram of the set; xs [G] and density [K,4,G]: gaussian_kde of the set on
    linspace(xmin, xmax, G); jsd [K,3]: the pairs of JSD_PAIRS; status [K,4] int32: 0, _lib.DIST_NONFINITE (NaN row: a failed
    learner), _lib.DIST_NO_KDE (NaN density) or STATUS_MISSING; rewards: None, or the four fp32 arrays [K,N_s] (None for a
    missing set) the statistics were taken from."""
    sets: tuple
    moments: np.ndarray
    counts: np.ndarray
    edges: np.ndarray
    xs: np.ndarray
    density: np.ndarray
    jsd: np.ndarray
    status: np.ndarray
    rewards: Optional[tuple] = None


def host_jsd(p, q):
    """actor_critic.JSD (mfg_ac2.py:546-563) of two histograms, on the host in fp64: zeros become 1e-100, M = (P + Q) / 2, and
    0.5 (KL(P || M) + KL(Q || M)) with P, Q and M each renormalised to sum 1 (scipy.stats.entropy's rule).  The arguments are
    copied, not written."""
    p = np.array(p, dtype=np.float64)
    q = np.array(q, dtype=np.float64)
    p[p == 0] = 1e-100
    q[q == 0] = 1e-100
    m = 0.5 * (p + q)
    p, q, m = p / p.sum(), q / q.sum(), m / m.sum()
    return 0.5 * (float(np.sum(p * np.log(p / m))) + float(np.sum(q * np.log(q / m))))


def summarise(rewards, K, device, num_bins=20, xmin=-0.1, xmax=0.4, num_points=200, hist_range=None, want_rewards=False):
    """rewards: four entries in the order of SETS, each a device fp32 tensor [K, N_s] or None (a missing set).  One
    ops.row_distribution launch per given set, all outputs in one device buffer, one host read.  Returns a RewardDistribution
    with the leading K."""
    bins, G = int(num_bins), int(num_points)
    S = len(SETS)
    # one buffer of 8-byte words: moments | counts | edges | density | status (int32, padded)
    sizes = (S * K * 6, S * K * bins, S * K * (bins + 1), S * K * G, (S * K + 1) // 2)
    offs = np.concatenate([[0], np.cumsum(sizes)])
    buf = torch.zeros(int(offs[-1]), dtype=torch.float64, device=device)

    def view(i, dtype, *shape):
        return buf[int(offs[i]):int(offs[i + 1])].view(dtype)[:int(np.prod(shape))].view(*shape)
    dev = {'moments': view(0, torch.float64, S, K, 6), 'counts': view(1, torch.int64, S, K, bins),
           'edges': view(2, torch.float64, S, K, bins + 1), 'density': view(3, torch.float64, S, K, G) if G else None,
           'status': view(4, torch.int32, S, K)}
    for s, r in enumerate(rewards):
        if r is None:
            continue
        ops.row_distribution(r, bins=bins, hist_range=hist_range, G=G, x_lo=xmin, x_hi=xmax,
                             out={name: (t[s] if t is not None else None) for name, t in dev.items()})
    host = buf.cpu()                                            # the one host read

    def hview(i, dtype, *shape):
        return host[int(offs[i]):int(offs[i + 1])].view(dtype)[:int(np.prod(shape))].view(*shape).numpy()
    moments = hview(0, torch.float64, S, K, 6).transpose(1, 0, 2).copy()
    counts = hview(1, torch.int64, S, K, bins).transpose(1, 0, 2).copy()
    edges = hview(2, torch.float64, S, K, bins + 1).transpose(1, 0, 2).copy()
    density = (hview(3, torch.float64, S, K, G).transpose(1, 0, 2).copy() if G else np.zeros((K, S, 0)))
    status = hview(4, torch.int32, S, K).T.copy()
    for s, r in enumerate(rewards):
        if r is None:
            moments[:, s] = np.nan
            edges[:, s] = np.nan
            density[:, s] = np.nan
            status[:, s] = STATUS_MISSING
    jsd = np.full((K, len(JSD_PAIRS)), np.nan)
    for k in range(K):
        for j, (a, b) in enumerate(JSD_PAIRS):
            if status[k, a] in (0, 2) and status[k, b] in (0, 2):
                jsd[k, j] = host_jsd(counts[k, a], counts[k, b])
    kept = None
    if want_rewards:
        kept = tuple(None if r is None else r.cpu().numpy() for r in rewards)
    return RewardDistribution(SETS, moments, counts, edges, np.linspace(float(xmin), float(xmax), G), density, jsd, status, kept)


def squeeze(dist):
    """The single-learner form of a K = 1 RewardDistribution: every array without its leading K."""
    rewards = None if dist.rewards is None else tuple(None if r is None else r[0] for r in dist.rewards)
    return RewardDistribution(dist.sets, dist.moments[0], dist.counts[0], dist.edges[0], dist.xs, dist.density[0], dist.jsd[0],
                              dist.status[0], rewards)


# ---------------------------------------------------------------------------------------------------------------------
# Reward sensitivities: the mean input gradients of the reward network over the same four sets (AC_IRLPopulation /
# AC_IRL.reward_sensitivity), and the prototypes of plot_reward_heatmap (ac_irl.py:1378-1443)
# ---------------------------------------------------------------------------------------------------------------------
@dataclass
class RewardSensitivity:
    """K learners' reward sensitivities over the four sets of `sets` (AC_IRL.reward_sensitivity: without the leading K).
    grad_state [K,4,d] / grad_action [K,4,d,d]: the mean over the set's transitions of d r / d state and d r / d action (fp64
    means of the fp32 per-sample gradients); gxi_state / gxi_action: the same shapes, the mean of gradient x input; count [4]:
    transitions per set (0: missing); status [K,4] int32: 0, _lib.DIST_NONFINITE (a failed learner: NaN rows) or
    STATUS_MISSING (NaN); rewards: the four fp32 arrays [K,N_s] of the forwards (None for a missing set); samples: None, or
    per set (None when missing) a pair (grad_state [K,N_s,d], grad_action [K,N_s,d,d]) of fp32 arrays.
    Topics are ordered by popularity: the lower triangle of grad_action is mass moved towards MORE popular topics."""
    sets: tuple
    grad_state: np.ndarray
    grad_action: np.ndarray
    gxi_state: np.ndarray
    gxi_action: np.ndarray
    count: np.ndarray
    status: np.ndarray
    rewards: Optional[tuple] = None
    samples: Optional[tuple] = None

    def learner(self, k):
        """Learner k's RewardSensitivity, without the leading K."""
        pick = lambda t: None if t is None else tuple(None if x is None else (tuple(y[k] for y in x) if isinstance(x, tuple) else x[k])
                                                      for x in t)
        return RewardSensitivity(self.sets, self.grad_state[k], self.grad_action[k], self.gxi_state[k], self.gxi_action[k],
                                 self.count, self.status[k], pick(self.rewards), pick(self.samples))


def sensitivity(inputs, K, d, active, device, run, want_samples=False):
    """inputs: four entries in the order of SETS, each (state, action) device tensors (shared [N,d] / [N,d,d] or per-learner
    [K,N,d] / [K,N,d,d]) or None.  run(s, state, action, reward, bufs): one population forward of the learners `active` with
    the input-gradient block bound, writing reward [K,N] and bufs (mean_state [K,2,d], mean_action [K,2,d,d], with
    want_samples grad_state / grad_action).  All means live in one device buffer: ONE host read (more for the rewards and the
    per-sample arrays).  Returns a RewardSensitivity with the leading K."""
    from . import _lib as L
    S, E = len(SETS), d + d * d
    buf = torch.full((S * K * 2 * E,), float('nan'), dtype=torch.float64, device=device)
    rewards, samples = [None] * S, [None] * S
    count = np.zeros(S, dtype=np.int64)
    status = np.full((K, S), STATUS_MISSING, dtype=np.int32)
    for s, inp in enumerate(inputs):
        if inp is None:
            continue
        st, ac = inp
        N = int(st.shape[-2])
        count[s] = N
        status[:, s] = L.DIST_NONFINITE
        status[list(active), s] = 0
        base = s * K * 2 * E
        bufs = {'mean_state': buf[base:base + K * 2 * d].view(K, 2, d),
                'mean_action': buf[base + K * 2 * d:base + K * 2 * E].view(K, 2, d, d)}
        if want_samples:
            bufs['grad_state'] = torch.full((K, N, d), float('nan'), dtype=torch.float32, device=device)
            bufs['grad_action'] = torch.full((K, N, d, d), float('nan'), dtype=torch.float32, device=device)
        rewards[s] = torch.full((K, N), float('nan'), dtype=torch.float32, device=device)
        if active:
            run(s, st, ac, rewards[s], bufs)
        if want_samples:
            samples[s] = (bufs['grad_state'], bufs['grad_action'])
    host = buf.cpu().numpy().reshape(S, K * 2 * E)              # the one host read; per set: mean_state | mean_action
    ms = host[:, :K * 2 * d].reshape(S, K, 2, d).transpose(1, 0, 2, 3)
    ma = host[:, K * 2 * d:].reshape(S, K, 2, d, d).transpose(1, 0, 2, 3, 4)
    kept = tuple(None if r is None else r.cpu().numpy() for r in rewards)
    smp = tuple(None if x is None else (x[0].cpu().numpy(), x[1].cpu().numpy()) for x in samples) if want_samples else None
    return RewardSensitivity(SETS, ms[:, :, 0].copy(), ma[:, :, 0].copy(), ms[:, :, 1].copy(), ma[:, :, 1].copy(), count, status,
                             kept, smp)


def heatmap_states(mat_pi0, d):
    """The three prototype states of plot_reward_heatmap, [3,d] fp32: the first row of the start table; weight 2^(d-i) on topic
    i (heavy ... light), normalised in fp32; uniform."""
    s2 = np.zeros(d, dtype=np.float32)
    for i in range(d):
        s2[i] = 2 ** (d - i)
    s2 = s2 / np.sum(s2)
    return np.stack([np.asarray(mat_pi0, dtype=np.float64)[0, :d].astype(np.float32), s2,
                     np.ones(d, dtype=np.float32) / np.float32(d)])


def heatmap_actions(action1):
    """The three prototype actions per learner, [K,3,d,d] fp32, from action1 [K,d,d] (mass moves towards more popular topics):
    action1, the uniform matrix, and action1 with every row reversed (towards less popular topics)."""
    a1 = np.asarray(action1, dtype=np.float32)
    K, d, _ = a1.shape
    uni = np.broadcast_to(np.ones((d, d), dtype=np.float32) / np.float32(d), (K, d, d))
    return np.ascontiguousarray(np.stack([a1, uni, a1[:, :, ::-1]], axis=1))


def heatmap_pairs(states, actions, K, d):
    """The nine (state, action) pairs per learner, state-major: ([K,9,d], [K,9,d,d]) fp32 from states [3,d] and actions
    [3,d,d] or [K,3,d,d]; ValueError for other shapes."""
    states = np.asarray(states, dtype=np.float32)
    actions = np.asarray(actions, dtype=np.float32)
    if states.shape != (3, d):
        raise ValueError('states: expected [3, %d], got %s' % (d, list(states.shape)))
    if actions.shape == (3, d, d):
        actions = np.broadcast_to(actions, (K, 3, d, d))
    if actions.shape != (K, 3, d, d):
        raise ValueError('actions: expected [3, %d, %d] or [%d, 3, %d, %d], got %s' % (d, d, K, d, d, list(actions.shape)))
    st = np.ascontiguousarray(np.broadcast_to(states[None, :, None, :], (K, 3, 3, d)).reshape(K, 9, d))
    ac = np.ascontiguousarray(np.broadcast_to(actions[:, None], (K, 3, 3, d, d)).reshape(K, 9, d, d))
    return st, ac, states, np.ascontiguousarray(actions)
