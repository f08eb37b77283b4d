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
