"""Plain NumPy fp64 restatement of the forecast scores (mfg_forecast_score, include/mfg_hip.h), written from the definitions of
Gneiting & Raftery (JASA 2007), kernel forms with beta = 1 -- the double sums over (r, s), deliberately NOT the sorted form the
kernel uses -- and the error bounds the GPU tests derive from the inputs.  Not a test module: tests import it.

For cell (k, n, l) with members x_r (rows r N + n of traj[k]) and observation y:
    crps_c  = 1/R sum_r |x_rc - y_c|     - 1/(2 R^2) sum_{r,s} |x_rc - x_sc|
    energy  = 1/R sum_r ||x_r - y||_2    - 1/(2 R^2) sum_{r,s} ||x_r - x_s||_2
    less_c  = #{r : x_rc < y32_c},  equal_c = #{r : x_rc == y32_c}      (fp32 comparisons)
"""
import math

import numpy as np

TILE = 64           # members per tile of the kernel's energy pass (MFG_FORECAST_SCORE_TILE)
U = 2.0 ** -53


def members(traj_k, N, R):
    """[N R, H, d] -> [N, R, H, d]: member r of start state n is trajectory r N + n."""
    return traj_k.reshape(R, N, *traj_k.shape[1:]).transpose(1, 0, 2, 3)


def crps_column(x, y):
    """CRPS of the members x [R] (fp64) against y, and the sum of the absolute values of the terms added."""
    R = x.shape[0]
    first = np.abs(x - y)
    second = np.abs(x[:, None] - x[None, :])
    return first.sum() / R - second.sum() / (2.0 * R * R), first.sum() / R + second.sum() / (2.0 * R * R)


def energy_cell(x, y):
    """Energy score of the members x [R, d] (fp64) against y [d], and the sum of the absolute values of the terms added."""
    R = x.shape[0]
    first = np.sqrt(((x - y[None, :]) ** 2).sum(axis=-1))
    total = 0.0
    for r0 in range(0, R, 128):     # (row blocks only bound the temporary)
        total += np.sqrt(((x[r0:r0 + 128, None, :] - x[None, :, :]) ** 2).sum(axis=-1)).sum()
    return first.sum() / R - total / (2.0 * R * R), first.sum() / R + total / (2.0 * R * R)


def sorted_pair_sum(x):
    """sum_{r,s} |x_r - x_s| by the sorted identity 2 sum_i (2 i - R + 1) x_(i) (the kernel's route), and the sum of the
    absolute values of ITS terms."""
    R = x.shape[0]
    w = 2.0 * np.arange(R) - R + 1.0
    t = w * np.sort(x)
    return 2.0 * t.sum(), 2.0 * np.abs(t).sum()


def pairwise_depth(n):
    """An upper bound of the additions any one term passes through in np.sum over n contiguous values: blocks of at most 128
    go through eight accumulators (16 additions) and their fold (3), the blocks through a binary tree."""
    n = int(n)
    if n <= 8:
        return n
    return min(n - 1, 19 + max(0, math.ceil(math.log2(n / 128.0))))


def crps_chain(R):
    """The longest chain of additions of the kernel's two column sums: a lane adds ceil(R / 64) values, then six butterfly steps."""
    return -(-int(R) // 64) + 6


def energy_chain(R):
    """The longest chain of the kernel's pair sum: a thread meets at most 16 rows in each of the nt (nt + 1) / 2 tile pairs, then
    six butterfly steps and the four wave totals."""
    nt = -(-int(R) // TILE)
    return nt * (nt + 1) // 2 * (TILE // 4) + 6 + 4


def score(traj, emp32, emp64, N, R, want_energy=True):
    """The restatement on traj [K, N R, H, d] fp32, emp32 / emp64 [N, H, d]: a dict with crps, less, equal, energy, summary and
    the bounds crps_bound, energy_bound, summary_bound.  A bound is (a + b + d + 4) 2^-53 T: a the kernel's longest chain of
    additions, b NumPy's pairwise depth here, d for the squares under a norm, 4 for the divisions and the final subtraction, T
    the sum of the absolute values of the terms added -- the larger of this restatement's (the double sum) and the kernel's
    (the sorted form, whose terms (2 i - R + 1) x_(i) are larger than the differences they stand for)."""
    K, NR, H, d = traj.shape
    assert NR == N * R
    crps = np.zeros((K, N, H, d))
    crps_bound = np.zeros((K, N, H, d))
    less = np.zeros((K, N, H, d), dtype=np.int32)
    equal = np.zeros((K, N, H, d), dtype=np.int32)
    energy = np.zeros((K, N, H)) if want_energy else None
    energy_bound = np.zeros((K, N, H))
    fac_c = (crps_chain(R) + pairwise_depth(R * R) + d + 4) * U
    fac_e = (energy_chain(R) + pairwise_depth(R * R) + d + 4) * U
    for k in range(K):
        m = members(traj[k], N, R)
        for n in range(N):
            for l in range(H):
                x32 = m[n, :, l, :]
                x = x32.astype(np.float64)
                less[k, n, l] = (x32 < emp32[n, l][None, :]).sum(axis=0)
                equal[k, n, l] = (x32 == emp32[n, l][None, :]).sum(axis=0)
                for c in range(d):
                    crps[k, n, l, c], t_ref = crps_column(x[:, c], emp64[n, l, c])
                    t_ker = np.abs(x[:, c] - emp64[n, l, c]).sum() / R + sorted_pair_sum(x[:, c])[1] / (2.0 * R * R)
                    crps_bound[k, n, l, c] = fac_c * max(t_ref, t_ker)
                if want_energy:
                    energy[k, n, l], t = energy_cell(x, emp64[n, l])
                    energy_bound[k, n, l] = fac_e * t
    # the means: the kernel adds a cell's d values in column order, then a lane's cells, then six butterfly steps
    a_s = d + -(-N // 64) + 6
    summary = np.full((K, H, 2), np.nan)
    summary_bound = np.zeros((K, H, 2))
    summary[:, :, 0] = crps.mean(axis=(1, 3))
    summary_bound[:, :, 0] = crps_bound.mean(axis=(1, 3)) + (a_s + pairwise_depth(N * d) + 4) * U * np.abs(crps).mean(axis=(1, 3))
    if want_energy:
        summary[:, :, 1] = energy.mean(axis=1)
        summary_bound[:, :, 1] = energy_bound.mean(axis=1) + (a_s + pairwise_depth(N) + 4) * U * np.abs(energy).mean(axis=1)
    return dict(crps=crps, less=less, equal=equal, energy=energy, summary=summary, crps_bound=crps_bound,
                energy_bound=energy_bound, summary_bound=summary_bound)
