"""NumPy restatement of mfg_demos_bootstrap and mfg_replicate_bands (include/mfg_hip.h, "Bootstrap replicates of the
demonstrations"): the yardstick of tests/test_demos_boot_host.py and tests/test_gpu_demos_bootstrap.py.  The weights come from
oracle/philox_ref.philox4x32_10 and the twelve literals of the header; weighted counts and moves are np.bincount(..., weights)
of integer weights (exact in fp64: a cell is at most 12 (2^31 - 1) / 12), steps 5 to 7 are demos_ref.finish over the R N days.
Everything is compared with demos_ref.same: no tolerance."""
import numpy as np

import demos_ref as D
from oracle import philox_ref

TAG = 0xB007                      # MFG_DEMOS_BOOT_TAG
TABLE = (1580030168, 3160060337, 3950075421, 4213413783, 4279248373, 4292415291, 4294609777, 4294923276, 4294962463, 4294966817,
         4294967252, 4294967292)  # MFG_DEMOS_BOOT_TABLE
UNITS = ('agent_day', 'agent')
OUTPUTS = ('state', 'action', 'counts', 'moves', 'present', 'left', 'entered', 'status')


def weight_of(x):
    """w = #{k < 12 : x >= T[k]} of uint32 words."""
    x = np.asarray(x, np.uint64)
    return (x[..., None] >= np.asarray(TABLE, np.uint64)).sum(-1).astype(np.int64)


def weights(R, N, U, seed, unit='agent_day', day_offset=0, agents=None):
    """w [R, N, U] int64 (agents: the agent indices, default arange(U))."""
    assert unit in UNITS
    u = np.arange(U, dtype=np.uint64) if agents is None else np.asarray(agents, np.uint64)
    key = np.zeros(N, np.uint64) if unit == 'agent' else (np.uint64(day_offset) + np.arange(N, dtype=np.uint64))
    c1 = (key & np.uint64(0xFFFFFFFF))[:, None]
    c3 = (np.uint64(TAG) | ((key >> np.uint64(32)) << np.uint64(16)))[:, None]
    out = np.empty((R, N, len(u)), np.int64)
    for quad in range((R + 3) // 4):
        x = philox_ref.philox4x32_10(u[None, :], c1, np.uint64(quad), c3, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
        for r in range(4 * quad, min(R, 4 * quad + 4)):
            out[r] = weight_of(x[r & 3])
    return out


def bootstrap(topic, rank, C, d, R, seed, width=None, unit='agent_day', day_offset=0, empty_row='uniform'):
    """Every output of the call, with a leading R."""
    topic = np.asarray(topic)
    N, H, U = topic.shape
    width = d if width is None else width
    W1 = width + 1
    g, bad = D.ranks(topic, C, 'given', np.atleast_2d(rank))
    cur = np.full((N, H, U), width, np.int64)
    for n in range(N):
        seen = (topic[n] >= 0) & (topic[n] < C)
        r = g[n][topic[n][seen]]
        cur[n][seen] = np.where((r >= 0) & (r < width), r, width)
    w = weights(R, N, U, seed, unit, day_offset)
    counts, moves = np.zeros((R, N, H, width), np.int64), np.zeros((R, N, H - 1, width, width), np.int64)
    for r in range(R):
        for n in range(N):
            wf = w[r, n].astype(np.float64)
            for h in range(H):
                counts[r, n, h] = np.bincount(cur[n, h], weights=wf, minlength=W1)[:width].astype(np.int64)
            for h in range(H - 1):
                moves[r, n, h] = np.bincount(cur[n, h] * W1 + cur[n, h + 1], weights=wf,
                                             minlength=W1 * W1).reshape(W1, W1)[:width, :width].astype(np.int64)
    out = D.finish(counts.reshape(R * N, H, width), moves.reshape(R * N, H - 1, width, width), d, empty_row)
    out = {k: v.reshape((R, N) + v.shape[1:]) for k, v in out.items()}
    bad_day = np.where(bad | (topic >= C).any((1, 2)), D.BAD_VALUE, 0)
    out['status'] = (out['status'] | bad_day[None, :]).astype(np.int32)
    out.update(counts=counts.astype(np.int32), moves=moves.astype(np.int32))
    return out


def resampled_log(topic_day, w):
    """The log [H, sum w] of one day in which agent u appears w[u] times."""
    return np.repeat(np.asarray(topic_day), np.asarray(w, np.int64), axis=1)


def bands(x, ranks):
    """(mean, std, quant) over axis 0 of x [R, ...] fp32: fp64 sums in the order r = 0 .. R - 1 (np.cumsum adds in sequence),
    every operation rounded on its own; the order statistics are elements.  A cell with a NaN is NaN in all three."""
    x = np.asarray(x, np.float32)
    R = x.shape[0]
    x64 = x.astype(np.float64)
    nan = np.isnan(x).any(0)
    mean = np.cumsum(x64, axis=0)[-1] / np.float64(R)
    e = x64 - mean
    std = np.sqrt(np.cumsum(e * e, axis=0)[-1] / np.float64(R))
    srt = np.sort(np.where(nan, np.float32(0), x), axis=0)
    quant = np.stack([srt[q] for q in ranks]) if len(ranks) else np.empty((0,) + x.shape[1:], np.float32)
    mean, std, quant = mean.copy(), std.copy(), quant.astype(np.float32)
    mean[nan], std[nan] = np.nan, np.nan
    quant[:, nan] = np.nan
    return mean, std, quant
