"""Plain NumPy restatement of one finite-population step (mfg_agents_step_pop, include/mfg_hip.h), written from the definition in
the header comment on oracle/philox_ref.philox4x32_10.  The whole state is integer, and the thresholds are defined operation
by operation in fp64, so the kernel is compared with this bit for bit."""
import numpy as np

from oracle.philox_ref import philox4x32_10

TWO32 = 4294967296.0


def thresholds(P):
    """(t [d, d] int64 in [0, 2^32], S_last [d] fp64) of an action P [d, d] fp32: S_ic the sequential fp64 row sums (np.cumsum
    adds in column order), t_ic = floor(S_ic / S_i,d-1 2^32) clamped; rows with an unusable S_last get t = 0."""
    S = np.cumsum(np.asarray(P, dtype=np.float32).astype(np.float64), axis=1)
    last = S[:, -1].copy()
    ok = np.isfinite(last) & (last > 0)
    with np.errstate(all='ignore'):
        q = S / np.where(ok, last, 1.0)[:, None] * TWO32
    t = np.where(ok[:, None], np.clip(np.floor(np.where(np.isnan(q), 0.0, q)), 0.0, TWO32), 0.0)
    return t.astype(np.int64), last


def words(seed, step, j, i, n):
    """The words of agents 0 .. n - 1 of topic i of member j: word a mod 4 of the block with c0 = 0x80000000 | i << 22 | a >> 2."""
    a = np.arange(n, dtype=np.int64)
    seed, j = int(seed) & 0xFFFFFFFFFFFFFFFF, int(j)
    r = philox4x32_10(0x80000000 | (i << 22) | (a >> 2), int(step), j & 0xFFFFFFFF, (j >> 32) & 0xFFFF, seed & 0xFFFFFFFF, seed >> 32)
    return np.stack(r)[a & 3, a].astype(np.int64)


def step(counts, P, agents, seed, step_, j):
    """One member: (counts_next [d] int32, moves [d, d] int32, pi_next [d] fp32); -1 / NaN for a member that fails."""
    counts = np.asarray(counts, dtype=np.int64)
    d = counts.shape[0]
    t, last = thresholds(P)
    bad = np.any(counts < 0) or np.any(counts > agents) or np.any((counts > 0) & ~(np.isfinite(last) & (last > 0)))
    if bad:
        return np.full(d, -1, np.int32), np.full((d, d), -1, np.int32), np.full(d, np.nan, np.float32)
    moves = np.zeros((d, d), dtype=np.int64)
    for i in range(d):
        if counts[i]:
            w = words(seed, step_, j, i, int(counts[i]))
            col = (w[:, None] < t[i][None, :]).argmax(axis=1)          # the first column with w < t
            moves[i] = np.bincount(col, minlength=d)
    nxt = moves.sum(axis=0)
    return nxt.astype(np.int32), moves.astype(np.int32), (nxt.astype(np.float64) / float(agents)).astype(np.float32)


def step_members(counts, P, seed, step_, js):
    """counts_next [M, d] int64 of the M members `js` that share the counts [d] and the action P (no negative entry, all rows usable): the same
    integers as step(), a row's words formed for all members at once."""
    counts, js = np.asarray(counts, dtype=np.int64), np.asarray(js, dtype=np.uint64)
    d, seed = counts.shape[0], int(seed) & 0xFFFFFFFFFFFFFFFF
    t, _ = thresholds(P)
    nxt = np.zeros((js.shape[0], d), dtype=np.int64)
    for i in range(d):
        n = int(counts[i])
        if n:
            q = np.arange((n + 3) // 4, dtype=np.int64)
            r = philox4x32_10((0x80000000 | (i << 22) | q)[None, :], int(step_), (js & np.uint64(0xFFFFFFFF))[:, None],
                              ((js >> np.uint64(32)) & np.uint64(0xFFFF))[:, None], seed & 0xFFFFFFFF, seed >> 32)
            w = np.stack(r, axis=-1).reshape(js.shape[0], -1)[:, :n].astype(np.int64)      # agent a: word a mod 4 of block a >> 2
            for c in range(d):
                lo = t[i, c - 1] if c else 0
                nxt[:, c] += ((w < t[i, c]) & (w >= lo)).sum(axis=1) if t[i, c] > lo else 0
    return nxt


def step_pop(counts, P, agents, seeds, step_, traj_offset=0):
    """counts [K, B, d], P [K, B, d, d], seeds [K] -> (counts_next, moves, pi_next) of every member (id traj_offset + b)."""
    K, B, d = counts.shape
    out = [[step(counts[k, b], P[k, b], agents, seeds[k], step_, traj_offset + b) for b in range(B)] for k in range(K)]
    pick = lambda q: np.array([[m[q] for m in row] for row in out]).reshape((K, B) + out[0][0][q].shape) if B else None
    return pick(0), pick(1), pick(2)
