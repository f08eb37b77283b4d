"""NumPy restatement of mfg_demos_from_logs (include/mfg_hip.h, "Demonstrations from agent logs"): the yardstick of
tests/test_demos_host.py, tests/test_gpu_demos.py and tests/test_gpu_demos_hazards.py.  Counting is np.bincount, ranking is
Python's stable sorted(..., reverse=True) (equal keys stay in ascending raw id), every ratio is
np.float32(np.float64(a) / np.float64(b)): integers and floats alike are compared with array_equal, no tolerance anywhere.
simulate_logs draws agents with identities that follow given row-stochastic matrices."""
import numpy as np

BAD_VALUE, EMPTY_HOUR, FAILED = 1, 2, 4
INT_OUTPUTS = ('counts', 'moves', 'order', 'present', 'left', 'entered', 'status')
FLOAT_OUTPUTS = ('state', 'action')


def raw_counts(topic, C):
    """raw [N, H, C]: the agents of day n in category c at hour h (negative values and values >= C are absent)."""
    N, H, _ = topic.shape
    raw = np.zeros((N, H, C), np.int64)
    for n in range(N):
        for h in range(H):
            v = topic[n, h]
            raw[n, h] = np.bincount(v[(v >= 0) & (v < C)], minlength=C)
    return raw


def rank_by(keys):
    """rank [C] of the categories by decreasing key, ties by ascending id."""
    C = len(keys)
    by_rank = sorted(range(C), key=lambda c: int(keys[c]), reverse=True)
    rank = np.empty(C, np.int64)
    rank[by_rank] = np.arange(C)
    return rank


def ranks(topic, C, order, order_given=None):
    """(rank [N, C] with -1 for a dropped category, bad [N]: a given rank outside [-1, C))."""
    N = topic.shape[0]
    bad = np.zeros(N, bool)
    if order == 'given':
        g = np.broadcast_to(np.asarray(order_given, np.int64), (N, C)).copy()
        out = (g < -1) | (g >= C)
        g[out] = -1
        return g, out.any(1)
    raw = raw_counts(topic, C)
    if order == 'first_hour':
        return np.stack([rank_by(raw[n, 0]) for n in range(N)]), bad
    if order == 'total':
        return np.broadcast_to(rank_by(raw.sum((0, 1))), (N, C)).copy(), bad
    raise ValueError(order)


def finish(counts, moves, d, empty_row='uniform'):
    """Steps 5 to 7 from counts [N, H, width] and moves [N, H-1, width, width] (the second mode of the call)."""
    counts, moves = np.asarray(counts, np.int64), np.asarray(moves, np.int64)
    N, H, width = counts.shape
    neg_counts = (counts < 0).any(-1)                                   # [N, H]
    failed = neg_counts.copy()
    failed[:, :-1] |= (moves < 0).any((-1, -2))
    present = counts.sum(-1)
    row_total, col_total = moves.sum(-1), moves.sum(-2)
    with np.errstate(divide='ignore', invalid='ignore'):
        state = np.float32(np.float64(counts[..., :d]) / np.float64(present)[..., None])
        action = np.float32(np.float64(moves[..., :d, :d]) / np.float64(row_total[..., :d, None]))
    eye = np.eye(d, dtype=np.float32)
    uniform = np.full(d, np.float32(np.float64(1) / np.float64(d)), np.float32)
    for n, h, i in zip(*np.nonzero(row_total[..., :d] == 0)):
        action[n, h, i] = uniform if counts[n, h, i] == 0 and empty_row == 'uniform' else eye[i]
    left, entered = counts[:, :-1] - row_total, counts[:, 1:] - col_total
    state[failed] = np.nan
    action[failed[:, :-1]] = np.nan
    left[failed[:, :-1]] = -1
    entered[failed[:, :-1] | neg_counts[:, 1:]] = -1
    status = (np.where(((present == 0) & ~failed).any(1), EMPTY_HOUR, 0) | np.where(failed.any(1), FAILED, 0)).astype(np.int32)
    present = np.where(failed, -1, present)
    return {'state': state, 'action': action, 'present': present.astype(np.int32), 'left': left.astype(np.int32),
            'entered': entered.astype(np.int32), 'status': status}


def from_logs(topic, C, d, width=None, order='first_hour', order_given=None, empty_row='uniform'):
    """Every output of the call from topic [N, H, U]."""
    topic = np.asarray(topic)
    N, H, U = topic.shape
    width = d if width is None else width
    assert 1 <= d <= width <= min(C, 64) and H >= 2
    rank, bad = ranks(topic, C, order, order_given)
    by_rank = np.full((N, C), -1, np.int32)
    for n in range(N):
        for c in range(C):
            if rank[n, c] >= 0:
                by_rank[n, rank[n, c]] = c
    W1 = width + 1
    cur = np.full((N, H, U), width, np.int64)                           # `width`: absent
    for n in range(N):
        seen = (topic[n] >= 0) & (topic[n] < C)
        r = rank[n][topic[n][seen]]
        cur[n][seen] = np.where((r >= 0) & (r < width), r, width)
    counts, moves = np.zeros((N, H, width), np.int64), np.zeros((N, H - 1, width, width), np.int64)
    for n in range(N):
        for h in range(H):
            counts[n, h] = np.bincount(cur[n, h], minlength=W1)[:width]
        for h in range(H - 1):
            moves[n, h] = np.bincount(cur[n, h] * W1 + cur[n, h + 1], minlength=W1 * W1).reshape(W1, W1)[:width, :width]
    out = finish(counts, moves, d, empty_row)
    out['status'] = (out['status'] | np.where(bad | (topic >= C).any((1, 2)), BAD_VALUE, 0)).astype(np.int32)
    out.update(counts=counts.astype(np.int32), moves=moves.astype(np.int32), order=by_rank)
    return out


def simulate_logs(P, pi0, U, H, seed):
    """topic [H, U] int32 of one day: U agents with identities, hour 0 drawn from pi0 [d], agent u at topic i at hour h moves to
    a topic drawn from P[h, i, :] (P [H-1, d, d], or one [d, d] for every hour).  Nobody is absent: a closed population."""
    P, pi0 = np.asarray(P, np.float64), np.asarray(pi0, np.float64)
    d = len(pi0)
    P = np.broadcast_to(P, (H - 1, d, d))
    rs = np.random.RandomState(seed)
    topic = np.empty((H, U), np.int32)
    topic[0] = np.minimum((rs.random_sample(U)[:, None] >= np.cumsum(pi0)[None, :]).sum(1), d - 1)
    for h in range(H - 1):
        cum = np.cumsum(P[h], axis=1)
        topic[h + 1] = np.minimum((rs.random_sample(U)[:, None] >= cum[topic[h]]).sum(1), d - 1)
    return topic


def same(a, b):
    """array_equal with NaN equal to NaN (shape and dtype included)."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and bool(np.array_equal(a, b, equal_nan=a.dtype.kind == 'f'))


def differing(got, want, names=None):
    """Names of the outputs of `got` (NumPy arrays or tensors) that are not the restatement's."""
    bad = []
    for name in (names or want):
        g = got[name]
        g = g.detach().cpu().numpy() if hasattr(g, 'detach') else np.asarray(g)
        if not same(g, want[name]):
            bad.append(name)
    return bad
