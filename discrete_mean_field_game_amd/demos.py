"""Demonstrations from agent logs: the first stage of the paper's pipeline, the one the reference leaves to a recorder that is
not part of it.  A log says which of C categories each of U agents was in at each hour of each day; from_logs counts it on the
device (ops.demos_from_logs, C ABI mfg_demos_from_logs: the definitions are in include/mfg_hip.h) into the states pi [d] and
actions P [d,d] that AC_IRL / AC_IRLPopulation take as demonstrations, the start table of the forward learners and the day
tables [N,H,d] of Validation, forecast_score, var.fit_population and rnn.fit_population.  from_moves does the same for integer
tables that exist already (ops.agents_step_pop): finite-population rollouts under a known policy become synthetic
demonstrations by the same bits.

What is the reference's: the ranking by the first hour's popularity (reorder, mfg_ac2.py:58-81), the normalisation over the
recorded width followed by the [0:d] slice (normalize, :116-137; init_pi0), the repair of empty action rows (convert_action,
ac_irl.py:116-157) and the file layout Demonstrations.write produces.  What is this project's: the log format, the counting,
order='total' / 'given', the churn tables `left` / `entered` and the status bits."""
import os

import numpy as np

from . import _lib as L

ARRAYS = ('state', 'action', 'counts', 'moves', 'order', 'present', 'left', 'entered', 'status')
BUDGET = 1 << 30          # device bytes of the log of one ops.demos_from_logs call of from_logs (more days go in chunks)


class Demonstrations:
    """The arrays of mfg_demos_from_logs for N days of H hours as NumPy: state [N,H,d] and action [N,H-1,d,d] fp32, counts
    [N,H,width], moves [N,H-1,width,width], present [N,H], left / entered [N,H-1,width], status [N] int32, and order [N,C]
    (rank -> raw category; None from from_moves)."""

    def __init__(self, arrays, d, width, empty_row='uniform'):
        if empty_row not in L.DEMOS_EMPTY_ROWS:
            raise ValueError('empty_row=%r: one of %s' % (empty_row, sorted(L.DEMOS_EMPTY_ROWS)))
        self.d, self.width, self.empty_row = int(d), int(width), empty_row
        for name in ARRAYS:
            a = arrays.get(name)
            setattr(self, name, None if a is None else np.asarray(a))
        self.N, self.H = self.state.shape[:2]
        if self.state.shape != (self.N, self.H, self.d) or self.action.shape != (self.N, self.H - 1, self.d, self.d):
            raise ValueError('state %s / action %s: expected [N, H, %d] and [N, H-1, %d, %d]'
                             % (self.state.shape, self.action.shape, self.d, self.d, self.d))
        if self.counts.shape != (self.N, self.H, self.width) or self.moves.shape != (self.N, self.H - 1, self.width, self.width):
            raise ValueError('counts %s / moves %s: expected width %d' % (self.counts.shape, self.moves.shape, self.width))

    def _days(self, days):
        days = range(self.N) if days is None else [int(n) for n in days]
        if any(not 0 <= n < self.N for n in days):
            raise ValueError('days outside [0, %d)' % self.N)
        return list(days)

    def demonstrations(self, days=None):
        """The list-of-trajectories form of AC_IRL(demonstrations=...) and AC_IRLPopulation: per day H - 1 pairs
        (state [d], action [d,d]) in fp64 (H = 16 gives the reference's 15)."""
        return [[(self.state[n, h].astype(np.float64), self.action[n, h].astype(np.float64)) for h in range(self.H - 1)]
                for n in self._days(days)]

    def pi0(self, days=None):
        """The start table [days, d] fp64: every day's first hour."""
        return self.state[self._days(days), 0].astype(np.float64)

    def emp(self, days=None):
        """The day table [days, H, d] fp64 of Validation(emp=...), forecast_score, var.fit_population, rnn.fit_population."""
        return self.state[self._days(days)].astype(np.float64)

    def closed(self):
        """[N] bool: nobody left or entered the recorded set on that day (left and entered all 0)."""
        return ~(self.left != 0).any((1, 2)) & ~(self.entered != 0).any((1, 2))

    def full_rows(self):
        """(state [N,H,width], action [N,H-1,width,width]) fp32 over the recorded width, by the definitions of the device call
        (their [..., :d] blocks are `state` and `action`): what the reference's files hold."""
        counts, moves = self.counts.astype(np.float64), self.moves.astype(np.float64)
        failed = self.present < 0
        with np.errstate(divide='ignore', invalid='ignore'):
            state = np.float32(counts / np.where(failed, np.nan, self.present).astype(np.float64)[..., None])
            row_total = moves.sum(-1)
            action = np.float32(moves / row_total[..., None])
        eye = np.eye(self.width, dtype=np.float32)
        uniform = np.full(self.width, np.float32(np.float64(1) / np.float64(self.d)))
        for n, h, i in zip(*np.nonzero(row_total == 0)):
            action[n, h, i] = uniform if self.counts[n, h, i] == 0 and self.empty_row == 'uniform' else eye[i]
        action[failed[:, :-1]] = np.nan
        return state, action

    def write(self, state_dir, action_dir, start_day=1):
        """The reference's layout: state_dir/trend_distribution_day%d.csv (H rows of `width` values, space separated, %.3e) and
        action_dir/action_day%d.txt (`width` rows per hour, a blank line between hours, as convert_action writes), days
        numbered from start_day.  AC_IRL.read_demonstrations(state_dir, action_dir, dim_action=width, start_day) and init_pi0
        read them back."""
        state, action = self.full_rows()
        os.makedirs(state_dir, exist_ok=True)
        os.makedirs(action_dir, exist_ok=True)
        line = lambda row: ' '.join('%.3e' % x for x in row) + '\n'
        for n in range(self.N):
            with open(os.path.join(state_dir, 'trend_distribution_day%d.csv' % (start_day + n)), 'w') as f:
                f.writelines(line(row) for row in state[n])
            with open(os.path.join(action_dir, 'action_day%d.txt' % (start_day + n)), 'w') as f:
                f.write('\n'.join(''.join(line(row) for row in action[n, h]) for h in range(self.H - 1)))


def _device(device):
    import torch
    if device is None:
        device = 'cuda'
    return torch.device(device)


def _to_device_i32(x, dev):
    import torch
    t = x if isinstance(x, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(x))
    if t.dtype not in (torch.int8, torch.int16, torch.int32, torch.int64, torch.uint8):
        raise ValueError('expected an integer array, got %s' % t.dtype)
    return t.to(device=dev, dtype=torch.int32).contiguous()


def check_from_logs_args(topic_shape, d, categories, width=None, order='first_hour', empty_row='uniform', layout='nhu'):
    """The argument rules of from_logs that need no GPU (ValueError).  Returns (N, H, U, C, d, width) of the [N, H, U] form."""
    from . import ops
    if layout not in ('nhu', 'nuh'):
        raise ValueError('layout=%r: \'nhu\' (day, hour, agent) or \'nuh\' (day, agent, hour)' % (layout,))
    if len(topic_shape) != 3:
        raise ValueError('topic: expected three axes (%s), got %s' % (layout, tuple(topic_shape),))
    N, a, b = (int(s) for s in topic_shape)
    H, U = (a, b) if layout == 'nhu' else (b, a)
    given = (1, int(categories)) if order == 'given' else None          # (the table itself is checked where it is sliced)
    return ops.check_demos_args((N, H, U), categories, d, width, order, given, empty_row)


def from_logs(topic, d, *, categories=None, width=None, order='first_hour', order_given=None, empty_row='uniform', layout='nhu',
              device=None, budget=None):
    """Demonstrations counted from a log: topic [N, H, U] (layout='nhu': day, hour, agent) or [N, U, H] ('nuh', transposed on
    the device), integers, NumPy or a tensor: the category in [0, categories) of every agent at every hour, negative when
    absent.  categories: None takes max + 1.  d: the model's topics; width (default d): the recorded width over which states
    are normalised, the reference's dim_action.  order: 'first_hour' (per day, the reference's reorder), 'total' (one ranking
    for all days) or 'given' with order_given [N, C], [1, C] or [C] of ranks (-1 drops a category).  The days go to the device
    in chunks whose log stays within `budget` bytes (None: BUDGET), as population.consistency does; order='total' ranks over
    every day and so needs them in one chunk.  Returns a Demonstrations."""
    import torch
    from . import ops
    from .population import consistency_chunks
    is_tensor = isinstance(topic, torch.Tensor)
    if not is_tensor:
        topic = np.asarray(topic)
    if categories is None:
        if (topic.numel() if is_tensor else topic.size) == 0:
            raise ValueError('topic is empty')
        categories = int(topic.max()) + 1
    N, H, U, C, d, width = check_from_logs_args(tuple(topic.shape), d, categories, width, order, empty_row, layout)
    if order == 'given':
        if order_given is None:
            raise ValueError('order=\'given\' needs order_given')
        g = order_given.detach().cpu().numpy() if isinstance(order_given, torch.Tensor) else np.asarray(order_given)
        g = g.reshape(1, -1) if g.ndim == 1 else g
        if g.ndim != 2 or g.shape not in ((N, C), (1, C)):
            raise ValueError('order_given: expected [%d, %d], [1, %d] or [%d], got %s' % (N, C, C, C, g.shape))
    elif order_given is not None:
        raise ValueError('order_given is read with order=\'given\' only')
    dev = topic.device if is_tensor and topic.is_cuda and device is None else _device(device)
    per_day = H * U * 4 * (2 if layout == 'nuh' else 1)
    chunks = consistency_chunks(N, per_day, BUDGET if budget is None else budget)
    if order == 'total' and len(chunks) > 1:
        raise ValueError('order=\'total\' ranks over all %d days at once: %d bytes of log, the budget is %d'
                         % (N, N * per_day, BUDGET if budget is None else budget))
    parts = []
    for first, count in chunks:
        part = _to_device_i32(topic[first:first + count], dev)
        if layout == 'nuh':
            part = part.permute(0, 2, 1).contiguous()
        table = None
        if order == 'given':
            table = _to_device_i32(g if g.shape[0] == 1 else g[first:first + count], dev)
        res = ops.demos_from_logs(part, C, d, width=width, order=order, order_given=table, empty_row=empty_row)
        parts.append({name: res[name].cpu().numpy() for name in ARRAYS})
        del part, res
    return Demonstrations({name: np.concatenate([p[name] for p in parts]) for name in ARRAYS}, d, width, empty_row)


def from_moves(counts, moves, d=None, *, empty_row='uniform', device=None):
    """Demonstrations from integer tables: counts [N, H, width] and moves [N, H-1, width, width] (NumPy or tensors), e.g. the
    (counts, counts_next) and moves of ops.agents_step_pop with every member a day of H = 2 (from_agents_step).  A negative
    entry is a failed member: NaN rows and status bit _lib.DEMOS_FAILED."""
    import torch
    from . import ops
    N, H, d, width = ops.check_demos_moves_args(tuple(counts.shape), tuple(moves.shape), d, empty_row)
    dev = counts.device if isinstance(counts, torch.Tensor) and counts.is_cuda and device is None else _device(device)
    res = ops.demos_from_moves(_to_device_i32(counts, dev), _to_device_i32(moves, dev), d, empty_row=empty_row)
    arrays = {name: res[name].cpu().numpy() for name in res}
    arrays['order'] = None
    return Demonstrations(arrays, d, width, empty_row)


def from_agents_step(counts, counts_next, moves, *, empty_row='uniform'):
    """from_moves on one ops.agents_step_pop step: counts, counts_next [K, B, d] and moves [K, B, d, d] device tensors; member
    (k, b) becomes day k B + b with H = 2."""
    import torch
    K, B, d = counts.shape
    both = torch.stack([counts.reshape(K * B, d), counts_next.reshape(K * B, d)], dim=1).contiguous()
    return from_moves(both, moves.reshape(K * B, 1, d, d).contiguous(), d, empty_row=empty_row)


BOOT_ARRAYS = ('state', 'action', 'counts', 'moves', 'present', 'left', 'entered', 'status')


class BootstrapDemonstrations:
    """R Poisson-bootstrap replicates of the demonstrations of one log (bootstrap): `sample`, the Demonstrations of the log
    itself, and the arrays of mfg_demos_bootstrap as NumPy with a leading R -- state [R,N,H,d], action [R,N,H-1,d,d], counts,
    moves, present, left, entered, status [R,N].  Every replicate shares the sample's ranking (`sample.order`)."""

    def __init__(self, sample, arrays, seed=0, unit='agent_day'):
        self.sample, self.seed, self.unit = sample, int(seed), unit
        self.d, self.width, self.empty_row, self.N, self.H = sample.d, sample.width, sample.empty_row, sample.N, sample.H
        for name in BOOT_ARRAYS:
            setattr(self, name, np.asarray(arrays[name]))
        self.R = self.state.shape[0]
        if self.state.shape != (self.R, self.N, self.H, self.d) or self.status.shape != (self.R, self.N):
            raise ValueError('state %s / status %s: expected [R, %d, %d, %d] and [R, %d]'
                             % (self.state.shape, self.status.shape, self.N, self.H, self.d, self.N))

    def _r(self, r):
        if not 0 <= int(r) < self.R:
            raise ValueError('replicate %d outside [0, %d)' % (r, self.R))
        return int(r)

    def replicate(self, r):
        """Replicate r as a Demonstrations (order: the sample's), for every consumer of one."""
        r = self._r(r)
        arrays = {name: getattr(self, name)[r] for name in BOOT_ARRAYS}
        arrays['order'] = self.sample.order
        return Demonstrations(arrays, self.d, self.width, self.empty_row)

    def emp(self, days=None):
        """[R, days, H, d] fp64: every replicate's day table."""
        return self.state[:, self.sample._days(days)].astype(np.float64)

    def days_table(self):
        """[R N, H, d] fp64: the days of all replicates as one table, replicate r's day n at row r N + n (day_index), so that
        var.fit_population / rnn.fit_population fit K = R models in one call, model r on replicate r's days."""
        return self.state.reshape(self.R * self.N, self.H, self.d).astype(np.float64)

    def day_index(self, r, days=None):
        """The rows of days_table() that hold the given days of replicate r."""
        return np.asarray([self._r(r) * self.N + n for n in self.sample._days(days)], np.int64)

    def bands(self, ranks=(), device=None):
        """Per cell over the R replicates, on the device (ops.replicate_bands): a dict name -> (mean fp64, std fp64 with ddof 0,
        quant [Q, ...] fp32) for 'state' [N,H,d] and 'action' [N,H-1,d,d].  quant[q] is the replicate value of 0-based rank
        ranks[q]; a cell that is NaN in any replicate is NaN."""
        import torch
        from . import ops
        dev = _device(device)
        out = {}
        for name in ('state', 'action'):
            res = ops.replicate_bands(torch.as_tensor(np.ascontiguousarray(getattr(self, name)), device=dev), ranks)
            out[name] = tuple(t.cpu().numpy() for t in res)
        return out

    def interval_ranks(self, level=0.9):
        """The two 0-based ranks of the percentile interval of the given level: floor(a (R - 1)) and ceil((1 - a) (R - 1)),
        a = (1 - level) / 2."""
        if not 0.0 < level < 1.0:
            raise ValueError('level=%r outside (0, 1)' % (level,))
        a = (1.0 - level) / 2.0
        return int(np.floor(a * (self.R - 1))), int(np.ceil((1.0 - a) * (self.R - 1)))

    def interval(self, level=0.9, device=None):
        """The percentile interval over the replicates: a dict name -> (low, high) fp32 for 'state' and 'action'."""
        b = self.bands(self.interval_ranks(level), device)
        return {name: (q[0], q[1]) for name, (_, _, q) in b.items()}


def bootstrap_day_bytes(H, U, d, width, replicates, layout='nhu'):
    """Device bytes one day costs a chunk of bootstrap: the log (twice when it is transposed) and the R-fold integer tables,
    once as outputs and once in the workspace, and the R-fold fp32 outputs."""
    tables = H * width + (H - 1) * width * width
    return H * U * 4 * (2 if layout == 'nuh' else 1) + replicates * 4 * (2 * tables + H * d + (H - 1) * d * d + H + 2 * (H - 1) * width)


def bootstrap(topic, d, replicates, *, seed=0, unit='agent_day', categories=None, width=None, order='first_hour', order_given=None,
              empty_row='uniform', layout='nhu', device=None, budget=None):
    """The demonstrations of a log with `replicates` Poisson-bootstrap replicates of them: the recorded agents resampled on the
    device, every agent with its whole trajectory (ops.demos_bootstrap, C ABI mfg_demos_bootstrap).  topic, d, categories,
    width, order, order_given, empty_row, layout, device as from_logs: the log is counted once as it is (the sample and its
    ranking), then once with R weighted tallies under that ranking.  unit='agent_day': an agent index is another person each
    day; 'agent': agent u is one person, who carries one weight through all days.  The days go in chunks whose log and R-fold
    tables stay within `budget` bytes (None: BUDGET); chunking changes no bit; order='total' needs one chunk.  Returns a
    BootstrapDemonstrations."""
    import torch
    from . import ops
    from .population import consistency_chunks
    is_tensor = isinstance(topic, torch.Tensor)
    if not is_tensor:
        topic = np.asarray(topic)
    if categories is None:
        if (topic.numel() if is_tensor else topic.size) == 0:
            raise ValueError('topic is empty')
        categories = int(topic.max()) + 1
    N, H, U, C, d, width = check_from_logs_args(tuple(topic.shape), d, categories, width, order, empty_row, layout)
    R = int(replicates)
    ops.check_demos_boot_args((N, H, U), (1, C), C, d, R, width, unit, 0, empty_row)
    g = None
    if order == 'given':
        if order_given is None:
            raise ValueError('order=\'given\' needs order_given')
        g = order_given.detach().cpu().numpy() if isinstance(order_given, torch.Tensor) else np.asarray(order_given)
        g = g.reshape(1, -1) if g.ndim == 1 else g
        if g.ndim != 2 or g.shape not in ((N, C), (1, C)):
            raise ValueError('order_given: expected [%d, %d], [1, %d] or [%d], got %s' % (N, C, C, C, g.shape))
    elif order_given is not None:
        raise ValueError('order_given is read with order=\'given\' only')
    dev = topic.device if is_tensor and topic.is_cuda and device is None else _device(device)
    limit = BUDGET if budget is None else budget
    chunks = consistency_chunks(N, bootstrap_day_bytes(H, U, d, width, R, layout), limit)
    if order == 'total' and len(chunks) > 1:
        raise ValueError('order=\'total\' ranks over all %d days at once: %d bytes, the budget is %d'
                         % (N, N * bootstrap_day_bytes(H, U, d, width, R, layout), limit))
    parts, boots = [], []
    for first, count in chunks:
        part = _to_device_i32(topic[first:first + count], dev)
        if layout == 'nuh':
            part = part.permute(0, 2, 1).contiguous()
        table = None
        if order == 'given':
            table = _to_device_i32(g if g.shape[0] == 1 else g[first:first + count], dev)
        res = ops.demos_from_logs(part, C, d, width=width, order=order, order_given=table, empty_row=empty_row)
        if order == 'given':
            rank = table
        else:                                   # order [count, C]: rank -> category, every category ranked; inverted
            rank = torch.empty_like(res['order'])
            rank.scatter_(1, res['order'].long(), torch.arange(C, dtype=torch.int32, device=dev).expand(count, C).contiguous())
        boot = ops.demos_bootstrap(part, rank, C, d, R, seed, width=width, unit=unit, day_offset=first, empty_row=empty_row)
        parts.append({name: res[name].cpu().numpy() for name in ARRAYS})
        boots.append({name: boot[name].cpu().numpy() for name in BOOT_ARRAYS})
        del part, res, boot
    sample = Demonstrations({name: np.concatenate([p[name] for p in parts]) for name in ARRAYS}, d, width, empty_row)
    return BootstrapDemonstrations(sample, {name: np.concatenate([b[name] for b in boots], axis=1) for name in BOOT_ARRAYS}, seed, unit)
