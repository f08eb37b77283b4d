"""Stream order of the C ABI: the call table and the two procedures of tests/test_gpu_stream_order.py.

include/mfg_hip.h promises that every entry point enqueues ALL of its work on the `stream` it is given and neither allocates nor
synchronises.  ROWS has at least one row per function of the header that takes an mfg_stream_t (tests/test_stream_order_host.py
checks that on the CPU, against NEEDS_COMM and DRAINS).  A row is a builder: given a Bufs it declares the inputs with their data,
the in/out buffers with their start values, the outputs and the workspace (sized by the matching *_workspace_bytes query, zeroed)
and returns a closure that issues the C-ABI call(s) on torch's current stream.  A Bufs has a `salt`: 0 gives the true data,
1 a DECOY -- another valid input of the same shapes (simplex rows, in-range indices, finite parameters inside the mixed range),
so a launch that runs ahead of its producer computes a well-defined wrong answer and nothing else.

  reference()     the row on the default stream, everything synchronised: clones of every output and in/out buffer.
  run_delayed()   method A: decoy buffers; on a side stream a sleep kernel, device copies of the true data into the buffers, the
                  call, clones.  Whatever the call put on another stream runs tens of milliseconds early and meets the decoy (or
                  a workspace the previous launch of its chain has not filled yet).
  run_captured()  method B: the call captured into a graph on decoy buffers (a hidden synchronise, allocation or legacy-stream
                  launch is a capture error), nothing may have run at capture; true data written in place, two replays.
  independent_side_stream()  the side stream both run on: one on which a null-stream kernel was measured to complete while a
                  sleep is pending (streams share a few hardware queues; a shared queue would hide a launch on stream 0).
No row hands a call a buffer smaller than it needs, and no decoy is garbage: nothing here can fault.

The table also knows each workspace's CONTRACT, in the words of include/mfg_hip.h (tests/test_stale_workspace_host.py holds the
two against each other): Row.work lists, per work buffer in the order of the builder's ws() calls, (entry point, parameter, kind)
  CTL      a workspace from mfg_workspace_bytes: bytes [0, 64), the control block, are zero before and after every call
  SLICES   K such slices back to back (the population forms): [k slice, k slice + 64) of every slice
  SCRATCH  "contents are scratch": nothing is promised, nothing may be assumed
and ws(..., zero=) hands the byte ranges over.  Bufs(dev, salt) zeroes the whole buffer as before.  Bufs(dev, salt, fill=byte)
is the POISONED mode of tests/test_gpu_stale_workspace.py: every work buffer is a guard_bands.Guarded of exactly nbytes whose
bytes outside the declared ranges are `byte`.  Bufs(dev, salt, donor=earlier_bufs) is the DONOR mode: ws() returns the leading
nbytes of the buffer the earlier Bufs used for the same ws() call, contents untouched.  A declared range that was not a
declared range of the call before (a slice boundary that lay in a neighbour's rows) is the caller's to zero: the procedures do
that, and only that, with Bufs.zero_new_ranges before they issue the call.
"""
import contextlib
import ctypes as C
import time

import numpy as np
import torch

import guard_bands

NAN = float('nan')
THETA, SHIFT, SCALE, GAMMA = 8.86349, 0.16, 12000.0, 0.9
LR_C, LR_A = 0.1, 0.001
NUM_START = 40
F32, F64, I32, I64, U8 = torch.float32, torch.float64, torch.int32, torch.int64, torch.uint8

# Entry points with an mfg_stream_t that have no row, and why (nothing else may be listed):
NEEDS_COMM = ('mfg_dist_all_reduce', 'mfg_train_rollouts_dist')       # need an RCCL communicator: tests/test_gpu_rccl.py, _multiproc.py
# Entry points whose header comment says that the stream is drained once before the first launch (a host array is uploaded into
# device scratch): they have rows, run_delayed() skips the pending check for them and run_captured() is not run.
DRAINS = ('mfg_reward_net_forward_pop', 'mfg_reward_net_train_steps_pop', 'mfg_reward_net_train_steps_pop_z', 'mfg_traj_log_z_pop')

_FORCED = [None]          # a stream handle every call() uses instead of torch's current stream (the negative controls)


def _ops():
    from discrete_mean_field_game_amd import ops
    return ops


def _L():
    from discrete_mean_field_game_amd import _lib
    return _lib


@contextlib.contextmanager
def forced_stream(handle):
    """Hand every call() the stream `handle` whatever torch's current stream is: a caller that passes the wrong stream."""
    _FORCED[0] = handle
    try:
        yield
    finally:
        _FORCED[0] = None


def call(name, *args):
    """One C ABI call on torch's current stream."""
    L = _L()
    st = _FORCED[0] if _FORCED[0] is not None else torch.cuda.current_stream().cuda_stream
    L.check(getattr(L.lib(), name)(*args, st), name)


def same(a, b):
    """Bit for bit (NaN payloads and signed zeros included)."""
    if a.dtype.is_floating_point:
        it = I32 if a.element_size() == 4 else I64
        return torch.equal(a.contiguous().view(it), b.contiguous().view(it))
    return torch.equal(a, b)


def p(t):
    return None if t is None else t.data_ptr()


# ---- the workspace contracts of include/mfg_hip.h (Row.work kinds and the `zero` ranges of Bufs.ws)
CONTROL_BYTES = 64                        # MFG_WS_CONTROL_BYTES
CTL, SLICES, SCRATCH_KIND = 'control', 'slices', 'scratch'
CONTROL = ((0, CONTROL_BYTES),)
SCRATCH = ()


def slices(K, slice_bytes):
    """The control blocks of K slices back to back."""
    return tuple((k * slice_bytes, k * slice_bytes + CONTROL_BYTES) for k in range(K))


def kind_of(zero, nbytes):
    if not zero:
        return SCRATCH_KIND
    if tuple(zero) == CONTROL:
        return CTL
    assert nbytes % len(zero) == 0 and tuple(zero) == slices(len(zero), nbytes // len(zero)), zero
    return SLICES


class Bufs:
    """The buffers of one call.  salt = 0: the true data; 1: the decoy.  fill / donor: see the module's docstring."""

    def __init__(self, dev, salt, fill=None, donor=None):
        assert fill is None or donor is None
        self.dev, self.salt, self.fill, self.donor = dev, salt, fill, donor
        self.guarded = []     # poisoned / donor mode: the Guarded behind work[i]
        self.zero = []        # the declared zero ranges of work[i]: ((first byte, end byte), ...)
        self.inputs = {}      # inputs and in/out buffers (what a producer has to write before the call)
        self.written = []     # names of the in/out buffers: compared after the call
        self.outs = {}        # name -> (tensor, fill)
        self.host = []        # closures that overwrite a host array the call was handed by pointer with other valid values
        self.keep = []        # objects that must outlive the call (contexts, host structs)
        self.work = []        # the workspaces and scratch buffers: owned here, a row may hold nothing but their addresses

    def seed(self, s):
        return s + 100003 * self.salt

    def inp(self, name, data):
        assert name not in self.inputs and name not in self.outs, name
        self.inputs[name] = data.detach().clone().contiguous()
        return self.inputs[name]

    def io(self, name, data):
        self.written.append(name)
        return self.inp(name, data)

    def out(self, name, shape, dtype=F32, keep=None):
        assert name not in self.inputs and name not in self.outs, name
        fill = keep if keep is not None else (NAN if dtype.is_floating_point else -7)
        t = torch.full(tuple(shape), fill, dtype=dtype, device=self.dev)
        self.outs[name] = (t, fill)
        return t

    def ws(self, nbytes, dtype=U8, shape=None, zero=SCRATCH):
        """A workspace of exactly the advertised bytes; its contents are not compared.  zero: the byte ranges the header
        requires to be zero (CTL, slices(K, slice_bytes), SCRATCH).  Plain mode: all of it zeroed.  Poisoned mode: a Guarded,
        `fill` everywhere outside `zero`.  Donor mode: the head of the donor's buffer, untouched."""
        item = torch.empty(0, dtype=dtype).element_size()
        assert nbytes % item == 0
        assert all(0 <= lo < hi <= nbytes for lo, hi in zero), (zero, nbytes)
        if self.fill is None and self.donor is None:
            t = torch.zeros(nbytes // item, dtype=dtype, device=self.dev)
        else:
            if self.donor is not None:
                i = len(self.work)
                g = self.donor.guarded[i]
                assert g.nbytes >= nbytes, 'the donor\'s buffer %d holds %d bytes, the call needs %d' % (i, g.nbytes, nbytes)
                raw = g.raw[g.start:g.start + nbytes]
            else:
                g = guard_bands.Guarded(nbytes, U8, self.dev, fill=self.fill)
                raw = g.t
                for lo, hi in zero:
                    raw[lo:hi] = 0
            self.guarded.append(g)
            t = raw.view(dtype)
        self.work.append(t)
        self.zero.append(tuple(zero))
        return t if shape is None else t.view(shape)

    def zero_new_ranges(self, before):
        """The caller's side of reusing a buffer: zero every declared range of work[i] that was not a declared range
        (before[i]) of the call that used the buffer last -- a slice's control block that lay in a neighbour's old rows.
        Nothing else of a reused buffer is ever touched."""
        for t, zero, old in zip(self.work, self.zero, before):
            raw = t.view(-1).view(U8)
            for lo, hi in zero:
                if (lo, hi) not in old:
                    raw[lo:hi] = 0

    def stale_ranges(self):
        """Names of the declared zero ranges that are not all zero (after a call: assertion (b) of the stale-workspace tests)."""
        bad = []
        for i, (t, zero) in enumerate(zip(self.work, self.zero)):
            raw = t.view(-1).view(U8)
            bad += ['work[%d] bytes [%d, %d)' % (i, lo, hi) for lo, hi in zero if bool(raw[lo:hi].any())]
        return bad

    def check_bands(self):
        for i, g in enumerate(self.guarded):
            g.check('work[%d]' % i)

    # ---- valid data by seed
    def simplex(self, shape, seed):
        g = torch.Generator(device=self.dev)
        g.manual_seed(self.seed(seed))
        x = torch.rand(shape, device=self.dev, generator=g) + 1e-3
        return (x / x.sum(-1, keepdim=True)).contiguous()

    def randn64(self, shape, seed):
        g = torch.Generator(device=self.dev)
        g.manual_seed(self.seed(seed))
        return torch.randn(shape, device=self.dev, generator=g, dtype=F64)

    def rand32(self, shape, seed):
        g = torch.Generator(device=self.dev)
        g.manual_seed(self.seed(seed))
        return torch.rand(shape, device=self.dev, generator=g)

    def index(self, n, high, seed):
        g = torch.Generator(device=self.dev)
        g.manual_seed(self.seed(seed))
        return torch.randint(high, (n,), device=self.dev, generator=g, dtype=I32)

    def f64(self, *values):
        """An fp64 vector; the decoy is 0.85 x the values (theta, shifts, rates: still inside every range)."""
        return torch.tensor(values, dtype=F64, device=self.dev) * (0.85 if self.salt else 1.0)

    def theta(self):
        return self.io_or_inp('theta', self.f64(THETA), False)

    def io_or_inp(self, name, data, written):
        return self.io(name, data) if written else self.inp(name, data)

    def w(self, d, written=False, lead=()):
        F = _ops().num_features(d)
        return self.io_or_inp('w', self.randn64(lead + (F,), d).abs_() * (0.1 if lead else 1.0), written)

    def policies(self, K):
        """thetas, shifts, alpha_scales (fp64 [K]) and seeds (int64 [K]) of K policies; two of them share a seed."""
        seeds = torch.arange(K, dtype=I64, device=self.dev) * 7919 + (1 << 33) + 31 * self.salt
        if K > 1:
            seeds[1] = seeds[0]
        return (self.inp('thetas', self.f64(*np.linspace(6.5, 9.5, K))), self.inp('shifts', self.f64(*np.linspace(0.1, 0.3, K))),
                self.inp('alpha_scales', self.f64(*np.linspace(9000.0, 13000.0, K))), self.inp('seeds', seeds))

    def compared(self):
        """name -> tensor of everything the call writes that is compared: the outputs and the in/out buffers."""
        d = {n: t for n, (t, _) in self.outs.items()}
        d.update({n: self.inputs[n] for n in self.written})
        return d

    def refill(self):
        for t, fill in self.outs.values():
            t.fill_(fill)

    def scribble(self):
        for fn in self.host:
            fn()


class Row:
    def __init__(self, name, entries, build, work=()):
        self.name, self.entries, self.build = name, tuple(entries), build
        self.work = tuple(work)          # (entry point, parameter, kind) per work buffer, in the order of the builder's ws() calls
        assert all(e in self.entries and k in (CTL, SLICES, SCRATCH_KIND) for e, _, k in self.work), name
        self.drains = any(e in DRAINS for e in self.entries)

    def __repr__(self):
        return self.name


ROWS = []
_SINK = [ROWS]


def row(name, *entries, work=()):
    def deco(build):
        _SINK[0].append(Row(name, entries, build, work))
        return build
    return deco


@contextlib.contextmanager
def extra_rows():
    """Rows made by the factories below inside this block go to the list it yields, not into ROWS: other shapes of a family."""
    out = []
    _SINK[0] = out
    try:
        yield out
    finally:
        _SINK[0] = ROWS


def _w(entry, *kinds):
    """Row.work of an entry point whose work buffers are all called `workspace` but for a leading pi_scratch (SCRATCH_KIND first)."""
    return tuple((entry, 'pi_scratch' if k == SCRATCH_KIND and len(kinds) > 1 and i == 0 else 'workspace', k)
                 for i, k in enumerate(kinds))


def wsb(N, d):
    return int(_L().lib().mfg_workspace_bytes(N, d))


# ---------------------------------------------------------------------------------------------------
# mfg_step_given_P, mfg_sample_dirichlet
# ---------------------------------------------------------------------------------------------------
def _step_given_P(d, B):
    @row('step_given_P-d%d-B%d' % (d, B), 'mfg_step_given_P')
    def build(a):
        pi, P = a.inp('pi', a.simplex((B, d), 1)), a.inp('P', a.simplex((B, d, d), 2))
        pn, r = a.out('pi_next', (B, d)), a.out('reward', (B,))
        return lambda: call('mfg_step_given_P', p(pi), p(P), B, d, 0, p(pn), p(r))


_step_given_P(21, 13)
_step_given_P(128, 6)


def _sample_dirichlet(d, B, precision):
    @row('sample_dirichlet-d%d-B%d-%s' % (d, B, precision), 'mfg_sample_dirichlet')
    def build(a):
        pi, th, P = a.inp('pi', a.simplex((B, d), 3)), a.theta(), a.out('P', (B, d, d))
        return lambda: call('mfg_sample_dirichlet', p(pi), B, d, p(th), SHIFT, SCALE, 99, 5, 1000, _L().PRECISIONS[precision], p(P))


_sample_dirichlet(21, 13, 'mixed')
_sample_dirichlet(21, 13, 'f64')
_sample_dirichlet(130, 3, 'mixed')


# ---------------------------------------------------------------------------------------------------
# mfg_rollout
# ---------------------------------------------------------------------------------------------------
def _rollout_outs(a, B, d, T, lead=()):
    return (a.out('pi_traj', lead + (B, T + 1, d)), a.out('pi_last', lead + (B, d)), a.out('reward', lead + (B, T)),
            a.out('delta', lead + (B, T), F64), a.out('g', lead + (B, T), F64))


def _rollout_td(d, B, T):
    @row('rollout-td-G-d%d-B%d-T%d' % (d, B, T), 'mfg_rollout', work=_w('mfg_rollout', CTL))
    def build(a):
        L = _L()
        F = _ops().num_features(d)
        pi0, th, w = a.inp('pi0', a.simplex((B, d), 4)), a.theta(), a.w(d)
        traj, last, r, delta, g = _rollout_outs(a, B, d, T)
        G, n = a.out('G', (F + 3,), F64), wsb(B * T, d)
        ws = a.ws(n, zero=CONTROL)
        return lambda: call('mfg_rollout', p(pi0), B, d, T, p(th), SHIFT, SCALE, p(w), GAMMA, L.REWARD_MFG_AC2, 99, 5, 1000,
                            L.ROLLOUT_TD, p(traj), p(last), p(r), p(delta), p(g), None, p(G), 0, p(ws), n)


_rollout_td(21, 13, 3)      # core, batch sums, row reduction
_rollout_td(128, 6, 2)      # k_core_large, k_value_mfma2, k_td_delta, k_grad_mfma2, k_reduce_partials
_rollout_td(100, 5, 2)      # the generic forms


@row('rollout-external+grad_accumulate-d21', 'mfg_rollout', 'mfg_grad_accumulate', work=_w('mfg_grad_accumulate', CTL))
def _rollout_external(a):
    """The IRL step by hand: rollout without a reward, then the batch sums with the reward added to delta."""
    L = _L()
    d, B, T = 21, 13, 3
    F = _ops().num_features(d)
    pi0, th, w = a.inp('pi0', a.simplex((B, d), 5)), a.theta(), a.w(d)
    reward = a.inp('reward', a.randn64((B, T), 6).float())
    traj, last = a.out('pi_traj', (B, T + 1, d)), a.out('pi_last', (B, d))
    delta, g, G = a.out('delta', (B, T), F64), a.out('g', (B, T), F64), a.out('G', (F + 3,), F64)
    n = wsb(B * T, d)
    ws = a.ws(n, zero=CONTROL)

    def issue():
        call('mfg_rollout', p(pi0), B, d, T, p(th), SHIFT, SCALE, p(w), GAMMA, L.REWARD_EXTERNAL, 99, 5, 1000, L.ROLLOUT_TD,
             p(traj), p(last), None, p(delta), p(g), None, None, 0, None, 0)
        call('mfg_grad_accumulate', p(traj), (T + 1) * d, p(delta), p(g), p(reward), B, T, d, 1, p(G), 0, p(ws), n)
    return issue


# ---------------------------------------------------------------------------------------------------
# batch sums and the update
# ---------------------------------------------------------------------------------------------------
def _sum_N(d):
    return 65 if d == 21 else 37          # d = 21: one chunk of 64 samples + 1


def _nm(N):
    return '' if N is None else '-N%d' % N


def _td_pg_accumulate(d, accumulate, N=None):
    @row('td_pg_accumulate-d%d-acc%d%s' % (d, accumulate, _nm(N)), 'mfg_td_pg_accumulate', work=_w('mfg_td_pg_accumulate', CTL))
    def build(a, N=N):
        N = N or _sum_N(d)
        F = _ops().num_features(d)
        pi, pin, P = a.inp('pi', a.simplex((N, d), 7)), a.inp('pi_next', a.simplex((N, d), 8)), a.inp('P', a.simplex((N, d, d), 9))
        reward, w, th = a.inp('reward', a.randn64((N,), 10).float()), a.w(d), a.theta()
        delta, g = a.out('delta', (N,), F64), a.out('g', (N,), F64)
        G = a.io('G', a.randn64((F + 3,), 11)) if accumulate else a.out('G', (F + 3,), F64)
        n = wsb(N, d)
        ws = a.ws(n, zero=CONTROL)
        return lambda: call('mfg_td_pg_accumulate', p(pi), p(pin), p(P), p(reward), p(w), p(th), SHIFT, GAMMA, N, d,
                            _L().PRECISION_MIXED, p(delta), p(g), p(G), accumulate, p(ws), n)


def _grad_accumulate(d, accumulate, N=None):
    @row('grad_accumulate-d%d-acc%d%s' % (d, accumulate, _nm(N)), 'mfg_grad_accumulate', work=_w('mfg_grad_accumulate', CTL))
    def build(a, N=N):
        """accumulate = 1 also runs add_reward = 1: delta is then updated in place."""
        N = N or _sum_N(d)
        F = _ops().num_features(d)
        pi, g, reward = a.inp('pi', a.simplex((N, d), 12)), a.inp('g', a.randn64((N,), 13)), a.inp('reward', a.randn64((N,), 14).float())
        delta = a.io_or_inp('delta', a.randn64((N,), 15), bool(accumulate))
        G = a.io('G', a.randn64((F + 3,), 16)) if accumulate else a.out('G', (F + 3,), F64)
        n = wsb(N, d)
        ws = a.ws(n, zero=CONTROL)
        return lambda: call('mfg_grad_accumulate', p(pi), d, p(delta), p(g), p(reward), N, 1, d, accumulate, p(G), accumulate,
                            p(ws), n)


def _grad_apply(d, add_reward, N=None):
    @row('grad_apply-d%d-add_reward%d%s' % (d, add_reward, _nm(N)), 'mfg_grad_apply', work=_w('mfg_grad_apply', CTL))
    def build(a, N=N):
        """mfg_grad_apply has no `accumulate`: its two forms are add_reward = 0 / 1 (delta then updated in place)."""
        N = N or _sum_N(d)
        F = _ops().num_features(d)
        pi, g, reward = a.inp('pi', a.simplex((N, d), 17)), a.inp('g', a.randn64((N,), 18)), a.inp('reward', a.randn64((N,), 19).float())
        delta = a.io_or_inp('delta', a.randn64((N,), 20), bool(add_reward))
        w, th, acc = a.w(d, True), a.io('theta', a.f64(THETA)), a.io('reward_acc', a.f64(-3.25))
        G, n = a.out('G', (F + 3,), F64), wsb(N, d)
        ws = a.ws(n, zero=CONTROL)
        return lambda: call('mfg_grad_apply', p(pi), d, p(delta), p(g), p(reward), N, 1, d, add_reward, p(G), LR_C, LR_A, p(w),
                            p(th), p(acc), p(ws), n)


for _d in (21, 128):
    for _f in (0, 1):
        _td_pg_accumulate(_d, _f)
        _grad_accumulate(_d, _f)
        _grad_apply(_d, _f)


def _pending_G(a, d, seed):
    F = _ops().num_features(d)
    G = a.randn64((F + 3,), seed)
    G[F + 2] = 7.0 + a.salt                # the count the sums are divided by
    return G


@row('apply_update-d21', 'mfg_apply_update')
def _apply_update(a):
    d = 21
    G, w, th, acc = a.inp('G', _pending_G(a, d, 21)), a.w(d, True), a.io('theta', a.f64(THETA)), a.io('reward_acc', a.f64(-3.25))
    return lambda: call('mfg_apply_update', p(G), d, LR_C, LR_A, p(w), p(th), p(acc))


# ---------------------------------------------------------------------------------------------------
# mfg_train_rollout (MFG_TRAIN_APPLY), mfg_train_rollout_deferred, mfg_train_rollouts
# ---------------------------------------------------------------------------------------------------
def _train_rollout(with_idx):
    @row('train_rollout-apply-%s' % ('idx' if with_idx else 'drawn'), 'mfg_train_rollout', work=_w('mfg_train_rollout', CTL))
    def build(a):
        L = _L()
        d, B, T = 21, 13, 3
        F = _ops().num_features(d)
        mat = a.inp('mat_pi0', a.simplex((NUM_START, d), 22))
        idx = a.inp('idx', a.index(B, NUM_START, 23)) if with_idx else None
        th, w, acc = a.io('theta', a.f64(THETA)), a.w(d, True), a.io('reward_acc', a.f64(-3.25))
        traj, last, r, delta, g = _rollout_outs(a, B, d, T)
        G, n = a.out('G', (F + 3,), F64), wsb(B * T, d)
        ws = a.ws(n, zero=CONTROL)
        return lambda: call('mfg_train_rollout', p(mat), NUM_START, p(idx), B, d, T, p(th), SHIFT, SCALE, p(w), GAMMA,
                            L.REWARD_MFG_AC2, 7, 3, 100, L.TRAIN_APPLY, LR_C, LR_A, p(traj), p(last), p(r), p(delta), p(g), p(G),
                            p(acc), p(ws), n)


_train_rollout(True)
_train_rollout(False)


_DEFERRED = {21: (13, 3), 128: (5, 2)}      # the table's shapes per d: their rows keep the names without a shape suffix


def _train_rollout_deferred(d, B, T):
    @row('train_rollout_deferred-x2-d%d%s' % (d, '' if (B, T) == _DEFERRED[d] else '-B%d-T%d' % (B, T)),
         'mfg_train_rollout_deferred', work=_w('mfg_train_rollout_deferred', CTL))
    def build(a):
        """Two chained calls that ping-pong the parameter sets: (theta, w) -> (theta_alt, w_alt) -> (theta, w), the second
        applying the sums the first left in G (d > 64: the out-of-place update launch and its device-to-device copies)."""
        L = _L()
        F = _ops().num_features(d)
        mat = a.inp('mat_pi0', a.simplex((NUM_START, d), 24))
        th, w, acc = a.io('theta', a.f64(THETA)), a.w(d, True), a.io('reward_acc', a.f64(-3.25))
        Gp = a.inp('G_pending', _pending_G(a, d, 25))
        th2, w2 = a.out('theta_alt', (1,), F64), a.out('w_alt', (F,), F64)
        traj, last, r, delta, g = _rollout_outs(a, B, d, T)
        G, n = a.out('G', (F + 3,), F64), wsb(B * T, d)
        ws = a.ws(n, zero=CONTROL)

        def one(t_in, w_in, pend, t_out, w_out, step):
            call('mfg_train_rollout_deferred', p(mat), NUM_START, None, B, d, T, p(t_in), p(w_in), p(pend), LR_C, LR_A, p(acc),
                 p(t_out), p(w_out), SHIFT, SCALE, GAMMA, L.REWARD_MFG_AC2, 7, step, 100, 0, p(traj), p(last), p(r), p(delta),
                 p(g), p(G), p(ws), n)

        def issue():
            one(th, w, Gp, th2, w2, 3)
            one(th2, w2, G, th, w, 3 + T)
        return issue


_train_rollout_deferred(21, 13, 3)
_train_rollout_deferred(128, 5, 2)


def _episode_bufs(a, B, d, lead=()):
    """pi_scratch is scratch by contract (no range of it is declared zero): not compared."""
    return (a.ws(int(np.prod(lead + (B, d))) * 4, F32, lead + (B, d)), a.out('reward', lead + (B,)), a.out('delta', lead + (B,), F64),
            a.out('g', lead + (B,), F64))


_EPISODE = {21: (13, 3), 47: (9, 2)}         # the table's shapes per d, as _DEFERRED


def _train_episode(d, B, T):
    @row('train_episode-d%d-T%d%s' % (d, T, '' if (B, T) == _EPISODE.get(d) else '-B%d' % B), 'mfg_train_episode',
         work=_w('mfg_train_episode', SCRATCH_KIND, CTL))
    def build(a):
        L = _L()
        F = _ops().num_features(d)
        pi = a.io('pi_io', a.simplex((B, d), 26))
        th, w, acc = a.io('theta', a.f64(THETA)), a.w(d, True), a.io('reward_acc', a.f64(-3.25))
        scratch, r, delta, g = _episode_bufs(a, B, d)
        G, n = a.out('G', (F + 3,), F64), wsb(B, d)
        ws = a.ws(n, zero=CONTROL)
        return lambda: call('mfg_train_episode', p(pi), p(scratch), B, d, T, p(th), SHIFT, SCALE, p(w), GAMMA, L.REWARD_MFG_AC2,
                            7, 3, 100, L.PRECISION_MIXED, LR_C, LR_A, p(r), p(delta), p(g), p(G), p(acc), p(ws), n)


_train_episode(21, 13, 3)       # the SUMS path and the row reduction; T odd: the copy-back of pi_io
_train_episode(47, 9, 2)        # the two-kernel path

EPISODES = 3


def _bt(B, T, B0=13, T0=3):
    return '' if (B, T) == (B0, T0) else '-B%d-T%d' % (B, T)


def _train_episodes(B=13, T=3):
    @row('train_episodes-x3' + _bt(B, T), 'mfg_train_episodes', work=_w('mfg_train_episodes', SCRATCH_KIND, CTL))
    def build(a):
        L = _L()
        d = 21
        F = _ops().num_features(d)
        mat, pi = a.inp('mat_pi0', a.simplex((NUM_START, d), 27)), a.out('pi_io', (B, d))
        th, w, acc = a.io('theta', a.f64(THETA)), a.w(d, True), a.io('reward_acc', a.f64(0.0, 0.0, 0.0) + a.salt)
        scratch, r, delta, g = _episode_bufs(a, B, d)
        G, n = a.out('G', (F + 3,), F64), wsb(B, d)
        ws = a.ws(n, zero=CONTROL)
        return lambda: call('mfg_train_episodes', p(mat), NUM_START, p(pi), p(scratch), B, d, T, EPISODES, 0, 0, p(th), SHIFT,
                            SCALE, p(w), GAMMA, L.REWARD_MFG_AC2, 7, 3, 100, L.PRECISION_MIXED, LR_C, LR_A, p(r), p(delta), p(g),
                            p(G), p(acc), p(ws), n)


_train_episodes()


def _train_rollouts(B=13, T=3):
    @row('train_rollouts-x3' + _bt(B, T), 'mfg_train_rollouts', work=_w('mfg_train_rollouts', CTL))
    def build(a):
        L = _L()
        d = 21
        F = _ops().num_features(d)
        mat = a.inp('mat_pi0', a.simplex((NUM_START, d), 28))
        th, w, acc = a.io('theta', a.f64(THETA)), a.w(d, True), a.io('reward_acc', a.f64(0.0, 0.0, 0.0) + a.salt)
        traj, last, r, delta, g = _rollout_outs(a, B, d, T)
        G, n = a.out('G', (F + 3,), F64), wsb(B * T, d)
        ws = a.ws(n, zero=CONTROL)
        return lambda: call('mfg_train_rollouts', p(mat), NUM_START, B, d, T, EPISODES, 0, 0, p(th), SHIFT, SCALE, p(w), GAMMA,
                            L.REWARD_MFG_AC2, 7, 3, 100, 0, LR_C, LR_A, p(traj), p(last), p(r), p(delta), p(g), p(G), p(acc), p(ws),
                            n)


_train_rollouts()


# ---------------------------------------------------------------------------------------------------
# populations, K = 3
# ---------------------------------------------------------------------------------------------------
POP = dict(K=3, B=13, T=2, E=2, d=21)


def _pop_name(shape):
    return '' if shape is POP else '-B%d-T%d' % (shape['B'], shape['T'])


def _pop_common(a, seed, shape=POP, scratch=False):
    K, B, T, E, d = (shape[k] for k in 'KBTEd')
    F = _ops().num_features(d)
    sb = _ops().pop_workspace_slice(B, d, T)
    mat = a.inp('mat_pi0', a.simplex((NUM_START, d), seed))
    sh, al, sd = a.policies(K)[1:]
    a.written.append('thetas')                                     # (theta [K] is updated in place)
    th = a.inputs['thetas']
    w, G = a.w(d, True, (K,)), a.out('G', (K, F + 3), F64)
    acc = a.io('reward_acc', torch.zeros(K, E, dtype=F64, device=a.dev) + a.salt)
    lrc, lra = a.inp('lr_critic', a.f64(*np.linspace(0.05, 0.15, K))), a.inp('lr_actor', a.f64(*np.linspace(5e-4, 2e-3, K)))
    ws = a.ws(K * sb, F64, (K, sb // 8), zero=SCRATCH if scratch else slices(K, sb))
    return mat, th, sh, al, sd, w, G, acc, lrc, lra, ws, sb


def _pop_step(entry, control=False, shape=POP):
    # (the resident form's header comment calls its workspace scratch: nothing of it is declared)
    kind = SCRATCH_KIND if entry.endswith('_resident') else SLICES

    @row(entry[4:] + ('-control' if control else '') + _pop_name(shape), entry, work=((entry, 'workspace', kind), (entry, 'pi_scratch', SCRATCH_KIND)))
    def build(a):
        L = _L()
        K, B, T, E, d = (shape[k] for k in 'KBTEd')
        mat, th, sh, al, sd, w, G, acc, lrc, lra, ws, sb = _pop_common(a, 29, shape, kind == SCRATCH_KIND)
        pi = a.out('pi_io', (K, B, d))
        scratch, r, delta, g = _episode_bufs(a, B, d, (K,))
        args = (p(mat), NUM_START, p(pi), p(scratch), B, K, d, T, E, 0, 0, p(th), p(sh), p(al), p(w), GAMMA, L.REWARD_MFG_AC2, p(sd),
                3, 100, L.PRECISION_MIXED, p(lrc), p(lra), p(r), p(delta), p(g), p(G), p(acc), p(ws), sb)
        if not control:
            return lambda: call(entry, *args)
        # a control block bound through a Context: k_pop_retire before the first episode and after every episode's update.
        # Learner 1 of the decoy is stopped already (a valid state): a retire kernel that ran early would leave it out.
        state = a.io('ctl_state', torch.tensor([0, a.salt, 0], dtype=I32, device=a.dev))
        status = a.io('ctl_status', torch.zeros(K, dtype=I32, device=a.dev))
        run = a.io('ctl_episodes_run', torch.zeros(K, dtype=I32, device=a.dev) + 5 * a.salt)
        prev = a.out('ctl_theta_prev', (K,), F64)
        stop = a.inp('ctl_stop_criteria', a.f64(-1.0, 1e3, -1.0))     # learner 1 stops after its first episode
        ctx = _ops().Context(a.dev)
        a.keep.append(ctx)

        def issue():
            before = ctx.bind_scoped()
            try:
                ctx.set_pop_control(state, status, prev, run, stop)
                call(entry, *args)
            finally:
                ctx.set_pop_control()
                ctx.restore(before)
        return issue


_pop_step('mfg_train_episodes_pop')
_pop_step('mfg_train_episodes_pop', control=True)
_pop_step('mfg_train_episodes_pop_resident')


def _pop_rollouts(shape=POP):
    @row('train_rollouts_pop' + _pop_name(shape), 'mfg_train_rollouts_pop', work=_w('mfg_train_rollouts_pop', SLICES))
    def build(a):
        L = _L()
        K, B, T, E, d = (shape[k] for k in 'KBTEd')
        mat, th, sh, al, sd, w, G, acc, lrc, lra, ws, sb = _pop_common(a, 30, shape)
        traj, last, r, delta, g = _rollout_outs(a, B, d, T, (K,))
        return lambda: call('mfg_train_rollouts_pop', p(mat), NUM_START, B, K, d, T, E, 0, 0, p(th), p(sh), p(al), p(w), GAMMA,
                            L.REWARD_MFG_AC2, p(sd), 3, 100, 0, p(lrc), p(lra), p(traj), p(last), p(r), p(delta), p(g), p(G), p(acc),
                            p(ws), sb)


_pop_rollouts()

VAL = dict(N=2, L=4, R=3)        # a held-out check: N files of L rows, R rollouts per file


def _pop_validated(shape=POP, VN=VAL['N']):
    """mfg_train_episodes_pop under a validation block (with the scores) and an evolve block: E = 2 episodes, period 1, so TWO
    checks run in one call, each followed by an exploit / explore step.  The blocks' work buffers reach the library through
    the structs of mfg_ctx_set_pop_validate / mfg_ctx_set_pop_evolve, not through a parameter: the validation workspace and
    the evolve block's order / active arrays, all three scratch in the header's words."""
    entry = 'mfg_train_episodes_pop'

    @row('train_episodes_pop-validate-evolve' + _pop_name(shape) + ('' if VN == VAL['N'] else '-VN%d' % VN), entry,
         work=((entry, 'workspace', SLICES), (entry, 'pi_scratch', SCRATCH_KIND), (entry, 'validate.workspace', SCRATCH_KIND),
               (entry, 'evolve.order', SCRATCH_KIND), (entry, 'evolve.active', SCRATCH_KIND)))
    def build(a):
        L, ops = _L(), _ops()
        K, B, T, E, d = (shape[k] for k in 'KBTEd')
        F = ops.num_features(d)
        mat, th, sh, al, sd, w, G, acc, lrc, lra, ws, sb = _pop_common(a, 78, shape)
        a.written += ['lr_critic', 'lr_actor']                      # (an evolve step rewrites the rates between two episodes)
        pi = a.out('pi_io', (K, B, d))
        scratch, r, delta, g = _episode_bufs(a, B, d, (K,))
        emp = a.simplex((VN, VAL['L'], d), 79)
        emp32, emp64 = a.inp('emp32', emp), a.inp('emp64', emp.double())
        i32 = lambda v: torch.full((K,), v, dtype=I32, device=a.dev)
        val = dict(curve=a.out('val_curve', (K, E, 10), F64), checks=a.io('val_checks', i32(0)),
                   best_value=a.io('val_best_value', torch.full((K,), float('inf'), dtype=F64, device=a.dev)),
                   best_check=a.io('val_best_check', i32(-1)), since_best=a.io('val_since_best', i32(0)),
                   best_theta=a.out('val_best_theta', (K,), F64), best_w=a.out('val_best_w', (K, F), F64))
        nv = ops.pop_validate_workspace_bytes(VN, VAL['L'], d, K, VAL['R'], True)
        vws = a.ws(nv)
        evo = dict(order=a.ws(4 * K, I32), active=a.ws(4, I32), rank=a.out('evo_rank', (K, E), I32, keep=-1),
                   parent=a.out('evo_parent', (K, E), I32, keep=-1), lr_log=a.out('evo_lr_log', (K, E, 2), F64))
        ctx = ops.Context(a.dev)
        a.keep.append(ctx)
        args = (p(mat), NUM_START, p(pi), p(scratch), B, K, d, T, E, 0, 0, p(th), p(sh), p(al), p(w), GAMMA, L.REWARD_MFG_AC2, p(sd),
                3, 100, L.PRECISION_MIXED, p(lrc), p(lra), p(r), p(delta), p(g), p(G), p(acc), p(ws), sb)

        def issue():
            before = ctx.bind_scoped()
            try:
                ctx.set_pop_validate(emp32, emp64, period=1, column=8, with_score=True, first_step=7, repeats=VAL['R'],
                                     workspace=vws, workspace_bytes=nv, **val)
                ctx.set_pop_evolve(lrc, lra, n_top=1, n_bottom=1, seed=0x5EED, **evo)
                call(entry, *args)
            finally:
                ctx.set_pop_evolve()
                ctx.set_pop_validate()
                ctx.restore(before)
        return issue


_pop_validated()


# ---------------------------------------------------------------------------------------------------
# the reward network and the IRL drivers
# ---------------------------------------------------------------------------------------------------
def _net(a, d, n3, n4, keep=0.8, K=None):
    """mfg_reward_net_t over parameter tensors registered as inputs (K: stacked, learner-major); the decoy is another network."""
    from oracle.reward_train_cases import _net as make
    L = _L()
    nets = [make(d, 'dropout_l1l2', n3, n4, a.dev, seed=a.seed(7 + k)) for k in range(K or 1)]
    st = L.RewardNetStruct()
    st.k1, st.f2, st.k2, st.n3, st.n4, st.keep_prob = 5, 2, 3, n3, n4, keep
    for name, get in (('conv1_w', lambda n: n.conv1.weight), ('conv1_b', lambda n: n.conv1.bias), ('conv2_w', lambda n: n.conv2.weight),
                      ('conv2_b', lambda n: n.conv2.bias), ('fc3_w', lambda n: n.fc3.weight), ('fc3_b', lambda n: n.fc3.bias),
                      ('fc4_w', lambda n: n.fc4.weight), ('fc4_b', lambda n: n.fc4.bias), ('out_w', lambda n: n.out.weight),
                      ('out_b', lambda n: n.out.bias)):
        t = torch.stack([get(n).detach().reshape(-1) for n in nets]) if K else get(nets[0]).detach().reshape(-1)
        setattr(st, name, a.inp('net_' + name, t).data_ptr())
    a.keep.append(st)
    return st


def _reward_net_forward(n3, kernel):
    @row('reward_net_forward-%s' % kernel, 'mfg_reward_net_forward')
    def build(a):
        d, B, n4 = 21, 37, 4
        st = _net(a, d, n3, n4)
        s, act, r = a.inp('state', a.simplex((B, d), 31)), a.inp('action', a.simplex((B, d, d), 32)), a.out('reward', (B,))
        return lambda: call('mfg_reward_net_forward', p(s), p(act), B, d, 5, 2, 3, n3, n4, st.conv1_w, st.conv1_b, st.conv2_w,
                            st.conv2_b, st.fc3_w, st.fc3_b, st.fc4_w, st.fc4_b, st.out_w, st.out_b, 0.8, 1234, 77, p(r))


_reward_net_forward(8, 'mfma')       # n_fc3 <= 16: the matrix-core kernel
_reward_net_forward(24, 'runs')      # n_fc3 > 16: the run-mapped kernel

IRL = dict(d=21, B=13, T=2, n3=8, n4=4)


def _irl_episode(draw, B=IRL['B'], T=IRL['T'], n3=IRL['n3']):
    """n3 <= 16: the two-launch env step (k_reward_net_mfma<.., SUMS>); above: three launches, the run-mapped network kernel."""
    entry = 'mfg_train_episode_irl' + ('_draw' if draw else '')

    @row(entry[4:] + _bt(B, T, IRL['B'], IRL['T']) + ('' if n3 == IRL['n3'] else '-n3_%d' % n3), entry,
         work=_w(entry, SCRATCH_KIND, CTL))
    def build(a):
        L = _L()
        d = IRL['d']
        F = _ops().num_features(d)
        st = _net(a, d, n3, IRL['n4'])
        if draw:
            mat, pi = a.inp('mat_pi0', a.simplex((NUM_START, d), 33)), a.out('pi_out', (B, d))
        else:
            pi = a.io('pi_io', a.simplex((B, d), 33))
        th, w, acc = a.io('theta', a.f64(THETA)), a.w(d, True), a.io('reward_acc', a.f64(-3.25))
        scratch, r, delta, g = _episode_bufs(a, B, d)
        P, G, n = a.out('P', (B, d, d)), a.out('G', (F + 3,), F64), wsb(B, d)
        ws = a.ws(n, zero=CONTROL)
        rest = (p(pi), p(scratch), B, d, T, p(th), SHIFT, SCALE, p(w), GAMMA, 7, 3, 100, L.PRECISION_MIXED, LR_C, LR_A, C.byref(st),
                0x5EED, 4, 100, p(P), p(r), p(delta), p(g), p(G), p(acc), p(ws), n)
        if draw:
            return lambda: call('mfg_train_episode_irl_draw', p(mat), NUM_START, *rest)
        return lambda: call('mfg_train_episode_irl', *rest)


_irl_episode(False)
_irl_episode(True)


def _irl_rollout(B=IRL['B'], T=IRL['T']):
    @row('train_rollout_irl' + _bt(B, T, IRL['B'], IRL['T']), 'mfg_train_rollout_irl', work=_w('mfg_train_rollout_irl', CTL))
    def build(a):
        L = _L()
        d = IRL['d']
        F = _ops().num_features(d)
        st = _net(a, d, IRL['n3'], IRL['n4'])
        mat = a.inp('mat_pi0', a.simplex((NUM_START, d), 34))
        th, w, acc = a.io('theta', a.f64(THETA)), a.w(d, True), a.io('reward_acc', a.f64(-3.25))
        traj, last, r, delta, g = _rollout_outs(a, B, d, T)
        P, G, n = a.out('P', (B, T, d, d)), a.out('G', (F + 3,), F64), wsb(B * T, d)
        ws = a.ws(n, zero=CONTROL)
        return lambda: call('mfg_train_rollout_irl', p(mat), NUM_START, None, B, d, T, p(th), SHIFT, SCALE, p(w), GAMMA, 7, 3, 100,
                            L.TRAIN_APPLY | L.ROLLOUT_DISCOUNT_POW, LR_C, LR_A, C.byref(st), 0xABCDEF, 100 * T, p(traj), p(last),
                            p(P), p(r), p(delta), p(g), p(G), p(acc), p(ws), n)


_irl_rollout()


def _irl_pop(step, shape=POP):
    entry = 'mfg_train_episodes_irl_pop' if step else 'mfg_train_rollouts_irl_pop'
    work = ((entry, 'workspace', SLICES),) + (((entry, 'pi_scratch', SCRATCH_KIND),) if step else ())

    @row(entry[4:] + _pop_name(shape), entry, work=work)
    def build(a):
        L = _L()
        K, B, T, E, d = (shape[k] for k in 'KBTEd')
        st = _net(a, d, IRL['n3'], IRL['n4'], K=K)               # per-learner networks, stacked tensors
        mat, th, sh, al, sd, w, G, acc, lrc, lra, ws, sb = _pop_common(a, 35, shape)
        rn_seed = a.inp('rn_seed', torch.arange(K, dtype=I64, device=a.dev) + 0x5EED + a.salt)
        rn_call0 = a.inp('rn_call0', torch.arange(K, dtype=I64, device=a.dev) * 3 + a.salt)
        head = (p(th), p(sh), p(al), p(w), GAMMA, p(sd), 3, 100)
        net = (p(lrc), p(lra), C.byref(st), 1, 0, None, None, p(rn_seed), p(rn_call0))
        if step:
            pi, P = a.out('pi_out', (K, B, d)), a.out('P', (K, B, d, d))
            scratch, r, delta, g = _episode_bufs(a, B, d, (K,))
            return lambda: call(entry, p(mat), NUM_START, p(pi), p(scratch), B, K, d, T, E, 1, 0, *head, L.PRECISION_MIXED, *net,
                                p(P), p(r), p(delta), p(g), p(G), p(acc), p(ws), sb)
        traj, last, r, delta, g = _rollout_outs(a, B, d, T, (K,))
        P = a.out('P', (K, B, T, d, d))
        return lambda: call(entry, p(mat), NUM_START, B, K, d, T, E, 1, 0, *head, L.ROLLOUT_DISCOUNT_POW, *net, p(traj), p(last),
                            p(P), p(r), p(delta), p(g), p(G), p(acc), p(ws), sb)


_irl_pop(True)
_irl_pop(False)

RN = dict(d=15, n3=8, n4=4, rows=6, T=3, nd=2, ng=3)


def _rn_dims():
    return (RN['d'], 5, 2, 3, RN['n3'], RN['n4'])


def _rn_state(a, lead=()):
    """Flat parameters and Adam moments ([NP], or [K, ld] with ld a multiple of 64) and the two trajectory stores."""
    NP = int(_L().lib().mfg_reward_net_num_params(*_rn_dims()))
    n = lead + ((NP + 63) // 64 * 64,) if lead else (NP,)
    d, rows, T = RN['d'], RN['rows'], RN['T']
    prm = a.io('params', (a.rand32(n, 36) - 0.5) * 0.4)
    m, v = a.io('adam_m', (a.rand32(n, 37) - 0.5) * 1e-3), a.io('adam_v', a.rand32(n, 38) * 1e-6)
    demo = (a.inp('demo_state', a.simplex((rows, T, d), 39)), a.inp('demo_action', a.simplex((rows, T, d, d), 40)))
    gen = (a.inp('gen_state', a.simplex(lead + (rows, T, d), 41)), a.inp('gen_action', a.simplex(lead + (rows, T, d, d), 42)))
    return NP, prm, m, v, demo, gen


def _rn_train_step(z):
    entry = 'mfg_reward_net_train_step' + ('_z' if z else '')

    @row(entry[4:], entry, work=_w(entry, SCRATCH_KIND))
    def build(a):
        nd, ng, T = RN['nd'], RN['ng'], RN['T']
        NP, prm, m, v, demo, gen = _rn_state(a)
        stats = a.out('stats', (4,))
        n = int(_L().lib().mfg_reward_net_train_workspace_bytes(*_rn_dims(), (nd + ng) * T))
        ws = a.ws((n + 3) // 4 * 4)
        dr, gr = (C.c_int32 * nd)(4, 1), (C.c_int32 * ng)(0, 5, 2)
        a.keep += [dr, gr]
        a.host.append(lambda: (dr.__setitem__(slice(0, nd), [0, 3]), gr.__setitem__(slice(0, ng), [1, 2, 3])))
        logz = (p(a.inp('gen_log_z', a.randn64((RN['rows'],), 43))),) if z else ()
        return lambda: call(entry, p(prm), p(m), p(v), *_rn_dims(), p(demo[0]), p(demo[1]), dr, nd, p(gen[0]), p(gen[1]), gr, ng, T,
                            5, 0.8, 1, 0xABCDEF0123, 2e-3, 0.9, 0.999, 1e-8, 3, 0, None, p(stats), p(ws), ws.numel(), *logz)


_rn_train_step(False)
_rn_train_step(True)


@row('reward_net_adam', 'mfg_reward_net_adam')
def _rn_adam(a):
    NP = int(_L().lib().mfg_reward_net_num_params(*_rn_dims()))
    prm = a.io('params', (a.rand32((NP,), 44) - 0.5) * 0.4)
    m, v = a.io('adam_m', (a.rand32((NP,), 45) - 0.5) * 1e-3), a.io('adam_v', a.rand32((NP,), 46) * 1e-6)
    grad = a.inp('grad', (a.rand32((NP,), 47) - 0.5) * 1e-2)
    return lambda: call('mfg_reward_net_adam', p(prm), p(m), p(v), p(grad), NP, 2e-3, 0.9, 0.999, 1e-8, 3)


# ---------------------------------------------------------------------------------------------------
# evaluation, forecast, scores, finite populations, consistency, distributions
# ---------------------------------------------------------------------------------------------------
@row('evaluate_pop', 'mfg_evaluate_pop', work=_w('mfg_evaluate_pop', SCRATCH_KIND))
def _evaluate_pop(a):
    d, K, R, N, Lr = 21, 3, 3, 5, 6
    emp = a.simplex((N, Lr, d), 48)
    e32, e64 = a.inp('emp32', emp), a.inp('emp64', emp.double())
    th, sh, al, sd = a.policies(K)
    metrics = a.out('metrics', (K, 8), F64)
    n = int(_L().lib().mfg_evaluate_pop_workspace_bytes(N, Lr, d, K, R, 0))
    ws = a.ws(n)
    return lambda: call('mfg_evaluate_pop', p(e32), p(e64), N, Lr, d, K, p(th), p(sh), p(al), p(sd), 37, R, _L().PRECISION_MIXED,
                        p(metrics), None, p(ws), n)


def _host_ranks(a, ranks, other):
    arr = (C.c_int32 * len(ranks))(*ranks)
    a.keep.append(arr)
    a.host.append(lambda: arr.__setitem__(slice(0, len(ranks)), list(other)))
    return arr


@row('forecast_pop-R3', 'mfg_forecast_pop', work=_w('mfg_forecast_pop', SCRATCH_KIND))
def _forecast_pop(a):
    d, K, N, H, R = 21, 2, 2, 4, 3
    emp = a.simplex((N, H, d), 49)
    s32, e32, e64 = a.inp('start32', emp[:, 0]), a.inp('emp32', emp), a.inp('emp64', emp.double())
    th, sh, al, sd = a.policies(K)
    ranks = _host_ranks(a, (0, R - 1, R // 2), (1, 1, 0))
    mean, std = a.out('mean', (K, N, H, d), F64), a.out('std', (K, N, H, d), F64)
    quant, curves = a.out('quant', (K, N, H, 3, d)), a.out('curves', (K, H, 4), F64)
    n = int(_L().lib().mfg_forecast_pop_workspace_bytes(N, H, d, K, R, 0))
    ws = a.ws(n)
    return lambda: call('mfg_forecast_pop', p(s32), N, H, d, K, p(th), p(sh), p(al), p(sd), 37, R, _L().PRECISION_MIXED, ranks, 3,
                        p(e32), p(e64), p(mean), p(std), p(quant), p(curves), None, p(ws), n)


@row('forecast_score-R65-energy', 'mfg_forecast_score', work=_w('mfg_forecast_score', SCRATCH_KIND))
def _forecast_score(a):
    d, K, N, H, R = 15, 2, 2, 3, 65
    emp = a.simplex((N, H, d), 50)
    traj, e32, e64 = a.inp('traj', a.simplex((K, N * R, H, d), 51)), a.inp('emp32', emp), a.inp('emp64', emp.double())
    crps, less, equal = a.out('crps', (K, N, H, d), F64), a.out('less', (K, N, H, d), I32), a.out('equal', (K, N, H, d), I32)
    en, summary = a.out('energy', (K, N, H), F64), a.out('summary', (K, H, 2), F64)
    n = int(_L().lib().mfg_forecast_score_workspace_bytes(N, H, d, K, R))
    ws = a.ws(n)
    return lambda: call('mfg_forecast_score', p(traj), N, H, d, K, R, p(e32), p(e64), p(crps), p(less), p(equal), p(en), p(summary),
                        p(ws), n)


AGENTS = 1000


def _counts(pi):
    """Rows of int32 counts that sum to AGENTS, apportioned from simplex rows."""
    c = torch.floor(pi.double() * AGENTS).to(I32)
    c[..., 0] += AGENTS - c.sum(-1).to(I32)
    return c


@row('agents_step_pop', 'mfg_agents_step_pop')
def _agents_step(a):
    K, B, d = 2, 13, 21
    counts, P = a.inp('counts', _counts(a.simplex((K, B, d), 52))), a.inp('P', a.simplex((K, B, d, d), 53))
    sd = a.policies(K)[3]
    cn, pn, mv = a.out('counts_next', (K, B, d), I32), a.out('pi_next', (K, B, d)), a.out('moves', (K, B, d, d), I32)
    return lambda: call('mfg_agents_step_pop', p(counts), p(P), B, d, K, AGENTS, p(sd), 5, 1000, p(cn), p(pn), p(mv))


@row('forecast_agents_pop-H4', 'mfg_forecast_agents_pop', work=_w('mfg_forecast_agents_pop', SCRATCH_KIND))
def _forecast_agents(a):
    d, K, N, H, R = 21, 2, 2, 4, 3
    emp = a.simplex((N, H, d), 54)
    c0, e32, e64 = a.inp('counts0', _counts(emp[:, 0])), a.inp('emp32', emp), a.inp('emp64', emp.double())
    th, sh, al, sd = a.policies(K)
    ranks = _host_ranks(a, (0, R - 1, R // 2), (1, 1, 0))
    mean, std = a.out('mean', (K, N, H, d), F64), a.out('std', (K, N, H, d), F64)
    quant, curves = a.out('quant', (K, N, H, 3, d)), a.out('curves', (K, H, 4), F64)
    ct, act = a.out('counts_traj', (K, N * R, H, d), I32), a.out('actions', (K, N * R, H - 1, d, d))
    n = int(_L().lib().mfg_forecast_agents_pop_workspace_bytes(N, H, d, K, R, 0, 1))
    ws = a.ws(n)
    return lambda: call('mfg_forecast_agents_pop', p(c0), N, H, d, K, AGENTS, p(th), p(sh), p(al), p(sd), 37, R,
                        _L().PRECISION_MIXED, ranks, 3, p(e32), p(e64), p(mean), p(std), p(quant), p(curves), None, p(ct), p(act),
                        p(ws), n)


@row('consistency_given', 'mfg_consistency_given', work=_w('mfg_consistency_given', SCRATCH_KIND))
def _consistency_given(a):
    """Without `steps` the per-hour values live in the workspace, which the second launch reads."""
    K, M, T, d = 2, 3, 2, 7
    P, metrics = a.inp('P', a.simplex((K, M, T, d, d), 55)), a.out('metrics', (K, 4), F64)
    n = int(_L().lib().mfg_consistency_given_workspace_bytes(K, M, T, 0))
    ws = a.ws(n)
    return lambda: call('mfg_consistency_given', p(P), K, M, T, d, p(metrics), None, None, p(ws), n)


@row('consistency_pop', 'mfg_consistency_pop', work=_w('mfg_consistency_pop', SCRATCH_KIND))
def _consistency_pop(a):
    d, K, N, H, R = 15, 2, 3, 3, 2
    s32 = a.inp('start32', a.simplex((N, d), 56))
    th, sh, al, sd = a.policies(K)
    metrics, steps = a.out('metrics', (K, 4), F64), a.out('steps', (K, N * R, H - 1, 2), F64)
    n = int(_L().lib().mfg_consistency_pop_workspace_bytes(N, H, d, K, R, 1, 0, 0))
    ws = a.ws(n)
    return lambda: call('mfg_consistency_pop', p(s32), N, H, d, K, p(th), p(sh), p(al), p(sd), 37, R, _L().PRECISION_MIXED,
                        p(metrics), p(steps), None, None, None, p(ws), n)


@row('row_distribution', 'mfg_row_distribution')
def _row_distribution(a):
    R, N, bins, G = 3, 257, 16, 20
    stride = N + 3
    v = a.inp('values', a.randn64((R, stride), 57).float())
    moments, counts = a.out('moments', (R, 6), F64), a.out('counts', (R, bins), I64)
    edges, status, density = a.out('edges', (R, bins + 1), F64), a.out('status', (R,), I32), a.out('density', (R, G), F64)
    n = int(_L().lib().mfg_row_distribution_workspace_bytes(R, N, bins, G))
    ws = a.ws(n) if n else None
    return lambda: call('mfg_row_distribution', p(v), R, N, stride, bins, 0, 0.0, 0.0, G, -3.0, 3.0, p(moments), p(counts), p(edges),
                        p(density), p(status), p(ws), n)


@row('action_mean_pop', 'mfg_action_mean_pop', work=_w('mfg_action_mean_pop', SCRATCH_KIND))
def _action_mean(a):
    K, N, d = 2, 37, 21
    act, mean = a.inp('action', a.simplex((K, N, d, d), 58)), a.out('mean', (K, d, d), F64)
    n = int(_L().lib().mfg_action_mean_pop_workspace_bytes(K, N, d))
    ws = a.ws(n)
    return lambda: call('mfg_action_mean_pop', p(act), N * d * d, K, N, d, p(mean), p(ws), n)


# ---------------------------------------------------------------------------------------------------
# launch-once kernels
# ---------------------------------------------------------------------------------------------------
LD, LB = 21, 5


@row('policy_logpdf', 'mfg_policy_logpdf')
def _policy_logpdf(a):
    pi, P = a.inp('pi', a.simplex((LB, LD), 59)), a.inp('P', a.simplex((LB, LD, LD), 60))
    th, out = a.inp('thetas', a.f64(2.0, 6.5, 8.64)), a.out('logpdf', (LB, 3), F64)
    return lambda: call('mfg_policy_logpdf', p(pi), p(P), LB, LD, p(th), 3, 0.05, 1.0, 1.0 + 1e-6, 0.0, p(out))


@row('backward_value', 'mfg_backward_value')
def _backward_value(a):
    T = 2
    P = a.inp('P', a.simplex((LB, T, LD, LD), 61))
    V, l1, js = a.out('V', (LB, T + 1, LD), F64), a.out('l1', (LB, T), F64), a.out('jsd', (LB, T), F64)
    return lambda: call('mfg_backward_value', p(P), LB, T, LD, p(V), p(l1), p(js))


@row('value', 'mfg_value')
def _value(a):
    pi, w, out = a.inp('pi', a.simplex((LB, LD), 62)), a.w(LD), a.out('value', (LB,), F64)
    return lambda: call('mfg_value', p(pi), p(w), LB, LD, p(out))


@row('features', 'mfg_features')
def _features(a):
    pi, out = a.inp('pi', a.simplex((LB, LD), 63)), a.out('phi', (LB, _ops().num_features(LD)), F64)
    return lambda: call('mfg_features', p(pi), LB, LD, p(out))


@row('alpha', 'mfg_alpha')
def _alpha(a):
    pi, th = a.inp('pi', a.simplex((LB, LD), 64)), a.theta()
    al, ad = a.out('alpha', (LB, LD, LD), F64), a.out('alpha_deriv', (LB, LD, LD), F64)
    return lambda: call('mfg_alpha', p(pi), LB, LD, p(th), SHIFT, p(al), p(ad))


@row('score', 'mfg_score')
def _score(a):
    pi, P, th = a.inp('pi', a.simplex((LB, LD), 65)), a.inp('P', a.simplex((LB, LD, LD), 66)), a.theta()
    gm, gf = a.out('g_mixed', (LB,), F64), a.out('g_f64', (LB,), F64)

    def issue():
        call('mfg_score', p(pi), p(P), LB, LD, p(th), SHIFT, _L().PRECISION_MIXED, p(gm))
        call('mfg_score', p(pi), p(P), LB, LD, p(th), SHIFT, _L().PRECISION_F64, p(gf))
    return issue


@row('jsd', 'mfg_jsd')
def _jsd(a):
    x, y, out = a.inp('p', a.simplex((LB, LD), 67)), a.inp('q', a.simplex((LB, LD), 68)), a.out('jsd', (LB,), F64)
    return lambda: call('mfg_jsd', p(x), p(y), LB, LD, p(out))


@row('gather_start', 'mfg_gather_start')
def _gather_start(a):
    mat, idx = a.inp('mat_pi0', a.simplex((NUM_START, LD), 69)), a.inp('idx', a.index(LB, NUM_START, 70))
    out = a.out('pi0', (LB, LD))
    return lambda: call('mfg_gather_start', p(mat), NUM_START, p(idx), LB, LD, p(out))


@row('draw_start', 'mfg_draw_start')
def _draw_start(a):
    mat = a.inp('mat_pi0', a.simplex((NUM_START, LD), 71))
    idx, out = a.out('idx', (LB,), I32), a.out('pi0', (LB, LD))
    return lambda: call('mfg_draw_start', p(mat), NUM_START, LB, LD, 2024, 30, 5, p(idx), p(out))


@row('dirichlet_from_gamma', 'mfg_dirichlet_from_gamma')
def _dirichlet_from_gamma(a):
    y = a.rand32((LB, LD, LD), 72) * 3.0
    y[0, 0] = 0.0                                       # an all-zero row: uniform
    y, out = a.inp('y', y), a.out('P', (LB, LD, LD))
    return lambda: call('mfg_dirichlet_from_gamma', p(y), LB, LD, p(out))


@row('philox_raw', 'mfg_philox_raw')
def _philox_raw(a):
    """No device input: only the pending check and the capture say something here."""
    out = a.out('out', (37, 4), I32)
    return lambda: call('mfg_philox_raw', 0x123456789ABCDEF, 5, 6, 7, 8, 37, p(out))


# ---------------------------------------------------------------------------------------------------
# the documented drainers: a host array goes into device scratch and the stream is drained before the first launch
# ---------------------------------------------------------------------------------------------------
@row('reward_net_forward_pop', 'mfg_reward_net_forward_pop', work=(('mfg_reward_net_forward_pop', 'scratch', SCRATCH_KIND),))
def _forward_pop(a):
    d, K, N = 21, 3, 37
    st = _net(a, d, 8, 4, K=K)
    s, act = a.inp('state', a.simplex((N, d), 73)), a.inp('action', a.simplex((N, d, d), 74))
    out, scratch = a.out('reward', (K, N), keep=7.0), a.ws(16 * 2)
    return lambda: _ops().reward_net_forward_pop(st, True, K, s, act, [2, 0], [77, 1 << 40], out=out, scratch=scratch)


def _train_steps_pop(z):
    entry = 'mfg_reward_net_train_steps_pop' + ('_z' if z else '')

    @row(entry[4:], entry, work=((entry, 'workspace', SCRATCH_KIND), (entry, 'plan_dev', SCRATCH_KIND)))
    def build(a):
        ops = _ops()
        nd, ng, T, rows = RN['nd'], RN['ng'], RN['T'], RN['rows']
        K, U, active = 3, 2, [2, 0]
        NP, prm, m, v, demo, gen = _rn_state(a, (K,))
        stats = a.out('stats', (K, 4), keep=7.0)
        sl = (int(_L().lib().mfg_reward_net_train_workspace_bytes(*_rn_dims(), (nd + ng) * T)) + 255) // 256 * 256
        plan = ops.rn_train_plan(U * len(active))

        def fill(shift):
            for u in range(U):
                for s, k in enumerate(active):
                    e = plan[u * len(active) + s]
                    e['learner'], e['key'], e['lr'], e['adam_step'] = k, 1000 * u + k + (1 << 35) + shift, 2e-3, u + 1 + shift
                    e['demo_rows'][:nd] = [(3 * j + u + shift) % rows for j in range(nd)]
                    e['gen_rows'][:ng] = [(rows - 1 - j - u - shift) % rows for j in range(ng)]
        fill(0)
        a.host.append(lambda: fill(1))
        ws, plan_dev = a.ws(len(active) * sl), a.ws(plan.nbytes)
        logz = a.inp('gen_log_z', a.randn64((K, rows), 75)) if z else None
        return lambda: ops.reward_net_train_steps_pop(prm, m, v, prm.shape[1], K, _rn_dims(), demo, gen, plan, U, len(active), nd, ng,
                                                      T, 5, 0.8, True, stats, ws, plan_dev, gen_log_z=logz)


_train_steps_pop(False)
_train_steps_pop(True)


@row('traj_log_z_pop', 'mfg_traj_log_z_pop', work=(('mfg_traj_log_z_pop', 'scratch', SCRATCH_KIND),))
def _traj_log_z(a):
    K, cap, T, d = 2, 6, 3, 15
    state, action = a.inp('state', a.simplex((cap, T, d), 76)), a.inp('action', a.simplex((cap, T, d, d), 77))
    th = a.inp('thetas', a.f64(7.9, 8.5, 8.8, 8.1).view(K, 2))
    sh = a.inp('shifts', a.f64(0.05, -0.02))
    out, scratch = a.out('log_z', (K, cap), F64, keep=7.0), a.ws(4 * 3, I32)
    return lambda: _ops().traj_log_z_pop(state, action, [4, 0, 2], th, sh, float(np.log(9.0)), out=out, scratch=scratch)


def covered_entries():
    return sorted({e for r in ROWS for e in r.entries})


# ---------------------------------------------------------------------------------------------------
# the procedures
# ---------------------------------------------------------------------------------------------------
class Reference:
    def __init__(self, true, want, enqueue_s):
        self.true, self.want, self.enqueue_s = true, want, enqueue_s


def reference(r, dev):
    """The row on the default stream with everything synchronised; once more on fresh buffers to time the (warm) enqueue."""
    a = Bufs(dev, 0)
    issue = r.build(a)
    true = {n: t.clone() for n, t in a.inputs.items()}
    torch.cuda.synchronize()
    issue()
    torch.cuda.synchronize()
    want = {n: t.clone() for n, t in a.compared().items()}
    b = Bufs(dev, 0)
    issue = r.build(b)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    issue()
    dt = time.perf_counter() - t0
    torch.cuda.synchronize()
    return Reference(true, want, dt)


def differing(got, want):
    """Names of the buffers whose bits differ from the reference."""
    assert set(got) == set(want)
    return sorted(n for n in want if got[n].shape != want[n].shape or not same(got[n], want[n]))


def _write_true(b, ref):
    assert set(b.inputs) == set(ref.true)
    for n, t in b.inputs.items():
        assert t.shape == ref.true[n].shape and t.dtype == ref.true[n].dtype, n
        t.copy_(ref.true[n])


def run_delayed(r, ref, dev, cycles, side, call_stream=None):
    """Method A on the stream `side`.  Returns (the producer was still pending when the call returned, {name: clone}).
    call_stream: the stream handle the call is handed instead of the producer's (a wrong-stream caller; the decoys are valid,
    nothing faults)."""
    b = Bufs(dev, 1)
    issue = r.build(b)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        torch.cuda._sleep(cycles)
        _write_true(b, ref)
        if call_stream is None:
            issue()
        else:
            with forced_stream(call_stream):
                issue()
        pending = not side.query()
        b.scribble()
        got = {n: t.clone() for n, t in b.compared().items()}
    side.synchronize()
    torch.cuda.synchronize()
    return pending, got


def run_captured(r, ref, dev, side):
    """Method B, captured on the stream `side`.  Returns the list of findings (empty: the row passes)."""
    b = Bufs(dev, 1)
    issue = r.build(b)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            issue()
    b.scribble()
    torch.cuda.synchronize()
    found = []
    for n, (t, fill) in b.outs.items():
        if not same(t, torch.full_like(t, fill)):
            found.append('%s was written at capture time' % n)
    for k in (1, 2):
        _write_true(b, ref)                  # (the in/out buffers go back to their start values)
        b.refill()
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        found += ['replay %d: %s differs from the reference' % (k, n) for n in differing(dict(b.compared()), ref.want)]
    return found


def sleep_cycles_per_ms():
    """torch.cuda._sleep's clock, measured: its cycles per millisecond on this device."""
    n = 20_000_000
    torch.cuda._sleep(1000)
    torch.cuda.synchronize()
    best = None
    for _ in range(2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        torch.cuda._sleep(n)
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1)
        best = ms if best is None else min(best, ms)
    assert best > 0.05, 'torch.cuda._sleep(%d) took %.4f ms: no usable delay' % (n, best)
    return n / best


def independent_side_stream(dev, cycles, tries=32):
    """A side stream behind whose pending work the null stream does NOT queue.  The runtime multiplexes its streams onto a few
    hardware queues; a launch that went to stream 0 by mistake and shares its queue with the producer's stream would run behind
    the producer by accident and look correct.  Measured, not assumed: a sleep on the candidate, one tiny kernel on the null
    stream, which must finish while the sleep is still pending."""
    x = torch.zeros(1, device=dev)
    for _ in range(tries):
        side = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            torch.cuda._sleep(cycles)
        x.add_(1.0)
        done = torch.cuda.Event()
        done.record()
        t0, ran = time.perf_counter(), False
        while not ran and time.perf_counter() - t0 < 5e-3:
            ran = done.query()
        independent = ran and not side.query()
        torch.cuda.synchronize()
        if independent:
            return side
    raise AssertionError('no side stream of %d found that runs independently of the null stream' % tries)
