"""Thin tensor-level wrappers over the C ABI: torch owns device memory and streams, HIP does the math.

Every function takes CUDA(ROCm) tensors, enqueues on torch's current stream and returns tensors.
Shapes follow include/mfg_hip.h: pi [B,d] fp32, P [B,d,d] fp32, theta / w fp64 device tensors.
"""
from __future__ import annotations

import torch

from . import _lib as L


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _chk_f32(t, name):
    if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
        raise ValueError('%s must be a contiguous float32 CUDA tensor' % name)
    return t


def _chk_f64(t, name):
    if not (t.is_cuda and t.dtype == torch.float64 and t.is_contiguous()):
        raise ValueError('%s must be a contiguous float64 CUDA tensor' % name)
    return t


def _rollout_flags(discount_pow, precision):
    """The MFG_ROLLOUT_DISCOUNT_POW / MFG_ROLLOUT_F64 bits of a rollout call's flags (callers add ROLLOUT_TD, ROLLOUT_WRITE_P
    or TRAIN_APPLY)."""
    return (L.ROLLOUT_DISCOUNT_POW if discount_pow else 0) | (L.ROLLOUT_F64 if L.PRECISIONS[precision] == L.PRECISION_F64 else 0)


def _ptr(t):
    """Device address of a tensor; None -> NULL; a plain int is taken as an address already (e.g. one entry of a
    per-episode accumulator array: base.data_ptr() + 8 * k, without building a tensor view per episode)."""
    if t is None or isinstance(t, int):
        return t
    return t.data_ptr()


def init():
    """One-time per-device setup of the HIP library (optional; done lazily otherwise)."""
    L.check(L.lib().mfg_init(), 'mfg_init')


def status(synchronize: bool = True) -> int:
    """Bits of the device status word (0 = healthy; _lib.STATUS_MIXED_RANGE: a mixed-precision sampling launch found
    theta outside the range of its separable exponential, include/mfg_hip.h).  synchronize=True waits for the current
    stream first so that every launch issued so far has reported."""
    import ctypes as C
    if synchronize:
        torch.cuda.current_stream().synchronize()
    bits = C.c_uint(0)
    L.lib().mfg_status(C.byref(bits))
    return int(bits.value)


def clear_status():
    L.check(L.lib().mfg_clear_status(), 'mfg_clear_status')


class Context:
    """An mfg_ctx_t (include/mfg_hip.h): the mutable library state of ONE model instance -- its status word.  `bind()` makes it
    the calling thread's current context: every ops.* call from this thread then reports into / is refused on this context's
    word, not another instance's.  The drop-in classes create one each and bind it at the start of every public method."""

    def __init__(self, device=None):
        import ctypes as C
        self._ptr = None
        dev = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
        out = C.c_void_p()
        with torch.cuda.device(dev):
            L.check(L.lib().mfg_ctx_create(C.byref(out)), 'mfg_ctx_create')
        self._ptr = out.value
        self.device = dev

    def bind(self):
        lib = L.lib()
        if lib.mfg_ctx_current() != self._ptr:
            with torch.cuda.device(self.device):
                L.check(lib.mfg_ctx_bind(self._ptr), 'mfg_ctx_bind')
        return self

    @staticmethod
    def unbind():
        L.check(L.lib().mfg_ctx_bind(None), 'mfg_ctx_bind')

    KEEP = object()        # bind_scoped(): this context was bound already, restore() has nothing to do

    def bind_scoped(self):
        """bind() that returns what restore() needs to put the calling thread's previous binding back: KEEP if this context
        was current already (nested public methods: one ctypes call), else the previous context's address (None = the
        device's default context)."""
        prev = L.lib().mfg_ctx_current()
        if prev == self._ptr:
            return Context.KEEP
        with torch.cuda.device(self.device):
            L.check(L.lib().mfg_ctx_bind(self._ptr), 'mfg_ctx_bind')
        return prev

    @staticmethod
    def restore(prev):
        if prev is Context.KEEP:
            return
        lib = L.lib()
        # (the previous context may have been destroyed meanwhile, or belong to another device than the current one: then the
        #  thread goes back to the default context -- never to a stale pointer)
        if prev is None or lib.mfg_ctx_bind(prev) != 0:
            lib.mfg_ctx_bind(None)

    def status(self, synchronize=True) -> int:
        import ctypes as C
        if synchronize:
            torch.cuda.current_stream(self.device).synchronize()
        bits = C.c_uint(0)
        L.lib().mfg_ctx_status(self._ptr, C.byref(bits))
        return int(bits.value)

    def clear_status(self):
        L.check(L.lib().mfg_ctx_clear_status(self._ptr), 'mfg_ctx_clear_status')

    def set_pop_control(self, state=None, status=None, theta_prev=None, episodes_run=None, stop_criteria=None):
        """mfg_ctx_set_pop_control: bind a population control block -- device tensors [K]: state / status / episodes_run int32,
        theta_prev / stop_criteria float64 -- to this context; every population training call made with the context bound
        then retires learners on the device (include/mfg_hip.h).  No arguments: clear it.  The caller keeps the tensors alive
        while the block is set."""
        import ctypes as C
        if state is None:
            L.check(L.lib().mfg_ctx_set_pop_control(self._ptr, None), 'mfg_ctx_set_pop_control')
            return
        K = int(state.shape[0])
        for name, t, dt in (('state', state, torch.int32), ('status', status, torch.int32),
                            ('theta_prev', theta_prev, torch.float64), ('episodes_run', episodes_run, torch.int32),
                            ('stop_criteria', stop_criteria, torch.float64)):
            if t is None or t.dtype != dt or t.dim() != 1 or t.shape[0] != K or not t.is_contiguous() or not t.is_cuda:
                raise ValueError('set_pop_control: %s must be a contiguous %s device tensor [%d]' % (name, dt, K))
        blk = L.PopControlStruct(state.data_ptr(), status.data_ptr(), theta_prev.data_ptr(), episodes_run.data_ptr(),
                                 stop_criteria.data_ptr(), K)
        L.check(L.lib().mfg_ctx_set_pop_control(self._ptr, C.byref(blk)), 'mfg_ctx_set_pop_control')

    def set_pop_validate(self, emp32=None, emp64=None, *, period=1, column=3, with_score=False, patience=0, first_step=0,
                         repeats=1, curve=None, checks=None, best_value=None, best_check=None, since_best=None,
                         best_theta=None, best_w=None, workspace=None, workspace_bytes=None):
        """mfg_ctx_set_pop_validate: bind a population validation block to this context; every population training call made
        with the context bound then runs a held-out check every `period` episodes (include/mfg_hip.h).  emp32 / emp64 [N,L,d]:
        the held-out rows; curve [K, max_checks, 10], best_value / best_theta [K], best_w [K,F] float64 and checks /
        best_check / since_best [K] int32 device tensors, initialised by the caller (checks, since_best 0; best_value +inf;
        best_check -1); workspace: pop_validate_workspace (workspace_bytes: what the block announces, default the tensor's
        size).  No arguments: clear it.  The caller keeps the tensors alive while the block is set."""
        import ctypes as C
        if emp32 is None:
            L.check(L.lib().mfg_ctx_set_pop_validate(self._ptr, None), 'mfg_ctx_set_pop_validate')
            return
        _chk_f32(emp32, 'emp32'); _chk_f64(emp64, 'emp64')
        if emp32.dim() != 3 or tuple(emp64.shape) != tuple(emp32.shape):
            raise ValueError('emp32 / emp64: expected two [N, L, d] tensors of the same shape, got %s and %s'
                             % (tuple(emp32.shape), tuple(emp64.shape)))
        N, Lr, _d = emp32.shape
        if curve is None or curve.dim() != 3 or curve.shape[2] != L.POP_VALIDATE_COLUMNS:
            raise ValueError('set_pop_validate: curve must be a [K, max_checks, %d] tensor' % L.POP_VALIDATE_COLUMNS)
        K, max_checks = int(curve.shape[0]), int(curve.shape[1])
        for name, t, dt, nd in (('curve', curve, torch.float64, 3), ('checks', checks, torch.int32, 1),
                                ('best_value', best_value, torch.float64, 1), ('best_check', best_check, torch.int32, 1),
                                ('since_best', since_best, torch.int32, 1), ('best_theta', best_theta, torch.float64, 1),
                                ('best_w', best_w, torch.float64, 2)):
            if t is None or t.dtype != dt or t.dim() != nd or t.shape[0] != K or not t.is_contiguous() or not t.is_cuda:
                raise ValueError('set_pop_validate: %s must be a contiguous %s device tensor with %d rows' % (name, dt, K))
        if workspace is None or not workspace.is_cuda or not workspace.is_contiguous():
            raise ValueError('set_pop_validate: workspace must be a contiguous device tensor')
        if workspace_bytes is None:
            workspace_bytes = workspace.numel() * workspace.element_size()
        blk = L.PopValidateStruct(emp32.data_ptr(), emp64.data_ptr(), curve.data_ptr(), checks.data_ptr(), best_value.data_ptr(),
                                  best_check.data_ptr(), since_best.data_ptr(), best_theta.data_ptr(), best_w.data_ptr(),
                                  workspace.data_ptr(), int(workspace_bytes), int(N), int(Lr), int(repeats), int(period),
                                  int(column), int(with_score), int(patience), max_checks, K, int(first_step))
        L.check(L.lib().mfg_ctx_set_pop_validate(self._ptr, C.byref(blk)), 'mfg_ctx_set_pop_validate')

    def set_pop_evolve(self, lr_critic=None, lr_actor=None, *, every=1, n_top=1, n_bottom=1, perturb=3, factors=(0.8, 1.25),
                       lr_critic_bounds=(1e-6, 10.0), lr_actor_bounds=(1e-8, 1.0), seed=0, order=None, active=None, rank=None,
                       parent=None, lr_log=None, K=None):
        """mfg_ctx_set_pop_evolve: bind a population evolve block to this context; the forward population training calls made
        with the context (and a validation block) bound then run an exploit / explore step behind every `every`-th held-out
        check (include/mfg_hip.h).  lr_critic / lr_actor [K] float64: the SAME device tensors the training call is given (a
        step writes them); order [K], active [1] int32 scratch; rank, parent [K, max_steps] int32 (the caller sets -1) and
        lr_log [K, max_steps, 2] float64 (NaN) logs.  perturb: bit 0 critic, bit 1 actor.  K: what the block announces
        (default the tensors').  No arguments: clear it.  The caller keeps the tensors alive while the block is set."""
        import ctypes as C
        if lr_critic is None:
            L.check(L.lib().mfg_ctx_set_pop_evolve(self._ptr, None), 'mfg_ctx_set_pop_evolve')
            return
        n = int(lr_critic.shape[0])
        if rank is None or rank.dim() != 2:
            raise ValueError('set_pop_evolve: rank must be a [K, max_steps] tensor')
        max_steps = int(rank.shape[1])
        for name, t, dt, shape in (('lr_critic', lr_critic, torch.float64, (n,)), ('lr_actor', lr_actor, torch.float64, (n,)),
                                   ('order', order, torch.int32, (n,)), ('active', active, torch.int32, (1,)),
                                   ('rank', rank, torch.int32, (n, max_steps)), ('parent', parent, torch.int32, (n, max_steps)),
                                   ('lr_log', lr_log, torch.float64, (n, max_steps, 2))):
            if t is None or t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous() or not t.is_cuda:
                raise ValueError('set_pop_evolve: %s must be a contiguous %s device tensor %s' % (name, dt, list(shape)))
        blk = L.PopEvolveStruct(lr_critic.data_ptr(), lr_actor.data_ptr(), order.data_ptr(), active.data_ptr(), rank.data_ptr(),
                                parent.data_ptr(), lr_log.data_ptr(), int(seed) & 0xFFFFFFFFFFFFFFFF, float(factors[0]),
                                float(factors[1]), float(lr_critic_bounds[0]), float(lr_critic_bounds[1]),
                                float(lr_actor_bounds[0]), float(lr_actor_bounds[1]), int(every), int(n_top), int(n_bottom),
                                int(perturb), max_steps, n if K is None else int(K))
        L.check(L.lib().mfg_ctx_set_pop_evolve(self._ptr, C.byref(blk)), 'mfg_ctx_set_pop_evolve')

    def close(self):
        if self._ptr is not None:
            try:
                L.lib().mfg_ctx_destroy(self._ptr)           # (also unbinds it from THIS thread)
            finally:
                self._ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def num_features(d: int) -> int:
    return int(L.lib().mfg_num_features(d))


def feature_index(i: int, j: int, d: int) -> int:
    return int(L.lib().mfg_feature_index(i, j, d))


def workspace(N: int, d: int, device) -> torch.Tensor:
    n = int(L.lib().mfg_workspace_bytes(N, d))
    return torch.zeros(max(n, 8) // 8, dtype=torch.float64, device=device)   # zeroed: trailing control block (mfg_hip.h)


def gather_start(mat_pi0, idx):
    _chk_f32(mat_pi0, 'mat_pi0')
    if idx.dtype != torch.int32 or not idx.is_cuda:
        raise ValueError('idx must be an int32 CUDA tensor')
    B, d = idx.numel(), mat_pi0.shape[1]
    out = torch.empty(B, d, dtype=torch.float32, device=mat_pi0.device)
    L.check(L.lib().mfg_gather_start(mat_pi0.data_ptr(), mat_pi0.shape[0], idx.data_ptr(), B, d, out.data_ptr(),
                                     _stream()), 'mfg_gather_start')
    return out


def draw_start(mat_pi0, B, seed, step, traj_offset=0, want_idx=False, want_pi0=True):
    """Start states of B trajectories drawn on the device (mfg_draw_start: Philox keyed by seed, the episode's first
    step, the global trajectory id).  Returns (idx int32 [B] | None, pi0 [B,d] | None)."""
    _chk_f32(mat_pi0, 'mat_pi0')
    d = mat_pi0.shape[1]
    idx = torch.empty(B, dtype=torch.int32, device=mat_pi0.device) if want_idx else None
    pi0 = torch.empty(B, d, dtype=torch.float32, device=mat_pi0.device) if want_pi0 else None
    L.check(L.lib().mfg_draw_start(mat_pi0.data_ptr(), mat_pi0.shape[0], int(B), d, int(seed), int(step), int(traj_offset),
                                   _ptr(idx), _ptr(pi0), _stream()), 'mfg_draw_start')
    return idx, pi0


def alpha(pi, theta, shift, want_alpha=True, want_deriv=True):
    _chk_f32(pi, 'pi'); _chk_f64(theta, 'theta')
    B, d = pi.shape
    a = torch.empty(B, d, d, dtype=torch.float64, device=pi.device) if want_alpha else None
    ad = torch.empty(B, d, d, dtype=torch.float64, device=pi.device) if want_deriv else None
    L.check(L.lib().mfg_alpha(pi.data_ptr(), B, d, theta.data_ptr(), float(shift), _ptr(a), _ptr(ad), _stream()),
            'mfg_alpha')
    return a, ad


def dirichlet_from_gamma(y):
    _chk_f32(y, 'y')
    B, d = y.shape[0], y.shape[-1]
    P = torch.empty_like(y)
    L.check(L.lib().mfg_dirichlet_from_gamma(y.data_ptr(), B, d, P.data_ptr(), _stream()), 'mfg_dirichlet_from_gamma')
    return P


def sample_dirichlet(pi, theta, shift, alpha_scale, seed, step=0, traj_offset=0, out=None, precision='mixed'):
    _chk_f32(pi, 'pi'); _chk_f64(theta, 'theta')
    B, d = pi.shape
    P = out if out is not None else torch.empty(B, d, d, dtype=torch.float32, device=pi.device)
    L.check(L.lib().mfg_sample_dirichlet(pi.data_ptr(), B, d, theta.data_ptr(), float(shift), float(alpha_scale),
                                         int(seed), int(step), int(traj_offset), L.PRECISIONS[precision], P.data_ptr(),
                                         _stream()),
            'mfg_sample_dirichlet')
    return P


def philox_raw(seed, first_ctr, c1, c2, c3, n, device):
    out = torch.empty(n, 4, dtype=torch.int32, device=device)
    L.check(L.lib().mfg_philox_raw(int(seed), int(first_ctr), int(c1), int(c2), int(c3), n, out.data_ptr(), _stream()),
            'mfg_philox_raw')
    return out


def step_given_P(pi, P, reward_kind=L.REWARD_MFG_AC2, want_reward=True):
    _chk_f32(pi, 'pi'); _chk_f32(P, 'P')
    B, d = pi.shape
    if P.shape != (B, d, d):
        raise ValueError('P must be [B,d,d]')
    pi_next = torch.empty_like(pi)
    reward = torch.empty(B, dtype=torch.float32, device=pi.device) if want_reward else None
    L.check(L.lib().mfg_step_given_P(pi.data_ptr(), P.data_ptr(), B, d, int(reward_kind), pi_next.data_ptr(),
                                     _ptr(reward), _stream()), 'mfg_step_given_P')
    return pi_next, reward


def value(pi, w):
    _chk_f32(pi, 'pi'); _chk_f64(w, 'w')
    B, d = pi.shape
    out = torch.empty(B, dtype=torch.float64, device=pi.device)
    L.check(L.lib().mfg_value(pi.data_ptr(), w.data_ptr(), B, d, out.data_ptr(), _stream()), 'mfg_value')
    return out


def features(pi):
    _chk_f32(pi, 'pi')
    B, d = pi.shape
    out = torch.empty(B, num_features(d), dtype=torch.float64, device=pi.device)
    L.check(L.lib().mfg_features(pi.data_ptr(), B, d, out.data_ptr(), _stream()), 'mfg_features')
    return out


def score(pi_alpha, P, theta, shift, precision='mixed'):
    _chk_f32(pi_alpha, 'pi'); _chk_f32(P, 'P'); _chk_f64(theta, 'theta')
    B, d = pi_alpha.shape
    g = torch.empty(B, dtype=torch.float64, device=P.device)
    L.check(L.lib().mfg_score(pi_alpha.data_ptr(), P.data_ptr(), B, d, theta.data_ptr(), float(shift),
                              L.PRECISIONS[precision], g.data_ptr(), _stream()), 'mfg_score')
    return g


def td_pg_accumulate(pi, pi_next, P, reward, w, theta, shift, gamma_or_discount, G=None, accumulate=False, ws=None,
                     precision='mixed', out=None):
    for t, n in ((pi, 'pi'), (pi_next, 'pi_next'), (P, 'P'), (reward, 'reward')):
        _chk_f32(t, n)
    _chk_f64(w, 'w'); _chk_f64(theta, 'theta')
    B, d = pi.shape
    F = num_features(d)
    if out is not None:
        delta, g = out
    else:
        delta = torch.empty(B, dtype=torch.float64, device=pi.device)
        g = torch.empty(B, dtype=torch.float64, device=pi.device)
    if G is None:
        G = torch.zeros(F + 3, dtype=torch.float64, device=pi.device)
    if ws is None:
        ws = workspace(B, d, pi.device)
    L.check(L.lib().mfg_td_pg_accumulate(pi.data_ptr(), pi_next.data_ptr(), P.data_ptr(), reward.data_ptr(),
                                         w.data_ptr(), theta.data_ptr(), float(shift), float(gamma_or_discount),
                                         B, d, L.PRECISIONS[precision], delta.data_ptr(), g.data_ptr(), G.data_ptr(),
                                         int(accumulate),
                                         ws.data_ptr(), ws.numel() * 8, _stream()), 'mfg_td_pg_accumulate')
    return delta, g, G


def apply_update(G, d, lr_critic, lr_actor, w, theta, reward_acc=None):
    """w, theta update from the batch sums; reward_acc (fp64 device scalar / 1-element view) += mean reward."""
    _chk_f64(G, 'G'); _chk_f64(w, 'w'); _chk_f64(theta, 'theta')
    L.check(L.lib().mfg_apply_update(G.data_ptr(), d, float(lr_critic), float(lr_actor), w.data_ptr(),
                                     theta.data_ptr(), _ptr(reward_acc), _stream()), 'mfg_apply_update')


def rollout(pi0, T, theta, shift, alpha_scale, w=None, gamma=1.0, reward_kind=L.REWARD_MFG_AC2, seed=0,
            first_step=0, traj_offset=0, td=True, write_P=False, discount_pow=False, G=None, accumulate=False,
            ws=None, out=None, precision='mixed'):
    """Fused T-step rollout.  Returns dict(pi_traj, pi_last, reward, delta, g, P, G)."""
    _chk_f32(pi0, 'pi0'); _chk_f64(theta, 'theta')
    B, d = pi0.shape
    dev = pi0.device
    o = out or {}
    pi_traj = o.get('pi_traj') if 'pi_traj' in o else torch.empty(B, T + 1, d, dtype=torch.float32, device=dev)
    pi_last = o.get('pi_last') if 'pi_last' in o else torch.empty(B, d, dtype=torch.float32, device=dev)
    ext = int(reward_kind) == L.REWARD_EXTERNAL
    if ext and G is not None:
        raise ValueError('external reward: the batch sums need the reward; call grad_accumulate(add_reward=True) afterwards')
    reward = None if ext else (o.get('reward') if 'reward' in o else torch.empty(B, T, dtype=torch.float32, device=dev))
    delta = g = None
    flags = 0
    if td:
        _chk_f64(w, 'w')
        flags |= L.ROLLOUT_TD
        delta = o.get('delta') if 'delta' in o else torch.empty(B, T, dtype=torch.float64, device=dev)
        g = o.get('g') if 'g' in o else torch.empty(B, T, dtype=torch.float64, device=dev)
        if not ext:
            if G is None:
                G = torch.zeros(num_features(d) + 3, dtype=torch.float64, device=dev)
            if ws is None:
                ws = workspace(B * T, d, dev)
    P = None
    if write_P:
        flags |= L.ROLLOUT_WRITE_P
        P = o.get('P') if 'P' in o else torch.empty(B, T, d, d, dtype=torch.float32, device=dev)
    flags |= _rollout_flags(discount_pow, precision)
    L.check(L.lib().mfg_rollout(pi0.data_ptr(), B, d, T, theta.data_ptr(), float(shift), float(alpha_scale),
                                _ptr(w) if td else None, float(gamma), int(reward_kind), int(seed), int(first_step),
                                int(traj_offset), flags, pi_traj.data_ptr(), _ptr(pi_last), _ptr(reward), _ptr(delta),
                                _ptr(g),
                                _ptr(P), _ptr(G) if (td and not ext) else None, int(accumulate),
                                _ptr(ws) if (td and not ext) else None,
                                ws.numel() * 8 if (td and not ext and ws is not None) else 0, _stream()), 'mfg_rollout')
    return {'pi_traj': pi_traj, 'pi_last': pi_last, 'reward': reward, 'delta': delta, 'g': g, 'P': P, 'G': G}


def train_rollout(mat_pi0, idx, T, theta, shift, alpha_scale, w, gamma, G, ws, bufs, lr_critic=0.0, lr_actor=0.0,
                  apply=False, reward_kind=L.REWARD_MFG_AC2, seed=0, first_step=0, traj_offset=0, discount_pow=False,
                  reward_acc=None, precision='mixed'):
    """One training update per episode: start-state gather (inside the kernel) + fused T-step TD rollout + batch sums
    [+ parameter update when apply=True (single GPU)].  bufs = dict(pi_traj [B,T+1,d], pi_last [B,d] | None,
    reward [B,T], delta [B,T], g [B,T]).  idx=None: the start rows are drawn inside the rollout kernel."""
    _chk_f32(mat_pi0, 'mat_pi0'); _chk_f64(theta, 'theta'); _chk_f64(w, 'w'); _chk_f64(G, 'G')
    if idx is not None and (idx.dtype != torch.int32 or not idx.is_cuda):
        raise ValueError('idx must be an int32 CUDA tensor (or None: start states drawn in the kernel)')
    B, d = bufs['pi_traj'].shape[0], mat_pi0.shape[1]
    if idx is not None and idx.numel() != B:
        raise ValueError('idx must have one entry per trajectory of the buffers')
    flags = _rollout_flags(discount_pow, precision) | (L.TRAIN_APPLY if apply else 0)
    L.check(L.lib().mfg_train_rollout(mat_pi0.data_ptr(), mat_pi0.shape[0], _ptr(idx), B, d, int(T), theta.data_ptr(),
                                      float(shift), float(alpha_scale), w.data_ptr(), float(gamma), int(reward_kind),
                                      int(seed), int(first_step), int(traj_offset), flags, float(lr_critic),
                                      float(lr_actor), bufs['pi_traj'].data_ptr(), _ptr(bufs.get('pi_last')),
                                      bufs['reward'].data_ptr(), bufs['delta'].data_ptr(), bufs['g'].data_ptr(),
                                      G.data_ptr(), _ptr(reward_acc), ws.data_ptr(), ws.numel() * 8, _stream()),
            'mfg_train_rollout')
    return bufs


def train_rollout_deferred(mat_pi0, idx, T, theta, w, pending, theta_out, w_out, shift, alpha_scale, gamma, G, ws, bufs,
                           reward_kind=L.REWARD_MFG_AC2, seed=0, first_step=0, traj_offset=0, discount_pow=False,
                           precision='mixed'):
    """Multi-rank update cycle without an update launch (mfg_train_rollout_deferred): `pending` = None or
    (G_all_reduced, lr_critic, lr_actor, reward_acc) of the PREVIOUS update, applied while this rollout stages its weights;
    the updated parameters land in (theta_out, w_out) -- other tensors than (theta, w).  G = this rank's sums afterwards."""
    _chk_f32(mat_pi0, 'mat_pi0'); _chk_f64(theta, 'theta'); _chk_f64(w, 'w'); _chk_f64(G, 'G')
    B, d = bufs['pi_traj'].shape[0], mat_pi0.shape[1]
    flags = _rollout_flags(discount_pow, precision)
    pG, plc, pla, pacc = pending if pending is not None else (None, 0.0, 0.0, None)
    L.check(L.lib().mfg_train_rollout_deferred(mat_pi0.data_ptr(), mat_pi0.shape[0], _ptr(idx), B, d, int(T), theta.data_ptr(),
                                               w.data_ptr(), _ptr(pG), float(plc), float(pla), _ptr(pacc), _ptr(theta_out),
                                               _ptr(w_out), float(shift), float(alpha_scale), float(gamma), int(reward_kind),
                                               int(seed), int(first_step), int(traj_offset), flags, bufs['pi_traj'].data_ptr(),
                                               _ptr(bufs.get('pi_last')), bufs['reward'].data_ptr(), bufs['delta'].data_ptr(),
                                               bufs['g'].data_ptr(), G.data_ptr(), ws.data_ptr(), ws.numel() * 8, _stream()),
            'mfg_train_rollout_deferred')
    return bufs


def train_rollouts(mat_pi0, T, episodes, first_episode, constant, theta, shift, alpha_scale, w, gamma, G, ws, bufs, lr_critic,
                   lr_actor, reward_kind=L.REWARD_MFG_AC2, seed=0, first_step=0, traj_offset=0, discount_pow=False,
                   reward_acc=None, precision='mixed'):
    """`episodes` training updates (one per episode) issued back to back by native code: start states drawn in the kernel,
    fused T-step rollout, batch sums, update with the reference's learning-rate schedule in episode numbers
    first_episode, first_episode + 1, ...  reward_acc: fp64 device array [episodes] (or an address), entry k += mean reward
    of episode k's update."""
    _chk_f32(mat_pi0, 'mat_pi0'); _chk_f64(theta, 'theta'); _chk_f64(w, 'w'); _chk_f64(G, 'G')
    B, d = bufs['pi_traj'].shape[0], mat_pi0.shape[1]
    flags = _rollout_flags(discount_pow, precision)
    L.check(L.lib().mfg_train_rollouts(mat_pi0.data_ptr(), mat_pi0.shape[0], B, d, int(T), int(episodes), int(first_episode),
                                       int(bool(constant)), theta.data_ptr(), float(shift), float(alpha_scale), w.data_ptr(),
                                       float(gamma), int(reward_kind), int(seed), int(first_step), int(traj_offset), flags,
                                       float(lr_critic), float(lr_actor), bufs['pi_traj'].data_ptr(), _ptr(bufs.get('pi_last')),
                                       bufs['reward'].data_ptr(), bufs['delta'].data_ptr(), bufs['g'].data_ptr(), G.data_ptr(),
                                       _ptr(reward_acc), ws.data_ptr(), ws.numel() * 8, _stream()), 'mfg_train_rollouts')
    return bufs


def train_rollouts_dist(comm, mat_pi0, T, episodes, first_episode, constant, theta, w, theta_alt, w_alt, shift, alpha_scale, gamma, G,
                        ws, bufs, lr_critic, lr_actor, reward_kind=L.REWARD_MFG_AC2, seed=0, first_step=0, traj_offset=0,
                        discount_pow=False, reward_acc=None, precision='mixed'):
    """`episodes` multi-GPU training updates issued natively (mfg_train_rollouts_dist): per episode the rollout kernel
    (previous update applied in its weight staging, start states drawn in the kernel), the batch sums and ONE RCCL all-reduce
    of G from the library itself; the last update is applied before returning, parameters end up in (theta, w).
    comm: address of a communicator from parallel.native_comm()."""
    _chk_f32(mat_pi0, 'mat_pi0'); _chk_f64(theta, 'theta'); _chk_f64(w, 'w'); _chk_f64(theta_alt, 'theta_alt'); _chk_f64(w_alt, 'w_alt')
    _chk_f64(G, 'G')
    B, d = bufs['pi_traj'].shape[0], mat_pi0.shape[1]
    flags = _rollout_flags(discount_pow, precision)
    L.check(L.lib().mfg_train_rollouts_dist(comm, mat_pi0.data_ptr(), mat_pi0.shape[0], B, d, int(T), int(episodes), int(first_episode),
                                            int(bool(constant)), theta.data_ptr(), w.data_ptr(), theta_alt.data_ptr(),
                                            w_alt.data_ptr(), float(shift), float(alpha_scale), float(gamma), int(reward_kind),
                                            int(seed), int(first_step), int(traj_offset), flags, float(lr_critic), float(lr_actor),
                                            bufs['pi_traj'].data_ptr(), _ptr(bufs.get('pi_last')), bufs['reward'].data_ptr(),
                                            bufs['delta'].data_ptr(), bufs['g'].data_ptr(), G.data_ptr(), _ptr(reward_acc),
                                            ws.data_ptr(), ws.numel() * 8, _stream()), 'mfg_train_rollouts_dist')
    return bufs


def grad_accumulate(pi, delta, g, reward, G, ws, T=1, stride_b=None, add_reward=False, accumulate=False):
    """Batch sums G (+)= [sum delta phi | sum delta g | sum r | N] over B*T samples; add_reward: delta += reward first
    (in place) -- the IRL step after the reward network has run."""
    d = pi.shape[-1]
    B = delta.numel() // T
    if stride_b is None:
        stride_b = (T + 1) * d if (pi.dim() == 3 and pi.shape[1] == T + 1) else T * d
    L.check(L.lib().mfg_grad_accumulate(pi.data_ptr(), int(stride_b), delta.data_ptr(), _ptr(g), _ptr(reward), B, int(T), d,
                                        int(bool(add_reward)), G.data_ptr(), int(bool(accumulate)), ws.data_ptr(),
                                        ws.numel() * 8, _stream()), 'mfg_grad_accumulate')
    return G


def grad_apply(pi, delta, g, reward, G, ws, lr_critic, lr_actor, w, theta, reward_acc=None, T=1, stride_b=None,
               add_reward=False):
    """grad_accumulate + apply_update in one call (single GPU): the update rides in the kernel that finishes the sums."""
    d = pi.shape[-1]
    B = delta.numel() // T
    if stride_b is None:
        stride_b = (T + 1) * d if (pi.dim() == 3 and pi.shape[1] == T + 1) else T * d
    L.check(L.lib().mfg_grad_apply(pi.data_ptr(), int(stride_b), delta.data_ptr(), _ptr(g), _ptr(reward), B, int(T), d,
                                   int(bool(add_reward)), G.data_ptr(), float(lr_critic), float(lr_actor), w.data_ptr(),
                                   theta.data_ptr(), _ptr(reward_acc), ws.data_ptr(), ws.numel() * 8, _stream()),
            'mfg_grad_apply')
    return G


def train_episode(pi, T, theta, shift, alpha_scale, w, gamma, lr_critic, lr_actor, G, ws, bufs, reward_kind=L.REWARD_MFG_AC2,
                  seed=0, first_step=0, traj_offset=0, reward_acc=None, precision='mixed'):
    """T env steps with the reference's per-step parameter updates, issued natively (single GPU).  `pi` [B,d] is
    updated in place to the final states; `bufs` = dict(scratch[B,d] f32, reward[B] f32, delta[B] f64, g[B] f64)."""
    _chk_f32(pi, 'pi'); _chk_f64(theta, 'theta'); _chk_f64(w, 'w')
    B, d = pi.shape
    L.check(L.lib().mfg_train_episode(pi.data_ptr(), bufs['scratch'].data_ptr(), B, d, int(T), theta.data_ptr(),
                                      float(shift), float(alpha_scale), w.data_ptr(), float(gamma), int(reward_kind),
                                      int(seed), int(first_step), int(traj_offset), L.PRECISIONS[precision],
                                      float(lr_critic), float(lr_actor), bufs['reward'].data_ptr(),
                                      bufs['delta'].data_ptr(), bufs['g'].data_ptr(), G.data_ptr(), _ptr(reward_acc),
                                      ws.data_ptr(), ws.numel() * 8, _stream()), 'mfg_train_episode')
    return pi


def train_episodes(mat_pi0, pi, T, episodes, first_episode, constant, theta, shift, alpha_scale, w, gamma, lr_critic, lr_actor,
                   G, ws, bufs, reward_kind=L.REWARD_MFG_AC2, seed=0, first_step=0, traj_offset=0, reward_acc=None,
                   precision='mixed'):
    """`episodes` x [start states drawn on the device into `pi` | T env steps with per-step updates], issued natively
    (single GPU); learning rates per episode as in train_rollouts.  `pi` [B,d] holds the last episode's final states."""
    _chk_f32(mat_pi0, 'mat_pi0'); _chk_f32(pi, 'pi'); _chk_f64(theta, 'theta'); _chk_f64(w, 'w')
    B, d = pi.shape
    L.check(L.lib().mfg_train_episodes(mat_pi0.data_ptr(), mat_pi0.shape[0], pi.data_ptr(), bufs['scratch'].data_ptr(), B, d,
                                       int(T), int(episodes), int(first_episode), int(bool(constant)), theta.data_ptr(),
                                       float(shift), float(alpha_scale), w.data_ptr(), float(gamma), int(reward_kind), int(seed),
                                       int(first_step), int(traj_offset), L.PRECISIONS[precision], float(lr_critic),
                                       float(lr_actor), bufs['reward'].data_ptr(), bufs['delta'].data_ptr(),
                                       bufs['g'].data_ptr(), G.data_ptr(), _ptr(reward_acc), ws.data_ptr(), ws.numel() * 8,
                                       _stream()), 'mfg_train_episodes')
    return pi


def pop_workspace_slice(B, d, T):
    """Bytes of ONE learner's workspace slice for every population flow (in-kernel and IRL rewards, step and rollout mode):
    what the single-learner calls get for B T samples (ops.workspace), rounded up to 256."""
    return (max(int(L.lib().mfg_workspace_bytes(B * T, d)), 8) + 255) // 256 * 256


irl_pop_workspace_slice = pop_workspace_slice   # (its name in the IRL population calls' API)


def _chk_pop(K, name, t, dtype):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dtype and t.is_contiguous() and t.numel() == K):
        raise ValueError('%s: expected a contiguous %s device tensor of %d entries (one per learner)' % (name, dtype, K))


def _chk_pop_args(K, B, d, T, episodes, theta, w, G, ws, bufs, reward_acc, mat_pi0, shifts, alpha_scales, lr_critic, lr_actor,
                  seeds, rn_seeds=None):
    """The per-learner arrays [K] and the shapes of the learner-major arrays of a population training call: an undersized
    one would be written past its end."""
    for name, t in (('shifts', shifts), ('alpha_scales', alpha_scales), ('lr_critic', lr_critic), ('lr_actor', lr_actor)):
        _chk_pop(K, name, t, torch.float64)
    _chk_pop(K, 'seeds', seeds, torch.int64)
    if rn_seeds is not None:
        _chk_pop(K, 'rn_seeds', rn_seeds, torch.int64)
    F = num_features(d)
    want = dict(theta=(theta, (K,)), w=(w, (K, F)), G=(G, (K, F + 3)))
    for key, t in bufs.items():
        if t is None:
            continue
        shape = {'pi': (K, B, d), 'scratch': (K, B, d), 'pi_traj': (K, B, T + 1, d), 'pi_last': (K, B, d)}.get(key)
        if shape is None:
            shape = (K, B) if 'scratch' in bufs else (K, B, T)
        want[key] = (t, shape)
    if reward_acc is not None:
        if not isinstance(reward_acc, torch.Tensor):
            raise ValueError('reward_acc: expected a [K, episodes] fp64 device tensor or None')
        want['reward_acc'] = (reward_acc, (K, max(int(episodes), 0)))
    for name, (t, shape) in want.items():
        if tuple(t.shape) != shape or not t.is_contiguous() or not t.is_cuda:
            raise ValueError('%s: expected a contiguous device tensor of shape %s, got %s' % (name, shape, tuple(t.shape)))
    if mat_pi0.dim() != 2 or mat_pi0.shape[1] != d:
        raise ValueError('mat_pi0: expected [num_start, %d]' % d)
    if ws.dim() != 2 or ws.shape[0] != K or not ws.is_contiguous() or ws.dtype != torch.float64:
        raise ValueError('ws: expected a contiguous fp64 [K, slice] workspace')


def _train_episodes_pop(entry, mat_pi0, pi, T, episodes, first_episode, constant, theta, shifts, alpha_scales, w, gamma,
                        lr_critic, lr_actor, seeds, G, ws, bufs, reward_kind, first_step, traj_offset, reward_acc, precision):
    """The step-mode population call `entry` (mfg_train_episodes_pop or its resident form: one parameter list)."""
    _chk_f32(mat_pi0, 'mat_pi0'); _chk_f32(pi, 'pi'); _chk_f64(theta, 'theta'); _chk_f64(w, 'w'); _chk_f64(G, 'G')
    K, B, d = pi.shape
    bufs = dict(bufs, pi=pi)
    _chk_pop_args(K, B, d, T, episodes, theta, w, G, ws, bufs, reward_acc, mat_pi0, shifts, alpha_scales, lr_critic, lr_actor,
                  seeds)
    fn = getattr(L.lib(), entry)
    L.check(fn(mat_pi0.data_ptr(), mat_pi0.shape[0], pi.data_ptr(), bufs['scratch'].data_ptr(), B, K, d, int(T), int(episodes),
               int(first_episode), int(bool(constant)), theta.data_ptr(), shifts.data_ptr(), alpha_scales.data_ptr(),
               w.data_ptr(), float(gamma), int(reward_kind), seeds.data_ptr(), int(first_step), int(traj_offset),
               L.PRECISIONS[precision], lr_critic.data_ptr(), lr_actor.data_ptr(), bufs['reward'].data_ptr(),
               bufs['delta'].data_ptr(), bufs['g'].data_ptr(), G.data_ptr(), _ptr(reward_acc), ws.data_ptr(),
               ws.shape[1] * ws.element_size(), _stream()), entry)
    return pi


def train_episodes_pop(mat_pi0, pi, T, episodes, first_episode, constant, theta, shifts, alpha_scales, w, gamma, lr_critic,
                       lr_actor, seeds, G, ws, bufs, reward_kind=L.REWARD_MFG_AC2, first_step=0, traj_offset=0, reward_acc=None,
                       precision='mixed'):
    """train_episodes for a population of K independent learners in the launches of one (mfg_train_episodes_pop): `pi`
    [K,Bk,d], theta [K], w [K,F], G [K,F+3], ws [K, slice] fp64 (one learner's slice per row); shifts, alpha_scales,
    lr_critic, lr_actor fp64 and seeds int64 (read as uint64) device arrays [K]; bufs = dict(scratch [K,Bk,d] f32,
    reward [K,Bk] f32, delta / g [K,Bk] f64); reward_acc [K,episodes] fp64 or None."""
    return _train_episodes_pop('mfg_train_episodes_pop', mat_pi0, pi, T, episodes, first_episode, constant, theta, shifts,
                               alpha_scales, w, gamma, lr_critic, lr_actor, seeds, G, ws, bufs, reward_kind, first_step,
                               traj_offset, reward_acc, precision)


def train_episodes_pop_resident(mat_pi0, pi, T, episodes, first_episode, constant, theta, shifts, alpha_scales, w, gamma,
                                lr_critic, lr_actor, seeds, G, ws, bufs, reward_kind=L.REWARD_MFG_AC2, first_step=0, traj_offset=0,
                                reward_acc=None, precision='mixed'):
    """train_episodes_pop with every learner resident in one workgroup (mfg_train_episodes_pop_resident): the same arguments
    and, bit for bit, the same outputs, in ceil(episodes / 64) launches instead of episodes x (1 + 2 T).  For learners of few
    trajectories (mfg_pop_resident_supported, include/mfg_hip.h); MfgError (MFG_EUNSUPPORTED) for another shape or under a
    population control block."""
    return _train_episodes_pop('mfg_train_episodes_pop_resident', mat_pi0, pi, T, episodes, first_episode, constant, theta,
                               shifts, alpha_scales, w, gamma, lr_critic, lr_actor, seeds, G, ws, bufs, reward_kind, first_step,
                               traj_offset, reward_acc, precision)


def train_rollouts_pop(mat_pi0, T, episodes, first_episode, constant, theta, shifts, alpha_scales, w, gamma, G, ws, bufs,
                       lr_critic, lr_actor, seeds, reward_kind=L.REWARD_MFG_AC2, first_step=0, traj_offset=0, discount_pow=False,
                       reward_acc=None, precision='mixed'):
    """train_rollouts for a population of K independent learners (mfg_train_rollouts_pop): bufs = dict(pi_traj
    [K,Bk,T+1,d] f32, pi_last [K,Bk,d] f32 (optional), reward [K,Bk,T] f32, delta / g [K,Bk,T] f64); the other arrays as
    for train_episodes_pop."""
    _chk_f32(mat_pi0, 'mat_pi0'); _chk_f64(theta, 'theta'); _chk_f64(w, 'w'); _chk_f64(G, 'G')
    K, B, d = bufs['pi_traj'].shape[0], bufs['pi_traj'].shape[1], mat_pi0.shape[1]
    _chk_pop_args(K, B, d, T, episodes, theta, w, G, ws, bufs, reward_acc, mat_pi0, shifts, alpha_scales, lr_critic, lr_actor,
                  seeds)
    flags = _rollout_flags(discount_pow, precision)
    L.check(L.lib().mfg_train_rollouts_pop(mat_pi0.data_ptr(), mat_pi0.shape[0], B, K, d, int(T), int(episodes),
                                           int(first_episode), int(bool(constant)), theta.data_ptr(), shifts.data_ptr(),
                                           alpha_scales.data_ptr(), w.data_ptr(), float(gamma), int(reward_kind),
                                           seeds.data_ptr(), int(first_step), int(traj_offset), flags, lr_critic.data_ptr(),
                                           lr_actor.data_ptr(), bufs['pi_traj'].data_ptr(), _ptr(bufs.get('pi_last')),
                                           bufs['reward'].data_ptr(), bufs['delta'].data_ptr(), bufs['g'].data_ptr(),
                                           G.data_ptr(), _ptr(reward_acc), ws.data_ptr(), ws.shape[1] * ws.element_size(),
                                           _stream()), 'mfg_train_rollouts_pop')
    return bufs


def reward_net_struct(net, dropout=None):
    """mfg_reward_net_t for a networks.RewardNet (device pointers of its parameters; keep the module alive while in use)."""
    if dropout is None:
        dropout = net.use_dropout and (net.dropout_always or net.training)
    st = L.RewardNetStruct()
    st.k1, st.f2, st.k2 = net.conv1.kernel_size[0], net.conv2.out_channels, net.conv2.kernel_size[0]
    st.n3, st.n4 = net.fc3.out_features, net.fc4.out_features
    for name, t in (('conv1_w', net.conv1.weight), ('conv1_b', net.conv1.bias), ('conv2_w', net.conv2.weight),
                    ('conv2_b', net.conv2.bias), ('fc3_w', net.fc3.weight), ('fc3_b', net.fc3.bias), ('fc4_w', net.fc4.weight),
                    ('fc4_b', net.fc4.bias), ('out_w', net.out.weight), ('out_b', net.out.bias)):
        if not t.is_contiguous():
            raise ValueError('reward net parameters must be contiguous')
        setattr(st, name, t.data_ptr())
    st.keep_prob = float(net.keep_prob) if dropout else 1.0
    return st


def train_episode_irl(pi, T, theta, shift, alpha_scale, w, gamma, lr_critic, lr_actor, net, G, ws, bufs, seed=0, first_step=0,
                      traj_offset=0, rn_seed=0, rn_call0=0, rn_sample_offset=0, reward_acc=None, precision='mixed', mat_pi0=None):
    """T env steps of AC_IRL.train with per-step updates, issued natively (single GPU): sample + transition + score,
    reward network, batch sums + update per step.  `pi` [B,d] is updated in place to the final states; `bufs` =
    dict(scratch [B,d] f32, P [B,d,d] f32, reward [B] f32, delta [B] f64, g [B] f64); `net` = networks.RewardNet.
    mat_pi0 [num_start,d]: the start states are drawn from this table inside the call (the draw of draw_start at step =
    first_step; `pi` is then an output only)."""
    import ctypes as C
    _chk_f32(pi, 'pi'); _chk_f64(theta, 'theta'); _chk_f64(w, 'w')
    B, d = pi.shape
    st = reward_net_struct(net)
    rest = (pi.data_ptr(), bufs['scratch'].data_ptr(), B, d, int(T), theta.data_ptr(), float(shift), float(alpha_scale),
            w.data_ptr(), float(gamma), int(seed), int(first_step), int(traj_offset), L.PRECISIONS[precision], float(lr_critic),
            float(lr_actor), C.byref(st), int(rn_seed) & 0xFFFFFFFFFFFFFFFF, int(rn_call0), int(rn_sample_offset),
            bufs['P'].data_ptr(), bufs['reward'].data_ptr(), bufs['delta'].data_ptr(), bufs['g'].data_ptr(), G.data_ptr(),
            _ptr(reward_acc), ws.data_ptr(), ws.numel() * 8, _stream())
    if mat_pi0 is None:
        L.check(L.lib().mfg_train_episode_irl(*rest), 'mfg_train_episode_irl')
    else:
        _chk_f32(mat_pi0, 'mat_pi0')
        if mat_pi0.dim() != 2 or mat_pi0.shape[1] != d:
            raise ValueError('train_episode_irl: mat_pi0 must be [num_start, %d]' % d)
        L.check(L.lib().mfg_train_episode_irl_draw(mat_pi0.data_ptr(), int(mat_pi0.shape[0]), *rest), 'mfg_train_episode_irl_draw')
    return pi


def train_rollout_irl(mat_pi0, idx, T, theta, shift, alpha_scale, w, gamma, lr_critic, lr_actor, net, G, ws, bufs, seed=0,
                      first_step=0, traj_offset=0, rn_key=0, rn_sample_offset=0, reward_acc=None, discount_pow=True, apply=True,
                      precision='mixed'):
    """One IRL update per episode issued natively (mfg_train_rollout_irl): fused rollout (start states drawn in the kernel when
    idx is None) | reward network over all B*T transitions | batch sums + update.  bufs: pi_traj [B,T+1,d], pi_last [B,d],
    P [B,T,d,d], reward [B*T] f32, delta / g [B*T] f64."""
    import ctypes as C
    _chk_f32(mat_pi0, 'mat_pi0'); _chk_f64(theta, 'theta'); _chk_f64(w, 'w'); _chk_f64(G, 'G')
    B, d = bufs['pi_traj'].shape[0], mat_pi0.shape[1]
    flags = _rollout_flags(discount_pow, precision) | (L.TRAIN_APPLY if apply else 0)
    st = reward_net_struct(net)
    L.check(L.lib().mfg_train_rollout_irl(mat_pi0.data_ptr(), mat_pi0.shape[0], _ptr(idx), B, d, int(T), theta.data_ptr(),
                                          float(shift), float(alpha_scale), w.data_ptr(), float(gamma), int(seed), int(first_step),
                                          int(traj_offset), flags, float(lr_critic), float(lr_actor), C.byref(st),
                                          int(rn_key) & 0xFFFFFFFFFFFFFFFF, int(rn_sample_offset), bufs['pi_traj'].data_ptr(),
                                          bufs['pi_last'].data_ptr(), bufs['P'].data_ptr(), bufs['reward'].data_ptr(),
                                          bufs['delta'].data_ptr(), bufs['g'].data_ptr(), G.data_ptr(), _ptr(reward_acc),
                                          ws.data_ptr(), ws.numel() * 8, _stream()), 'mfg_train_rollout_irl')
    return bufs


IRL_POP_D = (15, 21)     # the matrix-core reward-network kernel's sizes (mfg_train_*_irl_pop)
IRL_POP_MAX_FC3 = 16


def _irl_pop_net_shape(n):
    """((d, f1, k1, f2, k2, n_fc3, n_fc4), keep_prob in effect) of a networks.RewardNet."""
    keep = float(n.keep_prob) if (n.use_dropout and (n.dropout_always or n.training)) else 1.0
    return (n.d, n.conv1.out_channels, n.conv1.kernel_size[0], n.conv2.out_channels, n.conv2.kernel_size[0],
            n.fc3.out_features, n.fc4.out_features), keep


def irl_pop_net_geometries(nets):
    """(d, [(n_fc3, n_fc4, keep_prob, l1l2), ...]) of the networks.RewardNet modules `nets`, one entry per network: what a
    population with a per-learner geometry table (mfg_rn_geom_t) reads.  d, k1 = 5, f2 = 2, k2 = 3 are shared; ValueError where
    they differ or an entry is outside the matrix-core kernel (d = 15 / 21, n_fc3 <= 16, n_fc4 <= 32, keep_prob in (0, 1])."""
    if not nets:
        raise ValueError('no reward network')
    d0, out = nets[0].d, []
    for n in nets:
        (d, f1, k1, f2, k2, n3, n4), keep = _irl_pop_net_shape(n)
        if d != d0:
            raise ValueError('reward networks of one population must share d: %d vs %d' % (d, d0))
        if d not in IRL_POP_D or f1 != 1 or k1 != 5 or f2 != 2 or k2 != 3 or not 1 <= n3 <= IRL_POP_MAX_FC3 or not 1 <= n4 <= 32:
            raise ValueError('reward network d=%d, f1=%d, k1=%d, f2=%d, k2=%d, n_fc3=%d, n_fc4=%d: IRL populations need the '
                             'matrix-core kernel (d = 15 / 21, 1 / 5 / 2 / 3, n_fc3 <= %d, n_fc4 <= 32)'
                             % (d, f1, k1, f2, k2, n3, n4, IRL_POP_MAX_FC3))
        if not 0.0 < keep <= 1.0:
            raise ValueError('reward network keep_prob=%g outside (0, 1]' % keep)
        out.append((n3, n4, keep, bool(n.use_l1l2)))
    return d0, out


def irl_pop_net_geometry(nets):
    """(d, n_fc3, n_fc4, keep_prob) shared by the networks.RewardNet modules `nets`; ValueError where they differ or where the
    matrix-core reward-network kernel does not serve them (d = 15 / 21, k1 = 5, f2 = 2, k2 = 3, n_fc3 <= 16, n_fc4 <= 32)."""
    if not nets:
        raise ValueError('no reward network')
    g0, k0 = _irl_pop_net_shape(nets[0])
    for n in nets[1:]:
        g, k = _irl_pop_net_shape(n)
        if g != g0:
            raise ValueError('reward networks of one population must share their geometry: %s vs %s' % (g, g0))
        if k != k0:
            raise ValueError('reward networks of one population must share their dropout setting: keep %g vs %g' % (k, k0))
    d, ((n3, n4, keep, _),) = irl_pop_net_geometries(nets[:1])      # (all equal: the kernel's limits, checked once)
    return d, n3, n4, keep


RN_GEOM = None           # numpy dtype of mfg_rn_geom_t (L.RnGeomStruct)


def rn_geom_table(geoms, device=None):
    """The geometry table of the IRL population calls from [(n3, n4, keep_prob, l1l2), ...]: (host NumPy array of mfg_rn_geom_t,
    its device copy as a uint8 tensor, or None without a device)."""
    import numpy as np
    global RN_GEOM
    if RN_GEOM is None:
        RN_GEOM = np.dtype(L.RnGeomStruct)
    host = np.zeros(len(geoms), dtype=RN_GEOM)
    for k, (n3, n4, keep, l1l2) in enumerate(geoms):
        host[k] = (int(n3), int(n4), float(keep), int(bool(l1l2)))
    dev = None
    if device is not None:
        dev = torch.from_numpy(host.view(np.uint8).copy()).to(device)
    return host, dev


def _geom_ptrs(geom, K):
    """(host pointer, device pointer) of a table built by rn_geom_table, [K] entries; two NULLs for geom = None."""
    if geom is None:
        return None, None
    host, dev = geom
    if host.shape != (K,) or host.dtype.itemsize != 16 or not host.flags['C_CONTIGUOUS']:
        raise ValueError('geometry table: expected %d contiguous mfg_rn_geom_t entries on the host' % K)
    if dev is None or not dev.is_cuda or not dev.is_contiguous() or dev.numel() * dev.element_size() != 16 * K:
        raise ValueError('geometry table: expected a contiguous device copy of %d bytes' % (16 * K))
    return host.ctypes.data, dev.data_ptr()


def _rn_call0_ptr(rn_call0, K, like):
    """The per-learner reward-call counters [K] (int64 device array); an int counts for every learner."""
    if not isinstance(rn_call0, torch.Tensor):
        rn_call0 = torch.full((K,), int(rn_call0), dtype=torch.int64, device=like.device)
    _chk_pop(K, 'rn_call0', rn_call0, torch.int64)
    return rn_call0


def _chk_irl_pop(K, B, d, T, episodes, theta, w, G, ws, bufs, reward_acc, mat_pi0, per_learner, shifts, alpha_scales,
                 lr_critic, lr_actor, seeds, rn_seeds, net_struct):
    if not 1 <= K <= L.POP_MAX_K:
        raise ValueError('population size %d outside [1, %d]' % (K, L.POP_MAX_K))
    _chk_pop_args(K, B, d, T, episodes, theta, w, G, ws, bufs, reward_acc, mat_pi0, shifts, alpha_scales, lr_critic, lr_actor,
                  seeds, rn_seeds)
    if d not in IRL_POP_D:
        raise ValueError('d=%d: IRL populations cover d = 15 / 21 (the matrix-core reward-network kernel)' % d)
    if net_struct.n3 > IRL_POP_MAX_FC3:
        raise ValueError('n_fc3=%d > %d: outside the matrix-core reward-network kernel' % (net_struct.n3, IRL_POP_MAX_FC3))


def train_episodes_irl_pop(mat_pi0, pi, T, episodes, first_episode, constant, theta, shifts, alpha_scales, w, gamma, lr_critic,
                           lr_actor, seeds, net_struct, per_learner_net, rn_seeds, rn_call0, G, ws, bufs, first_step=0,
                           traj_offset=0, reward_acc=None, precision='mixed', net_stride=0, geom=None):
    """AC_IRL.train's step mode for K independent learners (mfg_train_episodes_irl_pop): `pi` [K,Bk,d] (output: the final
    states), theta [K], w [K,F], G [K,F+3], ws [K, slice] fp64; shifts, alpha_scales, lr_critic, lr_actor fp64 and seeds,
    rn_seeds int64 (read as uint64) device arrays [K]; net_struct = reward_net_struct(...) of the shared network or of the
    stacked parameters (per_learner_net); bufs = dict(scratch [K,Bk,d] f32, P [K,Bk,d,d] f32, reward [K,Bk] f32, delta / g
    [K,Bk] f64); reward_acc [K,episodes] fp64 or None.  The episode numbers of the schedule start at first_episode.
    rn_call0: the reward calls made before, an int64 device array [K] of per-learner counters or an int for all of them;
    net_stride: elements between two learners' weights in one flat buffer (0: stacked tensors).  geom: a per-learner geometry
    table (rn_geom_table); needs net_stride > 0 and net_struct.conv1_w as the base of learner 0's flat row."""
    import ctypes as C
    _chk_f32(mat_pi0, 'mat_pi0'); _chk_f32(pi, 'pi'); _chk_f64(theta, 'theta'); _chk_f64(w, 'w'); _chk_f64(G, 'G')
    if pi.dim() != 3:
        raise ValueError('pi: expected [K, Bk, d]')
    K, B, d = pi.shape
    P = bufs['P']
    _chk_irl_pop(K, B, d, T, episodes, theta, w, G, ws, dict(bufs, pi=pi, P=None), reward_acc, mat_pi0, per_learner_net,
                 shifts, alpha_scales, lr_critic, lr_actor, seeds, rn_seeds, net_struct)
    if tuple(P.shape) != (K, B, d, d) or not P.is_contiguous() or not P.is_cuda or P.dtype != torch.float32:
        raise ValueError('P: expected a contiguous f32 device tensor [%d, %d, %d, %d]' % (K, B, d, d))
    calls = _rn_call0_ptr(rn_call0, K, theta)
    L.check(L.lib().mfg_train_episodes_irl_pop(
        mat_pi0.data_ptr(), mat_pi0.shape[0], pi.data_ptr(), bufs['scratch'].data_ptr(), B, K, d, int(T), int(episodes),
        int(first_episode), int(bool(constant)), theta.data_ptr(), shifts.data_ptr(), alpha_scales.data_ptr(), w.data_ptr(),
        float(gamma), seeds.data_ptr(), int(first_step), int(traj_offset), L.PRECISIONS[precision], lr_critic.data_ptr(),
        lr_actor.data_ptr(), C.byref(net_struct), int(bool(per_learner_net)), int(net_stride), *_geom_ptrs(geom, K),
        rn_seeds.data_ptr(), calls.data_ptr(), P.data_ptr(), bufs['reward'].data_ptr(), bufs['delta'].data_ptr(),
        bufs['g'].data_ptr(), G.data_ptr(), _ptr(reward_acc), ws.data_ptr(), ws.shape[1] * ws.element_size(), _stream()),
        'mfg_train_episodes_irl_pop')
    return pi


def train_rollouts_irl_pop(mat_pi0, T, episodes, first_episode, constant, theta, shifts, alpha_scales, w, gamma, lr_critic,
                           lr_actor, seeds, net_struct, per_learner_net, rn_seeds, rn_call0, G, ws, bufs, first_step=0,
                           traj_offset=0, discount_pow=True, reward_acc=None, precision='mixed', net_stride=0, geom=None):
    """AC_IRL.train's rollout mode for K independent learners (mfg_train_rollouts_irl_pop): bufs = dict(pi_traj
    [K,Bk,T+1,d] f32, pi_last [K,Bk,d] f32 (optional), P [K,Bk,T,d,d] f32, reward [K,Bk,T] f32, delta / g [K,Bk,T] f64);
    the other arrays, rn_call0, net_stride and geom as for train_episodes_irl_pop."""
    import ctypes as C
    _chk_f32(mat_pi0, 'mat_pi0'); _chk_f64(theta, 'theta'); _chk_f64(w, 'w'); _chk_f64(G, 'G')
    if bufs['pi_traj'].dim() != 4:
        raise ValueError('pi_traj: expected [K, Bk, T+1, d]')
    K, B, d = bufs['pi_traj'].shape[0], bufs['pi_traj'].shape[1], mat_pi0.shape[1]
    P = bufs['P']
    _chk_irl_pop(K, B, d, T, episodes, theta, w, G, ws, dict(bufs, P=None), reward_acc, mat_pi0, per_learner_net, shifts,
                 alpha_scales, lr_critic, lr_actor, seeds, rn_seeds, net_struct)
    if tuple(P.shape) != (K, B, T, d, d) or not P.is_contiguous() or not P.is_cuda or P.dtype != torch.float32:
        raise ValueError('P: expected a contiguous f32 device tensor [%d, %d, %d, %d, %d]' % (K, B, T, d, d))
    flags = _rollout_flags(discount_pow, precision)
    calls = _rn_call0_ptr(rn_call0, K, theta)
    L.check(L.lib().mfg_train_rollouts_irl_pop(
        mat_pi0.data_ptr(), mat_pi0.shape[0], B, K, d, int(T), int(episodes), int(first_episode), int(bool(constant)),
        theta.data_ptr(), shifts.data_ptr(), alpha_scales.data_ptr(), w.data_ptr(), float(gamma), seeds.data_ptr(),
        int(first_step), int(traj_offset), flags, lr_critic.data_ptr(), lr_actor.data_ptr(), C.byref(net_struct),
        int(bool(per_learner_net)), int(net_stride), *_geom_ptrs(geom, K), rn_seeds.data_ptr(), calls.data_ptr(),
        bufs['pi_traj'].data_ptr(), _ptr(bufs.get('pi_last')), P.data_ptr(), bufs['reward'].data_ptr(),
        bufs['delta'].data_ptr(), bufs['g'].data_ptr(), G.data_ptr(), _ptr(reward_acc), ws.data_ptr(),
        ws.shape[1] * ws.element_size(), _stream()), 'mfg_train_rollouts_irl_pop')
    return bufs


def reward_net_forward_pop(net_struct, per_learner_net, K, state, action, learners, keys, out=None, net_stride=0, scratch=None,
                           geom=None):
    """mfg_reward_net_forward_pop: the reward network of the listed learners (distinct, in [0, K)) in one launch.  state [N,d] /
    action [N,d,d] (shared by every learner) or [K,N,d] / [K,N,d,d] (learner k reads row k); keys: the Philox keys of the listed
    learners (Python ints, read as uint64).  Returns out [K,N] f32 (rows of unlisted learners untouched); sample offset 0.
    geom: a per-learner geometry table (rn_geom_table)."""
    import ctypes as C
    import numpy as np
    _chk_f32(state, 'state'); _chk_f32(action, 'action')
    shared = state.dim() == 2
    if shared:
        N, d = state.shape
        if tuple(action.shape) != (N, d, d):
            raise ValueError('action: expected [%d, %d, %d]' % (N, d, d))
    else:
        if state.dim() != 3 or state.shape[0] != K:
            raise ValueError('state: expected [N, d] or [%d, N, d]' % K)
        _, N, d = state.shape
        if tuple(action.shape) != (K, N, d, d):
            raise ValueError('action: expected [%d, %d, %d, %d]' % (K, N, d, d))
    lr = np.ascontiguousarray(learners, dtype=np.int32).reshape(-1)
    ky = np.array([int(k) & 0xFFFFFFFFFFFFFFFF for k in keys], dtype=np.uint64).reshape(-1)
    if ky.shape != lr.shape:
        raise ValueError('one key per listed learner')
    if out is None:
        out = torch.empty(K, N, dtype=torch.float32, device=state.device)
    elif tuple(out.shape) != (K, N):
        raise ValueError('out: expected [%d, %d]' % (K, N))
    _chk_f32(out, 'out')
    if scratch is None:
        scratch = torch.empty(max(2 * lr.size, 2), dtype=torch.float64, device=state.device)
    L.check(L.lib().mfg_reward_net_forward_pop(
        state.data_ptr(), action.data_ptr(), 0 if shared else N * d, 0 if shared else N * d * d, N, d, C.byref(net_struct),
        int(bool(per_learner_net)), int(net_stride), *_geom_ptrs(geom, K), int(K), lr.ctypes.data, ky.ctypes.data, int(lr.size),
        0, out.data_ptr(), scratch.data_ptr(), scratch.numel() * scratch.element_size(), _stream()),
        'mfg_reward_net_forward_pop')
    return out


RN_INPUT_GRAD_OUTPUTS = ('grad_state', 'grad_action', 'mean_state', 'mean_action')


def check_reward_input_grad_args(K, state_shape, action_shape, learners, n_keys, want):
    """The argument check of reward_input_grad_pop (needs no GPU): returns (shared, N, d).  state [N,d] / action [N,d,d] shared by
    every learner, or [K,N,d] / [K,N,d,d]; d = 15 / 21; distinct learners in [0, K), one key each; `want` a non-empty subset of
    RN_INPUT_GRAD_OUTPUTS."""
    if not 1 <= int(K) <= L.POP_MAX_K:
        raise ValueError('population size %d outside [1, %d]' % (K, L.POP_MAX_K))
    state_shape, action_shape = tuple(state_shape), tuple(action_shape)
    shared = len(state_shape) == 2
    if shared:
        N, d = state_shape
        if action_shape != (N, d, d):
            raise ValueError('action: expected [%d, %d, %d], got %s' % (N, d, d, list(action_shape)))
    else:
        if len(state_shape) != 3 or state_shape[0] != K:
            raise ValueError('state: expected [N, d] or [%d, N, d], got %s' % (K, list(state_shape)))
        _, N, d = state_shape
        if action_shape != (K, N, d, d):
            raise ValueError('action: expected [%d, %d, %d, %d], got %s' % (K, N, d, d, list(action_shape)))
    if d not in IRL_POP_D:
        raise ValueError('d=%d: the reward input gradient covers d = 15 / 21 (the matrix-core reward-network geometry)' % d)
    if N < 1:
        raise ValueError('no samples (N < 1)')
    if N >= 1 << 31:
        raise ValueError('N=%d >= 2^31' % N)
    ids = [int(k) for k in learners]
    if any(not 0 <= k < K for k in ids):
        raise ValueError('learner id outside [0, %d)' % K)
    if len(set(ids)) != len(ids):
        raise ValueError('a learner twice in the list')
    if n_keys != len(ids):
        raise ValueError('one key per listed learner')
    want = tuple(want)
    if not want or any(w not in RN_INPUT_GRAD_OUTPUTS for w in want) or len(set(want)) != len(want):
        raise ValueError('want: a non-empty subset of %s, got %s' % (RN_INPUT_GRAD_OUTPUTS, want))
    return shared, int(N), int(d)


def rn_input_grad_workspace_bytes(K, N, d):
    """mfg_rn_input_grad_workspace_bytes: bytes of the workspace of a reward input-gradient block."""
    return int(L.lib().mfg_rn_input_grad_workspace_bytes(int(K), int(N), int(d)))


def _rn_input_grad_shape(name, K, N, d):
    return {'grad_state': (K, N, d), 'grad_action': (K, N, d, d), 'mean_state': (K, 2, d), 'mean_action': (K, 2, d, d)}[name]


def reward_input_grad_pop(net_struct, per_learner_net, K, state, action, learners, keys, out=None, net_stride=0, scratch=None,
                          geom=None, want_samples=False, *, want=None, bufs=None, workspace=None, workspace_bytes=None,
                          ctx=None):
    """reward_net_forward_pop with a reward input-gradient block (mfg_rn_input_grad_t) bound for this call only: the rewards
    and, for the listed learners, d r / d state and d r / d action on every sample and their means (include/mfg_hip.h).  The
    arguments of reward_net_forward_pop; per-learner inputs [K,N,d] / [K,N,d,d] may be views whose learner stride is larger
    than needed.  Returns a dict: reward [K,N] f32, mean_state [K,2,d] / mean_action [K,2,d,d] f64 ([k,0] the mean gradient,
    [k,1] the mean of gradient x input) and, with want_samples, grad_state [K,N,d] / grad_action [K,N,d,d] f32.  Rows of
    learners not in the list are left alone (fresh outputs: NaN).  want: the outputs of the block instead (a subset of
    RN_INPUT_GRAD_OUTPUTS); bufs: tensors to write into, by name; workspace (device tensor) / workspace_bytes: what the block
    announces; ctx: the Context that carries the block (default: the bound one, or one made for the call)."""
    import ctypes as C
    import numpy as np
    if want is None:
        want = ('mean_state', 'mean_action') + (('grad_state', 'grad_action') if want_samples else ())
    lr = np.ascontiguousarray(learners, dtype=np.int32).reshape(-1)
    ky = np.array([int(k) & 0xFFFFFFFFFFFFFFFF for k in keys], dtype=np.uint64).reshape(-1)
    shared, N, d = check_reward_input_grad_args(K, state.shape, action.shape, lr.tolist(), ky.size, want)
    for name, t in (('state', state), ('action', action)):
        inner = t if shared else t[0]
        if not (t.is_cuda and t.dtype == torch.float32 and inner.is_contiguous()):
            raise ValueError('%s must be a float32 CUDA tensor, contiguous within a learner' % name)
    s_state = 0 if shared else int(state.stride(0))
    s_action = 0 if shared else int(action.stride(0))
    if not shared and K > 1 and (s_state < N * d or s_action < N * d * d):
        raise ValueError('per-learner inputs overlap')
    if K == 1 and not shared:
        s_state, s_action = N * d, N * d * d
    dev = state.device
    if out is None:
        out = torch.empty(K, N, dtype=torch.float32, device=dev)
    elif tuple(out.shape) != (K, N):
        raise ValueError('out: expected [%d, %d]' % (K, N))
    _chk_f32(out, 'out')
    if scratch is None:
        scratch = torch.empty(max(2 * lr.size, 2), dtype=torch.float64, device=dev)
    res = {'reward': out}
    for name in want:
        shape, dt = _rn_input_grad_shape(name, K, N, d), (torch.float32 if name.startswith('grad') else torch.float64)
        t = bufs.get(name) if bufs else None
        if t is None:
            t = torch.full(shape, float('nan'), dtype=dt, device=dev)
        elif tuple(t.shape) != shape or t.dtype != dt or not t.is_cuda or not t.is_contiguous():
            raise ValueError('%s: expected a contiguous %s device tensor %s' % (name, dt, list(shape)))
        res[name] = t
    if workspace is None:
        workspace = torch.empty(max(rn_input_grad_workspace_bytes(K, N, d) // 8, 1), dtype=torch.float64, device=dev)
    if workspace_bytes is None:
        workspace_bytes = workspace.numel() * workspace.element_size()
    blk = L.RnInputGradStruct(_ptr(res.get('grad_state')), _ptr(res.get('grad_action')), _ptr(res.get('mean_state')),
                              _ptr(res.get('mean_action')), workspace.data_ptr(), int(workspace_bytes), N, int(K), d, 0)
    lib = L.lib()
    tmp = None
    if ctx is None and lib.mfg_ctx_current() is None:
        ctx = tmp = Context(dev)
    prev = ctx.bind_scoped() if ctx is not None else Context.KEEP
    ptr = lib.mfg_ctx_current()
    try:
        L.check(lib.mfg_ctx_set_rn_input_grad(ptr, C.byref(blk)), 'mfg_ctx_set_rn_input_grad')
        try:
            L.check(lib.mfg_reward_net_forward_pop(
                state.data_ptr(), action.data_ptr(), s_state, s_action, N, d, C.byref(net_struct), int(bool(per_learner_net)),
                int(net_stride), *_geom_ptrs(geom, K), int(K), lr.ctypes.data, ky.ctypes.data, int(lr.size), 0, out.data_ptr(),
                scratch.data_ptr(), scratch.numel() * scratch.element_size(), _stream()), 'mfg_reward_net_forward_pop')
        finally:
            lib.mfg_ctx_set_rn_input_grad(ptr, None)
    finally:
        Context.restore(prev)
        if tmp is not None:
            tmp.close()
    return res


RN_TRAIN_PLAN = None     # numpy dtype of mfg_rn_train_plan_t (L.RnTrainPlan)


def rn_train_plan(n):
    """A zeroed NumPy array of n mfg_rn_train_plan_t entries (fields learner, lr_t, key, lr, adam_step, demo_rows, gen_rows)."""
    import numpy as np
    global RN_TRAIN_PLAN
    if RN_TRAIN_PLAN is None:
        RN_TRAIN_PLAN = np.dtype(L.RnTrainPlan)
    return np.zeros(n, dtype=RN_TRAIN_PLAN)


def reward_net_train_steps_pop(params, m, v, param_stride, K, dims, demo, gen, plan, n_updates, n_active, n_demo, n_gen, steps,
                               demo_divisor, keep_prob, l1l2, stats, ws, plan_dev, beta1=0.9, beta2=0.999, eps=1e-8, geom=None,
                               gen_log_z=None):
    """mfg_reward_net_train_steps_pop: n_updates update_reward steps of n_active learners.  params / m / v [K, param_stride] f32,
    dims = (d, k1, f2, k2, n3, n4), demo = (state [rows,T,d], action [rows,T,d,d]) shared, gen = (state [K,cap,T,d], action
    [K,cap,T,d,d]), plan = rn_train_plan(n_updates * n_active), stats [K,4] f32, ws / plan_dev device byte buffers (uint8).
    geom: a per-learner geometry table (rn_geom_table): n3, n4, keep_prob and l1l2 come from the table (dims[4:], keep_prob and
    l1l2 are not read), rows hold learner k's own layout.
    gen_log_z: fp64 [K, cap], the learners' importance log-weights (traj_log_z_pop) -- the call is then
    mfg_reward_net_train_steps_pop_z; None: the unweighted symbol, as before."""
    for name, t in (('params', params), ('adam_m', m), ('adam_v', v)):
        _chk_f32(t, name)
        if tuple(t.shape) != (K, param_stride):
            raise ValueError('%s: expected [%d, %d]' % (name, K, param_stride))
    _chk_f32(stats, 'stats')
    if tuple(stats.shape) != (K, 4):
        raise ValueError('stats: expected [%d, 4]' % K)
    ds, da = demo
    gs, ga = gen
    for name, t in (('demo state', ds), ('demo action', da), ('gen state', gs), ('gen action', ga)):
        _chk_f32(t, name)
    if gs.dim() != 4 or gs.shape[0] != K or ga.shape[:2] != gs.shape[:2]:
        raise ValueError('generated stores: expected [%d, cap, T, d] / [%d, cap, T, d, d]' % (K, K))
    if plan.size < n_updates * n_active:
        raise ValueError('plan: fewer than n_updates * n_active entries')
    args = (params.data_ptr(), m.data_ptr(), v.data_ptr(), int(param_stride), int(K), *[int(x) for x in dims],
            *_geom_ptrs(geom, K), ds.data_ptr(), da.data_ptr(), ds.shape[0], gs.data_ptr(), ga.data_ptr(), gs.shape[1],
            plan.ctypes.data, plan_dev.data_ptr(), plan_dev.numel() * plan_dev.element_size(), int(n_updates), int(n_active),
            int(n_demo), int(n_gen), int(steps), int(demo_divisor), float(keep_prob), int(bool(l1l2)), float(beta1), float(beta2),
            float(eps), stats.data_ptr(), ws.data_ptr(), ws.numel() * ws.element_size())
    if gen_log_z is None:
        L.check(L.lib().mfg_reward_net_train_steps_pop(*args, _stream()), 'mfg_reward_net_train_steps_pop')
        return
    _chk_f64(gen_log_z, 'gen_log_z')
    if tuple(gen_log_z.shape) != (K, gs.shape[1]):
        raise ValueError('gen_log_z: expected [%d, %d]' % (K, gs.shape[1]))
    L.check(L.lib().mfg_reward_net_train_steps_pop_z(*args, gen_log_z.data_ptr(), _stream()), 'mfg_reward_net_train_steps_pop_z')


def episode_buffers(B, d, device):
    return {'scratch': torch.empty(B, d, dtype=torch.float32, device=device),
            'reward': torch.empty(B, dtype=torch.float32, device=device),
            'delta': torch.empty(B, dtype=torch.float64, device=device),
            'g': torch.empty(B, dtype=torch.float64, device=device)}


def jsd(p, q):
    _chk_f32(p, 'p'); _chk_f32(q, 'q')
    B, d = p.shape
    out = torch.empty(B, dtype=torch.float64, device=p.device)
    L.check(L.lib().mfg_jsd(p.data_ptr(), q.data_ptr(), B, d, out.data_ptr(), _stream()), 'mfg_jsd')
    return out


def evaluate_pop_workspace(N, L_rows, d, K, repeats, traj_given, device):
    """The scratch buffer of one evaluate_pop call (mfg_evaluate_pop_workspace_bytes, rounded up to whole doubles)."""
    nbytes = int(L.lib().mfg_evaluate_pop_workspace_bytes(int(N), int(L_rows), int(d), int(K), int(repeats), int(bool(traj_given))))
    return torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=device)


def pop_validate_workspace_bytes(N, L_rows, d, K, repeats, with_score=False):
    """Bytes of scratch a validation block needs (mfg_pop_validate_workspace_bytes; host only, 0 for a degenerate shape)."""
    return int(L.lib().mfg_pop_validate_workspace_bytes(int(N), int(L_rows), int(d), int(K), int(repeats), int(bool(with_score))))


def pop_validate_workspace(N, L_rows, d, K, repeats, with_score, device):
    """The scratch buffer of a validation block (Context.set_pop_validate), rounded up to whole doubles."""
    nbytes = pop_validate_workspace_bytes(N, L_rows, d, K, repeats, with_score)
    return torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=device)


def evaluate_pop(emp32, emp64, thetas, shifts, alpha_scales, seeds, first_step=0, repeats=1, precision='mixed', want_traj=False,
                 ws=None):
    """The eight evaluate() metrics of K policies in two launches (mfg_evaluate_pop, mfg_ac2.py:595-689): emp32 / emp64
    [N,L,d] the test files' rows; thetas, shifts, alpha_scales fp64 and seeds int64 (read as uint64) device arrays [K].
    Learner k's trajectory j (0 <= j < N repeats) starts at emp32[j mod N, 0] under Philox (seeds[k], first_step + t, j).
    Returns the device fp64 tensor [K, 8] (mean / std of l1_final, l1_mean, JSD_final, JSD_mean), and with want_traj also
    the trajectories [K, N repeats, L, d] fp32."""
    _chk_f32(emp32, 'emp32'); _chk_f64(emp64, 'emp64')
    if emp32.dim() != 3 or tuple(emp64.shape) != tuple(emp32.shape):
        raise ValueError('emp32 / emp64: expected two [N, L, d] tensors of the same shape, got %s and %s'
                         % (tuple(emp32.shape), tuple(emp64.shape)))
    N, Lr, d = emp32.shape
    K = thetas.numel()
    _chk_pop(K, 'thetas', thetas, torch.float64)
    for name, t in (('shifts', shifts), ('alpha_scales', alpha_scales)):
        _chk_pop(K, name, t, torch.float64)
    _chk_pop(K, 'seeds', seeds, torch.int64)
    repeats = int(repeats)
    if repeats < 1:
        raise ValueError('repeats=%d: at least one rollout per test file' % repeats)
    dev = emp32.device
    metrics = torch.empty(K, 8, dtype=torch.float64, device=dev)
    traj = torch.empty(K, N * repeats, Lr, d, dtype=torch.float32, device=dev) if want_traj else None
    if ws is None:
        ws = evaluate_pop_workspace(N, Lr, d, K, repeats, want_traj, dev)
    L.check(L.lib().mfg_evaluate_pop(emp32.data_ptr(), emp64.data_ptr(), N, Lr, d, K, thetas.data_ptr(), shifts.data_ptr(),
                                     alpha_scales.data_ptr(), seeds.data_ptr(), int(first_step), repeats, L.PRECISIONS[precision],
                                     metrics.data_ptr(), _ptr(traj), ws.data_ptr(), ws.numel() * ws.element_size(), _stream()),
            'mfg_evaluate_pop')
    return (metrics, traj) if want_traj else metrics


def forecast_pop_workspace(N, horizon, d, K, repeats, traj_given, device):
    """The scratch buffer of one forecast_pop call (mfg_forecast_pop_workspace_bytes, rounded up to whole doubles)."""
    nbytes = int(L.lib().mfg_forecast_pop_workspace_bytes(int(N), int(horizon), int(d), int(K), int(repeats), int(bool(traj_given))))
    return torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=device)


def check_forecast_args(start_shape, horizon, repeats, ranks, precision, emp32_shape=None, emp64_shape=None):
    """The argument rules of forecast_pop that need no GPU (ValueError): start32 [N, d], horizon >= 2, 1 <= repeats <=
    FORECAST_MAX_REPEATS, at most FORECAST_MAX_RANKS ranks, each in [0, repeats), a known precision, emp32 / emp64 both
    [N, horizon, d] or both absent.  Returns (N, d, horizon, repeats, ranks as a list of ints)."""
    if len(start_shape) != 2:
        raise ValueError('start32: expected [N, d], got %s' % (tuple(start_shape),))
    N, d = int(start_shape[0]), int(start_shape[1])
    horizon, repeats = int(horizon), int(repeats)
    if horizon < 2:
        raise ValueError('horizon=%d: a forecast rolls at least one step (horizon >= 2)' % horizon)
    if repeats < 1:
        raise ValueError('repeats=%d: at least one rollout per start state' % repeats)
    if repeats > L.FORECAST_MAX_REPEATS:
        raise ValueError('repeats=%d: at most %d members per start state (MFG_FORECAST_MAX_REPEATS)' % (repeats, L.FORECAST_MAX_REPEATS))
    ranks = [int(r) for r in ranks]
    if len(ranks) > L.FORECAST_MAX_RANKS:
        raise ValueError('%d ranks: at most %d order statistics per call (MFG_FORECAST_MAX_RANKS)' % (len(ranks), L.FORECAST_MAX_RANKS))
    for r in ranks:
        if not 0 <= r < repeats:
            raise ValueError('rank %d outside [0, repeats=%d)' % (r, repeats))
    if precision not in L.PRECISIONS:
        raise ValueError("precision must be 'mixed' or 'f64'")
    if (emp32_shape is None) != (emp64_shape is None):
        raise ValueError('emp32 and emp64: give both or neither')
    if emp32_shape is not None and (tuple(emp32_shape) != (N, horizon, d) or tuple(emp64_shape) != (N, horizon, d)):
        raise ValueError('emp32 / emp64: expected two [%d, %d, %d] tensors, got %s and %s'
                         % (N, horizon, d, tuple(emp32_shape), tuple(emp64_shape)))
    return N, d, horizon, repeats, ranks


def forecast_pop(start32, thetas, shifts, alpha_scales, seeds, horizon, first_step=0, repeats=1, ranks=(), precision='mixed',
                 emp32=None, emp64=None, want_traj=False, ws=None):
    """The ensemble forecast of K policies in at most three launches (mfg_forecast_pop; the forecast the reference plots from one
    path, mfg_ac2.py:566-592, :763): start32 [N,d] the start states; thetas, shifts, alpha_scales fp64 and seeds int64 (read
    as uint64) device arrays [K].  Learner k's member j (0 <= j < N repeats) starts at start32[j mod N] under Philox (seeds[k],
    first_step + t, j) and has `horizon` rows, row 0 the start row.  Returns a dict of device tensors: mean, std [K,N,horizon,d]
    fp64 over the `repeats` members of each start state (std: ddof = 0); quant [K,N,horizon,Q,d] fp32, the order statistics of
    the 0-based `ranks` among those members (None without ranks); curves [K,horizon,4] fp64 (l1_mean, l1_std, jsd_mean, jsd_std
    over all N repeats members per hour against emp32 / emp64 [N,horizon,d]; None without them); traj [K, N repeats, horizon, d]
    fp32 with want_traj (None otherwise)."""
    import ctypes as C
    _chk_f32(start32, 'start32')
    if emp32 is not None:
        _chk_f32(emp32, 'emp32')
    if emp64 is not None:
        _chk_f64(emp64, 'emp64')
    N, d, H, repeats, ranks = check_forecast_args(start32.shape, horizon, repeats, ranks, precision,
                                                  None if emp32 is None else emp32.shape, None if emp64 is None else emp64.shape)
    K = thetas.numel()
    _chk_pop(K, 'thetas', thetas, torch.float64)
    for name, t in (('shifts', shifts), ('alpha_scales', alpha_scales)):
        _chk_pop(K, name, t, torch.float64)
    _chk_pop(K, 'seeds', seeds, torch.int64)
    dev = start32.device
    Q = len(ranks)
    out = {'mean': torch.empty(K, N, H, d, dtype=torch.float64, device=dev),
           'std': torch.empty(K, N, H, d, dtype=torch.float64, device=dev),
           'quant': torch.empty(K, N, H, Q, d, dtype=torch.float32, device=dev) if Q else None,
           'curves': torch.empty(K, H, 4, dtype=torch.float64, device=dev) if emp32 is not None else None,
           'traj': torch.empty(K, N * repeats, H, d, dtype=torch.float32, device=dev) if want_traj else None}
    if ws is None:
        ws = forecast_pop_workspace(N, H, d, K, repeats, want_traj, dev)
    rk = (C.c_int32 * max(Q, 1))(*ranks)
    L.check(L.lib().mfg_forecast_pop(start32.data_ptr(), N, H, d, K, thetas.data_ptr(), shifts.data_ptr(), alpha_scales.data_ptr(),
                                     seeds.data_ptr(), int(first_step), repeats, L.PRECISIONS[precision], rk, Q, _ptr(emp32),
                                     _ptr(emp64), out['mean'].data_ptr(), out['std'].data_ptr(), _ptr(out['quant']),
                                     _ptr(out['curves']), _ptr(out['traj']), ws.data_ptr(), ws.numel() * ws.element_size(),
                                     _stream()), 'mfg_forecast_pop')
    return out


def _chk_i32(t, name):
    if not (t.is_cuda and t.dtype == torch.int32 and t.is_contiguous()):
        raise ValueError('%s must be a contiguous int32 CUDA tensor' % name)
    return t


def check_agents(agents):
    """`agents` as an int in [1, AGENTS_MAX] (ValueError otherwise)."""
    if isinstance(agents, bool) or int(agents) != agents:
        raise ValueError('agents=%r: a whole number of agents' % (agents,))
    agents = int(agents)
    if not 1 <= agents <= L.AGENTS_MAX:
        raise ValueError('agents=%d outside [1, %d] (MFG_AGENTS_MAX)' % (agents, L.AGENTS_MAX))
    return agents


def agents_step_pop(counts, P, agents, seeds, step=0, traj_offset=0, want_pi=True, want_moves=False):
    """One resampling step of finite-population members in one launch (mfg_agents_step_pop): counts [K,B,d] int32 (each row
    summing to `agents`), P [K,B,d,d] fp32 the members' actions, seeds int64 (read as uint64) device array [K].  Every agent of
    topic i of member (k, b) -- Philox (seeds[k], step, member id traj_offset + b) -- moves to a topic drawn from P[k,b,i,:].
    Returns (counts_next [K,B,d] int32, pi_next [K,B,d] fp32 = counts_next / agents or None, moves [K,B,d,d] int32 or None);
    a member with an unusable row (a sum that is not finite or <= 0 under agents, a count outside [0, agents]) gets -1 / NaN."""
    _chk_i32(counts, 'counts'); _chk_f32(P, 'P')
    if counts.dim() != 3:
        raise ValueError('counts: expected [K, B, d], got %s' % (tuple(counts.shape),))
    K, B, d = counts.shape
    if tuple(P.shape) != (K, B, d, d):
        raise ValueError('P: expected [%d, %d, %d, %d], got %s' % (K, B, d, d, tuple(P.shape)))
    if not 1 <= d <= 64:
        raise ValueError('d=%d: finite populations cover d <= 64 (as the populations do)' % d)
    agents = check_agents(agents)
    _chk_pop(K, 'seeds', seeds, torch.int64)
    dev = counts.device
    counts_next = torch.empty_like(counts)
    pi_next = torch.empty(K, B, d, dtype=torch.float32, device=dev) if want_pi else None
    moves = torch.empty(K, B, d, d, dtype=torch.int32, device=dev) if want_moves else None
    L.check(L.lib().mfg_agents_step_pop(counts.data_ptr(), P.data_ptr(), B, d, K, agents, seeds.data_ptr(), int(step),
                                        int(traj_offset), counts_next.data_ptr(), _ptr(pi_next), _ptr(moves), _stream()),
            'mfg_agents_step_pop')
    return counts_next, pi_next, moves


def forecast_agents_pop_workspace(N, horizon, d, K, repeats, traj_given, counts_given, device):
    """The scratch buffer of one forecast_agents_pop call (mfg_forecast_agents_pop_workspace_bytes; whole doubles)."""
    nbytes = int(L.lib().mfg_forecast_agents_pop_workspace_bytes(int(N), int(horizon), int(d), int(K), int(repeats),
                                                                 int(bool(traj_given)), int(bool(counts_given))))
    return torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=device)


def check_forecast_agents_args(counts_shape, agents, horizon, repeats, ranks, precision, emp32_shape=None, emp64_shape=None):
    """The argument rules of forecast_agents_pop that need no GPU (ValueError): those of check_forecast_args with counts0
    [N, d] for start32, 1 <= d <= 64, and agents a whole number in [1, AGENTS_MAX].  Returns (N, d, horizon, repeats, ranks as a
    list of ints, agents)."""
    N, d, horizon, repeats, ranks = check_forecast_args(counts_shape, horizon, repeats, ranks, precision, emp32_shape, emp64_shape)
    if not 1 <= d <= 64:
        raise ValueError('d=%d: finite populations cover d <= 64 (as the populations do)' % d)
    return N, d, horizon, repeats, ranks, check_agents(agents)


def forecast_agents_pop(counts0, agents, thetas, shifts, alpha_scales, seeds, horizon, first_step=0, repeats=1, ranks=(),
                        precision='mixed', emp32=None, emp64=None, want_traj=False, want_counts=False, want_actions=False, ws=None):
    """forecast_pop with finite-population members (mfg_forecast_agents_pop): counts0 [N,d] int32 the start counts, each row
    summing to `agents`.  Member j of learner k draws its action as forecast_pop's member j does -- from the histogram row of its
    counts, under Philox (seeds[k], first_step + t, j) -- and then moves each of its agents by a draw from the action's row of
    the agent's topic.  Returns forecast_pop's dict (mean, std, quant, curves, traj) with counts [K, N repeats, horizon, d] int32
    (want_counts) and actions [K, N repeats, horizon - 1, d, d] fp32 (want_actions), None otherwise."""
    import ctypes as C
    _chk_i32(counts0, 'counts0')
    if emp32 is not None:
        _chk_f32(emp32, 'emp32')
    if emp64 is not None:
        _chk_f64(emp64, 'emp64')
    N, d, H, repeats, ranks, agents = check_forecast_agents_args(
        counts0.shape, agents, horizon, repeats, ranks, precision, None if emp32 is None else emp32.shape,
        None if emp64 is None else emp64.shape)
    K = thetas.numel()
    _chk_pop(K, 'thetas', thetas, torch.float64)
    for name, t in (('shifts', shifts), ('alpha_scales', alpha_scales)):
        _chk_pop(K, name, t, torch.float64)
    _chk_pop(K, 'seeds', seeds, torch.int64)
    dev = counts0.device
    Q, NR = len(ranks), N * repeats
    out = {'mean': torch.empty(K, N, H, d, dtype=torch.float64, device=dev),
           'std': torch.empty(K, N, H, d, dtype=torch.float64, device=dev),
           'quant': torch.empty(K, N, H, Q, d, dtype=torch.float32, device=dev) if Q else None,
           'curves': torch.empty(K, H, 4, dtype=torch.float64, device=dev) if emp32 is not None else None,
           'traj': torch.empty(K, NR, H, d, dtype=torch.float32, device=dev) if want_traj else None,
           'counts': torch.empty(K, NR, H, d, dtype=torch.int32, device=dev) if want_counts else None,
           'actions': torch.empty(K, NR, H - 1, d, d, dtype=torch.float32, device=dev) if want_actions else None}
    if ws is None:
        ws = forecast_agents_pop_workspace(N, H, d, K, repeats, want_traj, want_counts, dev)
    rk = (C.c_int32 * max(Q, 1))(*ranks)
    L.check(L.lib().mfg_forecast_agents_pop(counts0.data_ptr(), N, H, d, K, agents, thetas.data_ptr(), shifts.data_ptr(),
                                            alpha_scales.data_ptr(), seeds.data_ptr(), int(first_step), repeats,
                                            L.PRECISIONS[precision], rk, Q, _ptr(emp32), _ptr(emp64), out['mean'].data_ptr(),
                                            out['std'].data_ptr(), _ptr(out['quant']), _ptr(out['curves']), _ptr(out['traj']),
                                            _ptr(out['counts']), _ptr(out['actions']), ws.data_ptr(),
                                            ws.numel() * ws.element_size(), _stream()), 'mfg_forecast_agents_pop')
    return out


def forecast_score_workspace_bytes(N, horizon, d, K, repeats):
    """mfg_forecast_score_workspace_bytes: the scratch bytes of one forecast_score call (needs the library, no GPU)."""
    return int(L.lib().mfg_forecast_score_workspace_bytes(int(N), int(horizon), int(d), int(K), int(repeats)))


def forecast_score_workspace(N, horizon, d, K, repeats, device):
    """The scratch buffer of one forecast_score call (whole doubles)."""
    return torch.empty((forecast_score_workspace_bytes(N, horizon, d, K, repeats) + 7) // 8, dtype=torch.float64, device=device)


def check_forecast_score_args(traj_shape, emp32_shape, emp64_shape, N, repeats):
    """The argument rules of forecast_score that need no GPU (ValueError): traj [K, N repeats, H, d] with 1 <= K <= POP_MAX_K,
    N >= 1, H >= 2, 1 <= d <= 64, 1 <= repeats <= FORECAST_MAX_REPEATS; emp32 and emp64 [N, H, d].  Returns (K, N, H, d,
    repeats)."""
    N, repeats = int(N), int(repeats)
    if N < 1:
        raise ValueError('N=%d: at least one start state' % N)
    if repeats < 1:
        raise ValueError('repeats=%d: an ensemble has at least one member' % repeats)
    if repeats > L.FORECAST_MAX_REPEATS:
        raise ValueError('repeats=%d: at most %d members per start state (MFG_FORECAST_MAX_REPEATS)' % (repeats, L.FORECAST_MAX_REPEATS))
    if len(traj_shape) != 4 or int(traj_shape[1]) != N * repeats:
        raise ValueError('traj: expected [K, N repeats = %d, H, d], got %s' % (N * repeats, tuple(traj_shape)))
    K, H, d = int(traj_shape[0]), int(traj_shape[2]), int(traj_shape[3])
    if not 1 <= K <= L.POP_MAX_K:
        raise ValueError('traj: %d policies outside [1, %d]' % (K, L.POP_MAX_K))
    if H < 2:
        raise ValueError('traj: H=%d rows per member, a forecast has at least 2' % H)
    if not 1 <= d <= 64:
        raise ValueError('d=%d: the forecast scores cover d <= 64 (as the ensemble forecast does)' % d)
    if tuple(emp32_shape) != (N, H, d) or tuple(emp64_shape) != (N, H, d):
        raise ValueError('emp32 / emp64: expected two [%d, %d, %d] tensors, got %s and %s'
                         % (N, H, d, tuple(emp32_shape), tuple(emp64_shape)))
    return K, N, H, d, repeats


def forecast_score(traj, emp32, emp64, N, repeats, want_energy=True, ws=None):
    """The proper scores of given ensemble members in at most two launches (mfg_forecast_score): traj [K, N repeats, H, d] fp32
    as forecast_pop(want_traj=True) returns it (member r of start row n is row r N + n), emp32 / emp64 [N, H, d] the held-out
    rows.  Returns a dict of device tensors: crps [K,N,H,d] fp64; less, equal [K,N,H,d] int32 (members below / equal to the
    fp32 observation; -1 in a cell with a non-finite value, whose scores are NaN); energy [K,N,H] fp64 (None without
    want_energy, which skips the O(repeats^2 d) pass); summary [K,H,2] fp64 (mean crps over (n, c), mean energy over n or NaN)."""
    for name, t in (('traj', traj), ('emp32', emp32)):
        _chk_f32(t, name)
    _chk_f64(emp64, 'emp64')
    K, N, H, d, repeats = check_forecast_score_args(traj.shape, emp32.shape, emp64.shape, N, repeats)
    dev = traj.device
    out = {'crps': torch.empty(K, N, H, d, dtype=torch.float64, device=dev),
           'less': torch.empty(K, N, H, d, dtype=torch.int32, device=dev),
           'equal': torch.empty(K, N, H, d, dtype=torch.int32, device=dev),
           'energy': torch.empty(K, N, H, dtype=torch.float64, device=dev) if want_energy else None,
           'summary': torch.empty(K, H, 2, dtype=torch.float64, device=dev)}
    if ws is None:
        ws = forecast_score_workspace(N, H, d, K, repeats, dev)
    L.check(L.lib().mfg_forecast_score(traj.data_ptr(), N, H, d, K, repeats, emp32.data_ptr(), emp64.data_ptr(),
                                       out['crps'].data_ptr(), out['less'].data_ptr(), out['equal'].data_ptr(),
                                       _ptr(out['energy']), out['summary'].data_ptr(), ws.data_ptr(),
                                       ws.numel() * ws.element_size(), _stream()), 'mfg_forecast_score')
    return out


def hist_edges(first, last, bins):
    """The bin edges of mfg_row_distribution, i.e. of np.histogram(x, bins, range=(first, last)), restated in plain Python
    floats: first - 0.5, last + 0.5 when the two are equal; step = (last - first) / bins; edge_i = fl(fl(i step) + first) for
    i < bins (two roundings) and edge_bins = last.  Returns a NumPy fp64 array [bins + 1]."""
    import numpy as np
    first, last, bins = float(first), float(last), int(bins)
    if first == last:
        first, last = first - 0.5, last + 0.5
    step = (last - first) / bins
    out = []
    for i in range(bins):
        m = float(i) * step
        out.append(m + first)
    out.append(last)
    return np.array(out, dtype=np.float64)


def check_row_distribution_args(R, N, stride, bins, hist_range, G, x_lo, x_hi, dtype=torch.float32, is_cuda=True):
    """The argument rules of row_distribution that need no GPU (ValueError): R >= 1 rows of 1 <= N < 2^31 values `stride` >= N
    apart, fp32 on the device; 1 <= bins <= DIST_MAX_BINS; hist_range None or finite (lo, hi) with lo < hi; 0 <= G <=
    DIST_MAX_GRID grid points between finite x_lo and x_hi.  Returns (use_range, lo, hi)."""
    import math
    if dtype != torch.float32 or not is_cuda:
        raise ValueError('values must be a contiguous float32 CUDA tensor')
    R, N, stride, bins, G = int(R), int(N), int(stride), int(bins), int(G)
    if R < 1:
        raise ValueError('R=%d: at least one row' % R)
    if not 1 <= N < 2 ** 31:
        raise ValueError('N=%d outside [1, 2^31)' % N)
    if stride < N:
        raise ValueError('stride=%d < N=%d' % (stride, N))
    if not 1 <= bins <= L.DIST_MAX_BINS:
        raise ValueError('bins=%d outside [1, %d] (MFG_DIST_MAX_BINS)' % (bins, L.DIST_MAX_BINS))
    if not 0 <= G <= L.DIST_MAX_GRID:
        raise ValueError('G=%d grid points outside [0, %d] (MFG_DIST_MAX_GRID)' % (G, L.DIST_MAX_GRID))
    if G and not (math.isfinite(float(x_lo)) and math.isfinite(float(x_hi))):
        raise ValueError('KDE grid: finite x_lo and x_hi needed')
    if hist_range is None:
        return 0, 0.0, 0.0
    lo, hi = (float(v) for v in hist_range)
    if not (math.isfinite(lo) and math.isfinite(hi)) or lo >= hi:
        raise ValueError('hist_range=(%r, %r): finite lo < hi needed' % (lo, hi))
    return 1, lo, hi


def row_distribution(values, N=None, bins=20, hist_range=None, G=0, x_lo=0.0, x_hi=1.0, out=None):
    """The distribution summary of the rows of `values` [R, stride] fp32 in one launch (mfg_row_distribution; plt.hist and
    gaussian_kde of plot_reward_distribution, ac_irl.py:1087-1119): the first N values of every row (default: all).  Returns
    a dict of device tensors: moments [R,6] fp64 (kept, min, max, mean, variance with ddof 1, KDE bandwidth variance), counts
    [R,bins] int64 and edges [R,bins+1] fp64 (np.histogram on the fp64 copy; hist_range=(lo, hi): a common range), density
    [R,G] fp64 (gaussian_kde on linspace(x_lo, x_hi, G); None with G = 0) and status [R] int32 (DIST_NONFINITE: NaN row,
    DIST_NO_KDE: NaN density).  out: the same dict with tensors to fill instead."""
    if values.dim() != 2:
        raise ValueError('values: expected [R, stride], got %s' % (tuple(values.shape),))
    R, stride = values.shape
    N = stride if N is None else int(N)
    use_range, lo, hi = check_row_distribution_args(R, N, stride, bins, hist_range, G, x_lo, x_hi, values.dtype, values.is_cuda)
    _chk_f32(values, 'values')
    bins, G = int(bins), int(G)
    dev = values.device
    if out is None:
        out = {'moments': torch.empty(R, 6, dtype=torch.float64, device=dev),
               'counts': torch.empty(R, bins, dtype=torch.int64, device=dev),
               'edges': torch.empty(R, bins + 1, dtype=torch.float64, device=dev),
               'density': torch.empty(R, G, dtype=torch.float64, device=dev) if G else None,
               'status': torch.empty(R, dtype=torch.int32, device=dev)}
    else:
        for name, shape, dt in (('moments', (R, 6), torch.float64), ('counts', (R, bins), torch.int64),
                                ('edges', (R, bins + 1), torch.float64), ('density', (R, G), torch.float64),
                                ('status', (R,), torch.int32)):
            t = out.get(name)
            if name == 'density' and not G:
                continue
            if t is None or tuple(t.shape) != shape or t.dtype != dt or not t.is_cuda or not t.is_contiguous():
                raise ValueError('out[%r]: expected a contiguous %s device tensor %s' % (name, dt, shape))
    nbytes = int(L.lib().mfg_row_distribution_workspace_bytes(R, N, bins, G))
    ws = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=dev) if nbytes else None
    L.check(L.lib().mfg_row_distribution(values.data_ptr(), R, N, stride, bins, use_range, lo, hi, G, float(x_lo), float(x_hi),
                                         out['moments'].data_ptr(), out['counts'].data_ptr(), out['edges'].data_ptr(),
                                         _ptr(out['density']) if G else None, out['status'].data_ptr(), _ptr(ws), nbytes,
                                         _stream()), 'mfg_row_distribution')
    return out


def action_mean_pop(action, K=None, out=None):
    """The mean action matrix of K learners in two launches (mfg_action_mean_pop; np.mean(actions, axis=0) of
    plot_action_heatmap, ac_irl.py:1276-1289): action [K,N,d,d] fp32, or [N,d,d] shared by K learners (default K = 1).
    Returns mean [K,d,d] fp64 on the device."""
    _chk_f32(action, 'action')
    shared = action.dim() == 3
    if shared:
        K = 1 if K is None else int(K)
        N, d = action.shape[0], action.shape[1]
    else:
        if action.dim() != 4 or (K is not None and int(K) != action.shape[0]):
            raise ValueError('action: expected [N, d, d] or [K, N, d, d], got %s' % (tuple(action.shape),))
        K, N, d = action.shape[:3]
    if action.shape[-1] != d or min(K, N, d) < 1:
        raise ValueError('action: square matrices and no empty dimension expected, got %s' % (tuple(action.shape),))
    if d > 64:
        raise ValueError('d=%d: the mean action covers d <= 64' % d)
    dev = action.device
    if out is None:
        out = torch.empty(K, d, d, dtype=torch.float64, device=dev)
    elif tuple(out.shape) != (K, d, d):
        raise ValueError('out: expected [%d, %d, %d]' % (K, d, d))
    _chk_f64(out, 'out')
    nbytes = int(L.lib().mfg_action_mean_pop_workspace_bytes(K, N, d))
    ws = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=dev)
    L.check(L.lib().mfg_action_mean_pop(action.data_ptr(), 0 if shared else N * d * d, K, N, d, out.data_ptr(), ws.data_ptr(),
                                        ws.numel() * ws.element_size(), _stream()), 'mfg_action_mean_pop')
    return out


def consistency_given(P, want_steps=True, want_V=True):
    """The backward-equation check of K groups of given actions in two launches (mfg_consistency_given; evaluate_synthetic /
    evaluate_synthetic_JSD, mfg_synthetic.py:741-899): P [K,M,T,d,d] fp32.  Returns a dict of device fp64 tensors: metrics
    [K,4] = (l1_mean, l1_std, jsd_mean, jsd_std) over each group's M T hours (std: ddof = 0); steps [K,M,T,2] (l1, jsd per
    hour) and V [K,M,T+1,d], each None unless asked for."""
    _chk_f32(P, 'P')
    if P.dim() != 5 or P.shape[3] != P.shape[4]:
        raise ValueError('P: expected [K, M, T, d, d], got %s' % (tuple(P.shape),))
    K, M, T, d, _ = P.shape
    if min(K, M, T, d) < 1:
        raise ValueError('P: an empty dimension in %s' % (tuple(P.shape),))
    dev = P.device
    out = {'metrics': torch.empty(K, 4, dtype=torch.float64, device=dev),
           'steps': torch.empty(K, M, T, 2, dtype=torch.float64, device=dev) if want_steps else None,
           'V': torch.empty(K, M, T + 1, d, dtype=torch.float64, device=dev) if want_V else None}
    nbytes = int(L.lib().mfg_consistency_given_workspace_bytes(K, M, T, int(bool(want_steps))))
    ws = torch.empty(max(nbytes // 8, 1), dtype=torch.float64, device=dev)
    L.check(L.lib().mfg_consistency_given(P.data_ptr(), K, M, T, d, out['metrics'].data_ptr(), _ptr(out['steps']), _ptr(out['V']),
                                          ws.data_ptr(), ws.numel() * ws.element_size(), _stream()), 'mfg_consistency_given')
    return out


def consistency_pop_workspace_bytes(N, hours, d, K, repeats, steps_given=False, actions_given=False, traj_given=False):
    """mfg_consistency_pop_workspace_bytes: the scratch bytes of one consistency_pop call (needs the library, not a GPU)."""
    return int(L.lib().mfg_consistency_pop_workspace_bytes(int(N), int(hours), int(d), int(K), int(repeats), int(bool(steps_given)),
                                                           int(bool(actions_given)), int(bool(traj_given))))


def check_consistency_args(start_shape, hours, repeats, precision, K=1, first_step=0):
    """The argument rules of consistency_pop that need no GPU (ValueError): start32 [N, d] with N >= 1 and 1 <= d <= 64,
    hours >= 2, repeats >= 1, 1 <= K <= POP_MAX_K, a known precision, a Philox step first_step + hours - 1 below 2^32.
    Returns (N, d, hours, repeats)."""
    if len(start_shape) != 2:
        raise ValueError('start32: expected [N, d], got %s' % (tuple(start_shape),))
    N, d = int(start_shape[0]), int(start_shape[1])
    hours, repeats, K, first_step = int(hours), int(repeats), int(K), int(first_step)
    if N < 1:
        raise ValueError('start32: no start rows')
    if not 1 <= d <= 64:
        raise ValueError('d=%d: the backward-equation check covers 1 <= d <= 64 (as the populations do)' % d)
    if hours < 2:
        raise ValueError('hours=%d: the check needs at least one action matrix (hours >= 2)' % hours)
    if repeats < 1:
        raise ValueError('repeats=%d: at least one rollout per start row' % repeats)
    if not 1 <= K <= L.POP_MAX_K:
        raise ValueError('K=%d policies: between 1 and %d per call (MFG_POP_MAX_K)' % (K, L.POP_MAX_K))
    if precision not in L.PRECISIONS:
        raise ValueError("precision must be 'mixed' or 'f64'")
    if first_step < 0 or first_step + hours - 1 > 0xFFFFFFFF:
        raise ValueError('first_step=%d: the Philox step counter would wrap within %d hours' % (first_step, hours))
    return N, d, hours, repeats


def consistency_pop(start32, thetas, shifts, alpha_scales, seeds, hours, *, first_step=0, repeats=1, precision='mixed',
                    want_steps=False, want_V=False, want_actions=False, want_traj=False, ws=None):
    """The backward-equation check of K policies in three launches (mfg_consistency_pop): start32 [N,d] the start rows; thetas,
    shifts, alpha_scales fp64 and seeds int64 (read as uint64) device arrays [K].  Learner k's member j (0 <= j < N repeats)
    starts at start32[j mod N] under Philox (seeds[k], first_step + t, j) and has `hours` rows, i.e. hours - 1 action matrices:
    generate_trajectory over the repeats-fold tiled start rows.  Returns a dict of device tensors: metrics [K,4] fp64 (l1_mean,
    l1_std, jsd_mean, jsd_std over the policy's N repeats (hours - 1) values, ddof = 0) and, each None unless asked for, steps
    [K, N repeats, hours-1, 2] fp64, V [K, N repeats, hours, d] fp64, actions [K, N repeats, hours-1, d, d] fp32 and traj
    [K, N repeats, hours, d] fp32."""
    _chk_f32(start32, 'start32')
    K = thetas.numel()
    N, d, H, repeats = check_consistency_args(start32.shape, hours, repeats, precision, K, first_step)
    _chk_pop(K, 'thetas', thetas, torch.float64)
    for name, t in (('shifts', shifts), ('alpha_scales', alpha_scales)):
        _chk_pop(K, name, t, torch.float64)
    _chk_pop(K, 'seeds', seeds, torch.int64)
    dev = start32.device
    NR, T = N * repeats, H - 1
    out = {'metrics': torch.empty(K, 4, dtype=torch.float64, device=dev),
           'steps': torch.empty(K, NR, T, 2, dtype=torch.float64, device=dev) if want_steps else None,
           'V': torch.empty(K, NR, H, d, dtype=torch.float64, device=dev) if want_V else None,
           'actions': torch.empty(K, NR, T, d, d, dtype=torch.float32, device=dev) if want_actions else None,
           'traj': torch.empty(K, NR, H, d, dtype=torch.float32, device=dev) if want_traj else None}
    if ws is None:
        nbytes = consistency_pop_workspace_bytes(N, H, d, K, repeats, want_steps, want_actions, want_traj)
        ws = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=dev)
    L.check(L.lib().mfg_consistency_pop(start32.data_ptr(), N, H, d, K, thetas.data_ptr(), shifts.data_ptr(),
                                        alpha_scales.data_ptr(), seeds.data_ptr(), int(first_step), repeats,
                                        L.PRECISIONS[precision], out['metrics'].data_ptr(), _ptr(out['steps']), _ptr(out['V']),
                                        _ptr(out['actions']), _ptr(out['traj']), ws.data_ptr(), ws.numel() * ws.element_size(),
                                        _stream()), 'mfg_consistency_pop')
    return out


def check_var_fit_args(days_shape, lags, ridges, train_n, test_n, origins, train_stride=None, test_stride=None):
    """The argument rules of var_fit_pop that need no GPU (ValueError), the limits of mfg_var_fit_pop: days [D, Hd, d] with
    1 <= Hd <= 64 and 1 <= d <= 64; per model a lag >= 1 with m = 1 + lag d <= VAR_MAX_REGRESSORS, 1 to 64 training and 0 to 64
    test days (within the index tables' strides when given), n = n_train Hd - lag >= 1, origin 0 or 1 and with origin 1
    lag <= n_train Hd + 1, a ridge that is finite and > 0.  Returns (K, D, Hd, d, M, S_max): M the largest m, S_max the largest
    n_test Hd."""
    import math
    if len(days_shape) != 3:
        raise ValueError('days: expected [D, Hd, d], got %s' % (tuple(days_shape),))
    D, Hd, d = (int(s) for s in days_shape)
    if D < 1:
        raise ValueError('days: no day')
    if not 1 <= Hd <= L.VAR_MAX_HOURS:
        raise ValueError('Hd=%d: a day has 1 to %d rows' % (Hd, L.VAR_MAX_HOURS))
    if not 1 <= d <= L.VAR_MAX_D:
        raise ValueError('d=%d: the VAR population covers 1 <= d <= %d' % (d, L.VAR_MAX_D))
    cols = [list(lags), list(ridges), list(train_n), list(test_n), list(origins)]
    K = len(cols[0])
    if K < 1:
        raise ValueError('no models')
    if K > L.POP_MAX_K:
        raise ValueError('%d models: at most %d in one call (MFG_POP_MAX_K)' % (K, L.POP_MAX_K))
    if any(len(c) != K for c in cols):
        raise ValueError('lags, ridges, train_n, test_n and origins must have one entry per model (%d)' % K)
    M = S_max = 0
    for k, (p, lam, ntr, nte, org) in enumerate(zip(*cols)):
        p, ntr, nte, lam = int(p), int(ntr), int(nte), float(lam)
        if p < 1:
            raise ValueError('model %d: lag=%d < 1' % (k, p))
        if 1 + p * d > L.VAR_MAX_REGRESSORS:
            raise ValueError('model %d: 1 + lag d = %d regressors, at most %d (MFG_VAR_MAX_REGRESSORS)'
                             % (k, 1 + p * d, L.VAR_MAX_REGRESSORS))
        if not 1 <= ntr <= L.VAR_MAX_DAYS or (train_stride is not None and ntr > train_stride):
            raise ValueError('model %d: %d training days, a model has 1 to %d (and train_idx holds them)' % (k, ntr, L.VAR_MAX_DAYS))
        if not 0 <= nte <= L.VAR_MAX_DAYS or (test_stride is not None and nte > test_stride):
            raise ValueError('model %d: %d test days, a model has 0 to %d (and test_idx holds them)' % (k, nte, L.VAR_MAX_DAYS))
        if ntr * Hd - p < 1:
            raise ValueError('model %d: lag=%d leaves no row to fit of %d training rows' % (k, p, ntr * Hd))
        if org not in (0, 1):
            raise ValueError('model %d: origin=%r, 0 (the end of the training series) or 1 (rolling)' % (k, org))
        if int(org) == 1 and p > ntr * Hd + 1:
            raise ValueError('model %d: a rolling origin needs lag <= training rows + 1' % k)
        if not (lam > 0.0 and math.isfinite(lam)):
            raise ValueError('model %d: ridge=%r must be finite and > 0' % (k, lam))
        M, S_max = max(M, 1 + p * d), max(S_max, nte * Hd)
    return K, D, Hd, d, M, S_max


def var_models(lags, ridges, train_n, test_n, origins, d):
    """The host table of mfg_var_fit_pop: (an array of K _lib.VarModelStruct with ws_offset laid out by
    mfg_var_fit_workspace_bytes, the workspace bytes of the call).  Needs the library, no GPU."""
    K = len(lags)
    table = (L.VarModelStruct * K)()
    for k in range(K):
        table[k].lag, table[k].origin, table[k].n_train, table[k].n_test = int(lags[k]), int(origins[k]), int(train_n[k]), int(test_n[k])
        table[k].ridge = float(ridges[k])
    nbytes = int(L.lib().mfg_var_fit_workspace_bytes(K, table, int(d)))
    if nbytes == 0:
        raise ValueError('var_models: a lag outside [1, (MFG_VAR_MAX_REGRESSORS - 1) / d] or d outside [1, 64]')
    return table, nbytes


def var_models_device(table, device):
    """The device copy of a var_models table (a uint8 tensor of 32 K bytes)."""
    import ctypes as C
    import numpy as np
    raw = np.frombuffer(C.string_at(C.addressof(table), C.sizeof(table)), dtype=np.uint8).copy()
    return torch.as_tensor(raw).to(device)


VAR_OUTPUTS = ('coef', 'sse', 'insample', 'future', 'per_day', 'metrics', 'status')


def var_fit_shapes(K, d, M, S_max, test_stride):
    """name -> (shape, dtype) of the outputs of var_fit_pop."""
    f64 = torch.float64
    return {'coef': ((K, M, d), f64), 'sse': ((K, d), f64), 'insample': ((K, 2), f64), 'future': ((K, S_max, d), f64),
            'per_day': ((K, test_stride, 4), f64), 'metrics': ((K, 8), f64), 'status': ((K,), torch.int32)}


def var_fit_pop(days, lags, ridges, train_idx, train_n, test_idx, test_n, origins, *, want_future=True, want_per_day=True,
                out=None, workspace=None, models=None, M=None, S_max=None):
    """K vector autoregressions fitted, forecast and scored in the three launches of one call (mfg_var_fit_pop; the definitions
    are in include/mfg_hip.h).  days [D, Hd, d] fp64 on the device; lags, ridges, train_n, test_n, origins: K host values each
    (sequences or CPU tensors); train_idx [K, >= max train_n] and test_idx [K, >= max test_n] int32 device tensors of day indices
    (test_idx may be None when no model has a test day).  The fit is RIDGE regression of order lag (no information criterion
    picks a smaller order).  Returns a dict of device tensors: coef [K, M, d], sse [K, d], insample [K, 2], future [K, S_max, d]
    (None without want_future), per_day [K, test_stride, 4] (None without want_per_day), metrics [K, 8], status [K] int32.
    out / workspace / models: preallocated outputs (a dict by name), the scratch buffer and the (host table, device copy,
    bytes) of var_models / var_models_device -- then the call allocates nothing.  M / S_max: rows of coef / future per model
    when more than this call's models need (a chunk of a larger population)."""
    import ctypes as C
    M_want, S_want = M, S_max
    _chk_f64(days, 'days')
    as_list = lambda x: x.tolist() if hasattr(x, 'tolist') else list(x)
    lags, ridges, train_n, test_n, origins = (as_list(x) for x in (lags, ridges, train_n, test_n, origins))
    train_idx = _chk_i32(train_idx, 'train_idx')
    if train_idx.dim() != 2:
        raise ValueError('train_idx: expected [K, days], got %s' % (tuple(train_idx.shape),))
    test_stride = 0
    if test_idx is not None:
        test_idx = _chk_i32(test_idx, 'test_idx')
        if test_idx.dim() != 2:
            raise ValueError('test_idx: expected [K, days], got %s' % (tuple(test_idx.shape),))
        test_stride = int(test_idx.shape[1])
    K, D, Hd, d, M, S_max = check_var_fit_args(days.shape, lags, ridges, train_n, test_n, origins, int(train_idx.shape[1]),
                                               test_stride)
    if int(train_idx.shape[0]) != K or (test_idx is not None and int(test_idx.shape[0]) != K):
        raise ValueError('train_idx / test_idx: one row per model (%d)' % K)
    if M_want is not None:
        if not M <= int(M_want) <= L.VAR_MAX_REGRESSORS:
            raise ValueError('M=%d: the models need %d rows, at most %d' % (M_want, M, L.VAR_MAX_REGRESSORS))
        M = int(M_want)
    if S_want is not None:
        if int(S_want) < S_max:
            raise ValueError('S_max=%d: the models forecast up to %d rows' % (S_want, S_max))
        S_max = int(S_want)
    dev = days.device
    if models is None:
        table, nbytes = var_models(lags, ridges, train_n, test_n, origins, d)
        models = (table, var_models_device(table, dev), nbytes)
    table, table_dev, nbytes = models
    if workspace is None:
        workspace = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=dev)
    shapes = var_fit_shapes(K, d, M, S_max, test_stride)
    res = {}
    for name in VAR_OUTPUTS:
        if (name == 'future' and not want_future) or (name == 'per_day' and not want_per_day):
            res[name] = None
        elif out is not None and name in out:
            t = out[name]
            if tuple(t.shape) != shapes[name][0] or t.dtype != shapes[name][1] or not t.is_cuda or not t.is_contiguous():
                raise ValueError('out[%r]: expected a contiguous %s %s device tensor' % (name, shapes[name][0], shapes[name][1]))
            res[name] = t
        else:
            res[name] = torch.empty(shapes[name][0], dtype=shapes[name][1], device=dev)
    fit = L.VarFitStruct()
    fit.days, fit.models_host, fit.models = days.data_ptr(), C.addressof(table), table_dev.data_ptr()
    fit.train_idx, fit.test_idx = train_idx.data_ptr(), _ptr(test_idx)
    for name in VAR_OUTPUTS:
        setattr(fit, name, _ptr(res[name]))
    fit.workspace, fit.workspace_bytes = workspace.data_ptr(), workspace.numel() * workspace.element_size()
    fit.stream = _stream()
    fit.D, fit.Hd, fit.d, fit.K, fit.train_stride, fit.test_stride, fit.M, fit.S_max = D, Hd, d, K, int(train_idx.shape[1]), test_stride, M, S_max
    L.check(L.lib().mfg_var_fit_pop(C.byref(fit)), 'mfg_var_fit_pop')
    return res


RNN_OPTIMIZERS = {'adam': L.RNN_ADAM, 'sgd': L.RNN_SGD}


def rnn_weight_count(H, d):
    """W(H, d) = 4H (d + H + 1) + d (H + 1): the packed weights Wx [4H, d] | Wh [4H, H] | b [4H] | Wo [d, H] | bo [d]."""
    return 4 * H * (d + H + 1) + d * (H + 1)


def rnn_check_count(epochs, n_val, eval_every):
    """The held-out checks of a model: after every eval_every-th epoch and after the last; none without validation days."""
    return -(-int(epochs) // int(eval_every)) if n_val > 0 else 0


def check_rnn_fit_args(days_shape, hidden, epochs, lrs, wds, clips, train_n, val_n, test_n, optimizer='adam', eval_every=1,
                       train_stride=None, val_stride=None, test_stride=None):
    """The argument rules of rnn_fit_pop that need no GPU (ValueError), the limits of mfg_rnn_fit_pop: days [D, Hd, d] with
    2 <= Hd <= 64 and 2 <= d <= 64; per model a hidden size that is a multiple of 4 in [4, 64], 1 to 65 535 epochs, 1 to 64
    training and 0 to 64 validation / test days (within the index tables' strides when given), lr finite and > 0, wd and clip
    finite and >= 0; optimizer 'adam' or 'sgd', eval_every >= 1.  Returns (K, D, Hd, d, W_max, E_max, C_max): the largest
    weight count, epochs and number of held-out checks."""
    import math
    if len(days_shape) != 3:
        raise ValueError('days: expected [D, Hd, d], got %s' % (tuple(days_shape),))
    D, Hd, d = (int(s) for s in days_shape)
    if D < 1:
        raise ValueError('days: no day')
    if not 2 <= Hd <= L.RNN_MAX_HOURS:
        raise ValueError('Hd=%d: a day has 2 to %d rows' % (Hd, L.RNN_MAX_HOURS))
    if not 2 <= d <= L.RNN_MAX_D:
        raise ValueError('d=%d: the RNN population covers 2 <= d <= %d' % (d, L.RNN_MAX_D))
    if optimizer not in RNN_OPTIMIZERS:
        raise ValueError("optimizer=%r: 'adam' or 'sgd'" % (optimizer,))
    if isinstance(eval_every, bool) or int(eval_every) != eval_every or eval_every < 1:
        raise ValueError('eval_every=%r: a whole number >= 1' % (eval_every,))
    cols = [list(c) for c in (hidden, epochs, lrs, wds, clips, train_n, val_n, test_n)]
    K = len(cols[0])
    if K < 1:
        raise ValueError('no models')
    if K > L.POP_MAX_K:
        raise ValueError('%d models: at most %d in one call (MFG_POP_MAX_K)' % (K, L.POP_MAX_K))
    if any(len(c) != K for c in cols):
        raise ValueError('hidden, epochs, lrs, wds, clips, train_n, val_n and test_n must have one entry per model (%d)' % K)
    W_max = E_max = C_max = 0
    for k, (H, E, lr, wd, clip, ntr, nva, nte) in enumerate(zip(*cols)):
        H, E, ntr, nva, nte = int(H), int(E), int(ntr), int(nva), int(nte)
        lr, wd, clip = float(lr), float(wd), float(clip)
        if not 4 <= H <= L.RNN_MAX_HIDDEN or H % 4:
            raise ValueError('model %d: hidden=%d, a multiple of 4 in [4, %d]' % (k, H, L.RNN_MAX_HIDDEN))
        if not 1 <= E <= L.RNN_MAX_EPOCHS:
            raise ValueError('model %d: epochs=%d outside [1, %d]' % (k, E, L.RNN_MAX_EPOCHS))
        if not 1 <= ntr <= L.RNN_MAX_DAYS or (train_stride is not None and ntr > train_stride):
            raise ValueError('model %d: %d training days, a model has 1 to %d (and train_idx holds them)' % (k, ntr, L.RNN_MAX_DAYS))
        if not 0 <= nva <= L.RNN_MAX_DAYS or (val_stride is not None and nva > val_stride):
            raise ValueError('model %d: %d validation days, a model has 0 to %d (and val_idx holds them)' % (k, nva, L.RNN_MAX_DAYS))
        if not 0 <= nte <= L.RNN_MAX_DAYS or (test_stride is not None and nte > test_stride):
            raise ValueError('model %d: %d test days, a model has 0 to %d (and test_idx holds them)' % (k, nte, L.RNN_MAX_DAYS))
        if not (lr > 0.0 and math.isfinite(lr)):
            raise ValueError('model %d: lr=%r must be finite and > 0' % (k, lr))
        if not (wd >= 0.0 and math.isfinite(wd)):
            raise ValueError('model %d: wd=%r must be finite and >= 0' % (k, wd))
        if not (clip >= 0.0 and math.isfinite(clip)):
            raise ValueError('model %d: clip=%r must be finite and >= 0' % (k, clip))
        W_max, E_max = max(W_max, rnn_weight_count(H, d)), max(E_max, E)
        C_max = max(C_max, rnn_check_count(E, nva, eval_every))
    return K, D, Hd, d, W_max, E_max, C_max


def rnn_models(hidden, epochs, lrs, wds, clips, train_n, val_n, test_n, d, Hd):
    """The host table of mfg_rnn_fit_pop: (an array of K _lib.RnnModelStruct with ws_offset laid out by
    mfg_rnn_fit_workspace_bytes, the workspace bytes of the call).  Needs the library, no GPU."""
    K = len(hidden)
    table = (L.RnnModelStruct * K)()
    for k in range(K):
        t = table[k]
        t.hidden, t.epochs, t.n_train, t.n_val, t.n_test = int(hidden[k]), int(epochs[k]), int(train_n[k]), int(val_n[k]), int(test_n[k])
        t.lr, t.wd, t.clip = float(lrs[k]), float(wds[k]), float(clips[k])
    nbytes = int(L.lib().mfg_rnn_fit_workspace_bytes(K, table, int(d), int(Hd)))
    if nbytes == 0:
        raise ValueError('rnn_models: a record, d or Hd outside the limits of mfg_rnn_fit_pop')
    return table, nbytes


def rnn_models_device(table, device):
    """The device copy of an rnn_models table (a uint8 tensor of 56 K bytes)."""
    return var_models_device(table, device)


RNN_OUTPUTS = ('weights', 'loss', 'val', 'best_epoch', 'future', 'per_day', 'metrics', 'status')


def rnn_fit_shapes(K, Hd, d, W_max, E_max, C_max, test_stride):
    """name -> (shape, dtype) of the outputs of rnn_fit_pop."""
    f64 = torch.float64
    return {'weights': ((K, W_max), f64), 'loss': ((K, E_max), f64), 'val': ((K, C_max), f64), 'best_epoch': ((K,), torch.int32),
            'future': ((K, test_stride, Hd, d), f64), 'per_day': ((K, test_stride, 4), f64), 'metrics': ((K, 8), f64),
            'status': ((K,), torch.int32)}


def rnn_fit_pop(days, w0, hidden, epochs, lrs, wds, clips, train_idx, train_n, val_idx=None, val_n=None, test_idx=None, test_n=None,
                *, optimizer='adam', eval_every=1, out=None, workspace=None, models=None, E_max=None, C_max=None):
    """K one-layer LSTMs with a softmax head trained, selected on held-out days, forecast and scored in the two launches of one
    call (mfg_rnn_fit_pop; the model and every definition are in include/mfg_hip.h).  days [D, Hd, d] fp64 on the device;
    w0 [K, W_max] fp64 on the device, the packed initial weights of each model in the first W(H, d) entries of its row;
    hidden, epochs, lrs, wds, clips, train_n, val_n, test_n: K host values each; train_idx [K, >= max train_n], val_idx and
    test_idx int32 device tensors of day indices (None: no model has such a day).  Returns a dict of device tensors: weights
    [K, W_max] (the selected iterate), loss [K, E_max], val [K, C_max], best_epoch [K] int32, future [K, test_stride, Hd, d],
    per_day [K, test_stride, 4], metrics [K, 8], status [K] int32.  out / workspace / models: preallocated outputs (a dict by
    name), the scratch buffer and the (host table, device copy, bytes) of rnn_models / rnn_models_device -- then the call
    allocates nothing.  E_max / C_max: columns of loss / val when more than this call's models need (a chunk of a larger
    population)."""
    import ctypes as C
    _chk_f64(days, 'days')
    _chk_f64(w0, 'w0')
    as_list = lambda x: x.tolist() if hasattr(x, 'tolist') else list(x)
    K0 = len(as_list(hidden))
    val_n = [0] * K0 if val_n is None else val_n
    test_n = [0] * K0 if test_n is None else test_n
    hidden, epochs, lrs, wds, clips, train_n, val_n, test_n = (as_list(x) for x in (hidden, epochs, lrs, wds, clips, train_n, val_n, test_n))
    strides = []
    for name, t in (('train_idx', train_idx), ('val_idx', val_idx), ('test_idx', test_idx)):
        if t is None:
            if name == 'train_idx':
                raise ValueError('train_idx: every model has training days')
            strides.append(0)
            continue
        _chk_i32(t, name)
        if t.dim() != 2 or int(t.shape[0]) != K0:
            raise ValueError('%s: expected [K = %d, days], got %s' % (name, K0, tuple(t.shape)))
        strides.append(int(t.shape[1]))
    K, D, Hd, d, W_max, E_need, C_need = check_rnn_fit_args(days.shape, hidden, epochs, lrs, wds, clips, train_n, val_n, test_n,
                                                            optimizer, eval_every, *strides)
    if w0.dim() != 2 or int(w0.shape[0]) != K or int(w0.shape[1]) < W_max:
        raise ValueError('w0: expected [K = %d, >= %d], got %s' % (K, W_max, tuple(w0.shape)))
    W_max = int(w0.shape[1])
    if E_max is not None and int(E_max) < E_need:
        raise ValueError('E_max=%d: the models train up to %d epochs' % (E_max, E_need))
    if C_max is not None and int(C_max) < C_need:
        raise ValueError('C_max=%d: the models make up to %d checks' % (C_max, C_need))
    E_max, C_max = int(E_need if E_max is None else E_max), int(C_need if C_max is None else C_max)
    dev = days.device
    if models is None:
        table, nbytes = rnn_models(hidden, epochs, lrs, wds, clips, train_n, val_n, test_n, d, Hd)
        models = (table, rnn_models_device(table, dev), nbytes)
    table, table_dev, nbytes = models
    if workspace is None:
        workspace = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=dev)
    shapes = rnn_fit_shapes(K, Hd, d, W_max, E_max, C_max, strides[2])
    res = {}
    for name in RNN_OUTPUTS:
        if out is not None and name in out:
            t = out[name]
            if tuple(t.shape) != shapes[name][0] or t.dtype != shapes[name][1] or not t.is_cuda or not t.is_contiguous():
                raise ValueError('out[%r]: expected a contiguous %s %s device tensor' % (name, shapes[name][0], shapes[name][1]))
            res[name] = t
        else:
            res[name] = torch.empty(shapes[name][0], dtype=shapes[name][1], device=dev)
    fit = L.RnnFitStruct()
    fit.days, fit.models_host, fit.models = days.data_ptr(), C.addressof(table), table_dev.data_ptr()
    fit.train_idx, fit.val_idx, fit.test_idx, fit.w0 = train_idx.data_ptr(), _ptr(val_idx), _ptr(test_idx), w0.data_ptr()
    for name in RNN_OUTPUTS:
        setattr(fit, name, res[name].data_ptr() if res[name].numel() else None)
    fit.workspace, fit.workspace_bytes = workspace.data_ptr(), workspace.numel() * workspace.element_size()
    fit.stream = _stream()
    fit.D, fit.Hd, fit.d, fit.K = D, Hd, d, K
    fit.train_stride, fit.val_stride, fit.test_stride = strides
    fit.W_max, fit.E_max, fit.C_max = W_max, E_max, C_max
    fit.optimizer, fit.eval_every = RNN_OPTIMIZERS[optimizer], int(eval_every)
    L.check(L.lib().mfg_rnn_fit_pop(C.byref(fit)), 'mfg_rnn_fit_pop')
    return res


def policy_logpdf(pi, P, thetas, shift, alpha_scale=1.0, alpha_floor=0.0, p_floor=0.0):
    """log q_k(P_n | pi_n) [N,K] of the product-Dirichlet policy under K thetas (ac_irl.py:270-289, :324-379)."""
    _chk_f32(pi, 'pi'); _chk_f32(P, 'P'); _chk_f64(thetas, 'thetas')
    N, d = pi.shape
    if P.shape != (N, d, d):
        raise ValueError('P must be [N,d,d]')
    K = thetas.numel()
    out = torch.empty(N, K, dtype=torch.float64, device=pi.device)
    L.check(L.lib().mfg_policy_logpdf(pi.data_ptr(), P.data_ptr(), N, d, thetas.data_ptr(), K, float(shift),
                                      float(alpha_scale), float(alpha_floor), float(p_floor), out.data_ptr(), _stream()),
            'mfg_policy_logpdf')
    return out


def traj_log_z_pop(state, action, rows, thetas, shifts, log_start, alpha_scale=1.0, alpha_floor=1.0 + 1e-6, p_floor=0.0, out=None,
                   scratch=None):
    """mfg_traj_log_z_pop: ln z of the listed PHYSICAL rows of a trajectory store under K learners' policy lists, in one launch
    (ac_irl.py:292-379 calc_z in log space; the defaults are calc_z's alpha_scale 1 and alpha floor 1 + 1e-6):
        out[k, row] = ln n_pol - logsumexp_p( sum_t ln q_{thetas[k, p]}(a_t; s_t) - log_start ).
    state [cap, T, d] / action [cap, T, d, d] (one store shared by the K learners) or [K, cap, T, d] / [K, cap, T, d, d] (one
    store per learner); thetas [K, n_pol] and shifts [K] fp64 device tensors; rows: distinct ints in [0, cap).  Returns out
    [K, cap] fp64 (given: rows not listed keep their values; created: they hold NaN).  A trajectory whose every density is 0 (an
    exact zero in P with p_floor = 0) gets +inf."""
    import ctypes as C
    _chk_f32(state, 'state'); _chk_f32(action, 'action'); _chk_f64(thetas, 'thetas'); _chk_f64(shifts, 'shifts')
    if thetas.dim() != 2 or thetas.shape[1] < 1:
        raise ValueError('thetas: expected [K, n_pol]')
    K, n_pol = thetas.shape
    if tuple(shifts.shape) != (K,):
        raise ValueError('shifts: expected [%d]' % K)
    per_learner = state.dim() == 4
    if state.dim() not in (3, 4) or (per_learner and state.shape[0] != K):
        raise ValueError('state: expected [cap, T, d] or [%d, cap, T, d]' % K)
    cap, T, d = state.shape[-3:]
    if tuple(action.shape) != tuple(state.shape) + (d,):
        raise ValueError('action: expected %s' % (tuple(state.shape) + (d,),))
    if out is None:
        out = torch.full((K, cap), float('nan'), dtype=torch.float64, device=state.device)
    elif tuple(out.shape) != (K, cap):
        raise ValueError('out: expected [%d, %d]' % (K, cap))
    _chk_f64(out, 'out')
    n = len(rows)
    rw = (C.c_int32 * max(n, 1))(*[int(r) for r in rows])
    if scratch is None:
        scratch = torch.empty(max(n, 1), dtype=torch.int32, device=state.device)
    L.check(L.lib().mfg_traj_log_z_pop(state.data_ptr(), action.data_ptr(), int(cap), rw, n, int(T), int(d), thetas.data_ptr(),
                                       int(n_pol), shifts.data_ptr(), int(K), int(per_learner), float(alpha_scale),
                                       float(alpha_floor), float(p_floor), float(log_start), out.data_ptr(), scratch.data_ptr(),
                                       scratch.numel() * scratch.element_size(), _stream()), 'mfg_traj_log_z_pop')
    return out


def reward_net_supported(net) -> bool:
    """True when networks.RewardNet `net` fits the HIP forward kernel (d <= 32, f1 = 1, f2 <= 2, n_fc <= 32)."""
    k1, k2 = net.conv1.kernel_size[0], net.conv2.kernel_size[0]
    return (net.conv1.out_channels == 1 and net.conv2.out_channels <= 2 and net.d <= 32 and k1 % 2 == 1 and k2 % 2 == 1
            and k1 <= 7 and k2 <= 7 and net.fc3.out_features <= 32 and net.fc4.out_features <= 32
            and next(net.parameters()).dtype == torch.float32 and next(net.parameters()).is_cuda)


def reward_net_forward(net, state, action, dropout=None, seed=0, sample_offset=0):
    """r(state, action) [B] with the weights of a networks.RewardNet, one HIP launch (ac_irl.py:683 batched).
    dropout: None -> follow the module (active when the variant has dropout and dropout_always/training)."""
    _chk_f32(state, 'state'); _chk_f32(action, 'action')
    B, d = state.shape
    if dropout is None:
        dropout = net.use_dropout and (net.dropout_always or net.training)
    keep = float(net.keep_prob) if dropout else 1.0
    out = torch.empty(B, dtype=torch.float32, device=state.device)
    def P(t):
        if not t.is_contiguous():
            raise ValueError('reward net parameters must be contiguous')
        return t.data_ptr()
    L.check(L.lib().mfg_reward_net_forward(
        state.data_ptr(), action.data_ptr(), B, d, net.conv1.kernel_size[0], net.conv2.out_channels,
        net.conv2.kernel_size[0], net.fc3.out_features, net.fc4.out_features, P(net.conv1.weight), P(net.conv1.bias),
        P(net.conv2.weight), P(net.conv2.bias), P(net.fc3.weight), P(net.fc3.bias), P(net.fc4.weight), P(net.fc4.bias),
        P(net.out.weight), P(net.out.bias), keep, int(seed), int(sample_offset), out.data_ptr(), _stream()),
        'mfg_reward_net_forward')
    return out


def backward_value(P_seq, want_jsd=True):
    """mfg_synthetic backward recursion on actions P_seq [B,T,d,d]: returns V [B,T+1,d], diff_l1 [B,T], diff_jsd [B,T]|None."""
    _chk_f32(P_seq, 'P_seq')
    B, T, d, _ = P_seq.shape
    V = torch.empty(B, T + 1, d, dtype=torch.float64, device=P_seq.device)
    l1 = torch.empty(B, T, dtype=torch.float64, device=P_seq.device)
    js = torch.empty(B, T, dtype=torch.float64, device=P_seq.device) if want_jsd else None
    L.check(L.lib().mfg_backward_value(P_seq.data_ptr(), B, T, d, V.data_ptr(), l1.data_ptr(), _ptr(js), _stream()),
            'mfg_backward_value')
    return V, l1, js


DEMOS_OUTPUTS = ('state', 'action', 'counts', 'moves', 'order', 'present', 'left', 'entered', 'status')
DEMOS_REQUIRED = ('order', 'status')


def check_demos_args(topic_shape, C, d, width=None, order='first_hour', order_given_shape=None, empty_row='uniform',
                     lds_update='plain'):
    """The argument rules of demos_from_logs that need no GPU (ValueError), the limits of mfg_demos_from_logs: topic [N, H, U]
    with N >= 1, H >= 2, 1 <= U <= 2^31 - 1; 1 <= C <= 4096; 1 <= d <= width <= min(C, 64) (width None: d); order one of
    'first_hour', 'total', 'given', the last with a table [N, C] or [1, C]; empty_row 'uniform' or 'identity'.  Returns
    (N, H, U, C, d, width)."""
    if len(topic_shape) != 3:
        raise ValueError('topic: expected [N, H, U] (day, hour, agent), got %s' % (tuple(topic_shape),))
    N, H, U = (int(s) for s in topic_shape)
    C, d = int(C), int(d)
    width = d if width is None else int(width)
    if N < 1 or H < 2:
        raise ValueError('topic [%d, %d, %d]: at least one day and two hours' % (N, H, U))
    if not 1 <= U <= 2 ** 31 - 1:
        raise ValueError('U=%d agents outside [1, 2^31 - 1]' % U)
    if not 1 <= C <= L.DEMOS_MAX_C:
        raise ValueError('C=%d categories outside [1, %d] (MFG_DEMOS_MAX_C)' % (C, L.DEMOS_MAX_C))
    if not 1 <= d <= width <= C:
        raise ValueError('d=%d, width=%d, C=%d: 1 <= d <= width <= C' % (d, width, C))
    if width > L.DEMOS_MAX_WIDTH:
        raise ValueError('width=%d: demonstrations cover width <= %d (as the populations do)' % (width, L.DEMOS_MAX_WIDTH))
    if order not in L.DEMOS_ORDERS:
        raise ValueError('order=%r: one of %s' % (order, sorted(L.DEMOS_ORDERS)))
    if empty_row not in L.DEMOS_EMPTY_ROWS:
        raise ValueError('empty_row=%r: one of %s' % (empty_row, sorted(L.DEMOS_EMPTY_ROWS)))
    if lds_update not in L.DEMOS_LDS_UPDATES:
        raise ValueError('lds_update=%r: one of %s' % (lds_update, sorted(L.DEMOS_LDS_UPDATES)))
    if order == 'given':
        if order_given_shape is None or tuple(order_given_shape) not in ((N, C), (1, C)):
            raise ValueError('order=\'given\' needs order_given [%d, %d] or [1, %d], got %s'
                             % (N, C, C, None if order_given_shape is None else tuple(order_given_shape)))
    elif order_given_shape is not None:
        raise ValueError('order_given is read with order=\'given\' only')
    return N, H, U, C, d, width


def demos_shapes(N, H, C, d, width):
    """name -> (shape, dtype) of the outputs of demos_from_logs."""
    f32, i32 = torch.float32, torch.int32
    return {'state': ((N, H, d), f32), 'action': ((N, H - 1, d, d), f32), 'counts': ((N, H, width), i32),
            'moves': ((N, H - 1, width, width), i32), 'order': ((N, C), i32), 'present': ((N, H), i32),
            'left': ((N, H - 1, width), i32), 'entered': ((N, H - 1, width), i32), 'status': ((N,), i32)}


def demos_workspace_bytes(N, H, C, width):
    """mfg_demos_workspace_bytes: needs the library, no GPU."""
    nbytes = int(L.lib().mfg_demos_workspace_bytes(int(N), int(H), int(C), int(width)))
    if nbytes == 0:
        raise ValueError('demos_workspace_bytes: N=%d, H=%d, C=%d, width=%d outside the limits of mfg_demos_from_logs' % (N, H, C, width))
    return nbytes


def _demos_outputs(shapes, names, out, want, dev):
    res = {}
    for name in names:
        if want is not None and name not in want and name not in DEMOS_REQUIRED:
            res[name] = None
        elif out is not None and name in out:
            t = out[name]
            if tuple(t.shape) != shapes[name][0] or t.dtype != shapes[name][1] or not t.is_cuda or not t.is_contiguous():
                raise ValueError('out[%r]: expected a contiguous %s %s device tensor' % (name, shapes[name][0], shapes[name][1]))
            res[name] = t
        else:
            res[name] = torch.empty(shapes[name][0], dtype=shapes[name][1], device=dev)
    return res


def demos_from_logs(topic, C, d, *, width=None, order='first_hour', order_given=None, empty_row='uniform', out=None,
                    workspace=None, want=None, lds_update='plain', groups=0):
    """States and actions counted from an agent log (mfg_demos_from_logs; the definitions are in include/mfg_hip.h).  topic
    [N, H, U] int32 on the device: the category in [0, C) of agent u at hour h of day n, negative when absent.  Categories are
    ranked per day by the first hour's popularity ('first_hour', the reference's reorder), once for all days ('total') or by
    order_given (int32 device tensor [N, C] or [1, C] of ranks, -1 drops); the top `width` (default d) are the recorded set, the
    top d the model's topics.  Returns a dict of device tensors: state [N, H, d] and action [N, H-1, d, d] fp32, counts
    [N, H, width], moves [N, H-1, width, width], order [N, C], present [N, H], left and entered [N, H-1, width], status [N]
    int32.  want: the names to compute (None: all; order and status always) -- the others are None.  out / workspace:
    preallocated outputs (a dict by name) and the scratch buffer (demos_workspace_bytes) -- then the call allocates nothing.
    lds_update ('plain' / 'combine') and groups (workgroups of the counting pass per day, 0: from the device) change no output."""
    import ctypes as C_
    _chk_i32(topic, 'topic')
    if order_given is not None:
        _chk_i32(order_given, 'order_given')
    N, H, U, C, d, width = check_demos_args(topic.shape, C, d, width, order, None if order_given is None else order_given.shape,
                                            empty_row, lds_update)
    if want is not None and not set(want) <= set(DEMOS_OUTPUTS):
        raise ValueError('want: unknown outputs %s' % sorted(set(want) - set(DEMOS_OUTPUTS)))
    dev = topic.device
    nbytes = demos_workspace_bytes(N, H, C, width)
    if workspace is None:
        workspace = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=dev)
    res = _demos_outputs(demos_shapes(N, H, C, d, width), DEMOS_OUTPUTS, out, want, dev)
    f = L.DemosStruct()
    f.topic, f.order_given = topic.data_ptr(), _ptr(order_given)
    for name in DEMOS_OUTPUTS:
        setattr(f, name, _ptr(res[name]))
    f.workspace, f.workspace_bytes, f.stream = workspace.data_ptr(), workspace.numel() * workspace.element_size(), _stream()
    f.U, f.N, f.H, f.C, f.d, f.width = U, N, H, C, d, width
    f.order_mode, f.empty_row, f.lds_update = L.DEMOS_ORDERS[order], L.DEMOS_EMPTY_ROWS[empty_row], L.DEMOS_LDS_UPDATES[lds_update]
    f.order_given_rows = 0 if order_given is None else int(order_given.shape[0])
    f.groups = int(groups)
    L.check(L.lib().mfg_demos_from_logs(C_.byref(f)), 'mfg_demos_from_logs')
    return res


DEMOS_MOVES_OUTPUTS = ('state', 'action', 'present', 'left', 'entered', 'status')


def check_demos_moves_args(counts_shape, moves_shape, d=None, empty_row='uniform'):
    """The argument rules of demos_from_moves that need no GPU: counts [N, H, width], moves [N, H-1, width, width], H >= 2,
    1 <= d <= width <= 64 (d None: width).  Returns (N, H, d, width)."""
    if len(counts_shape) != 3:
        raise ValueError('counts: expected [N, H, width], got %s' % (tuple(counts_shape),))
    N, H, width = (int(s) for s in counts_shape)
    if N < 1 or H < 2:
        raise ValueError('counts [%d, %d, %d]: at least one day and two hours' % (N, H, width))
    if tuple(moves_shape) != (N, H - 1, width, width):
        raise ValueError('moves: expected [%d, %d, %d, %d], got %s' % (N, H - 1, width, width, tuple(moves_shape)))
    d = width if d is None else int(d)
    if not 1 <= d <= width:
        raise ValueError('d=%d, width=%d: 1 <= d <= width' % (d, width))
    if width > L.DEMOS_MAX_WIDTH:
        raise ValueError('width=%d: demonstrations cover width <= %d (as the populations do)' % (width, L.DEMOS_MAX_WIDTH))
    if empty_row not in L.DEMOS_EMPTY_ROWS:
        raise ValueError('empty_row=%r: one of %s' % (empty_row, sorted(L.DEMOS_EMPTY_ROWS)))
    return N, H, d, width


def demos_from_moves(counts, moves, d=None, *, empty_row='uniform', out=None, want=None):
    """The second mode of mfg_demos_from_logs: states and actions from integer tables that exist already -- counts [N, H, width]
    and moves [N, H-1, width, width] int32 on the device, e.g. (counts, counts_next) stacked and the moves of
    agents_step_pop(..., want_moves=True) with every member a day of H = 2.  Returns state, action, present, left, entered and
    status as demos_from_logs does (counts and moves are the inputs); an hour with a negative entry (a failed member) gives NaN
    rows and status bit _lib.DEMOS_FAILED."""
    import ctypes as C_
    _chk_i32(counts, 'counts'); _chk_i32(moves, 'moves')
    N, H, d, width = check_demos_moves_args(counts.shape, moves.shape, d, empty_row)
    if want is not None and not set(want) <= set(DEMOS_MOVES_OUTPUTS):
        raise ValueError('want: unknown outputs %s' % sorted(set(want) - set(DEMOS_MOVES_OUTPUTS)))
    shapes = demos_shapes(N, H, width, d, width)
    res = _demos_outputs(shapes, DEMOS_MOVES_OUTPUTS, out, want, counts.device)
    f = L.DemosStruct()
    for name in DEMOS_MOVES_OUTPUTS:
        setattr(f, name, _ptr(res[name]))
    f.counts, f.moves, f.stream = counts.data_ptr(), moves.data_ptr(), _stream()
    f.N, f.H, f.C, f.d, f.width, f.empty_row = N, H, width, d, width, L.DEMOS_EMPTY_ROWS[empty_row]
    L.check(L.lib().mfg_demos_from_logs(C_.byref(f)), 'mfg_demos_from_logs')
    res.update(counts=counts, moves=moves)
    return res


DEMOS_BOOT_OUTPUTS = ('state', 'action', 'counts', 'moves', 'present', 'left', 'entered', 'status')


def check_demos_boot_args(topic_shape, rank_shape, C, d, R, width=None, unit='agent_day', day_offset=0, empty_row='uniform',
                          groups=0):
    """The argument rules of demos_bootstrap that need no GPU (ValueError), the limits of mfg_demos_bootstrap: those of
    demos_from_logs with a given order (rank [N, C] or [1, C]), 1 <= R <= 1024, 12 U <= 2^31 - 1 (a weighted cell must fit
    int32), unit 'agent_day' or 'agent', day_offset + n in [0, 2^48).  Returns (N, H, U, C, d, width)."""
    if rank_shape is None:
        raise ValueError('rank: the ranking of the recorded sample is required, [N, C] or [1, C]')
    N, H, U, C, d, width = check_demos_args(topic_shape, C, d, width, 'given', tuple(rank_shape), empty_row)
    R = int(R)
    if not 1 <= R <= L.DEMOS_BOOT_MAX_R:
        raise ValueError('R=%d replicates outside [1, %d] (MFG_DEMOS_BOOT_MAX_R)' % (R, L.DEMOS_BOOT_MAX_R))
    if 12 * U > 2 ** 31 - 1:
        raise ValueError('U=%d agents: a cell weighted up to 12 times must fit int32, 12 U <= 2^31 - 1' % U)
    if R * N * H > 2 ** 31 - 1:
        raise ValueError('R N H = %d > 2^31 - 1' % (R * N * H))
    if unit not in L.DEMOS_UNITS:
        raise ValueError('unit=%r: one of %s' % (unit, sorted(L.DEMOS_UNITS)))
    if unit == 'agent_day' and not 0 <= int(day_offset) <= 2 ** 48 - N:
        raise ValueError('day_offset=%d: day_offset + n must lie in [0, 2^48)' % day_offset)
    if int(groups) < 0:
        raise ValueError('groups=%d < 0' % groups)
    return N, H, U, C, d, width


def demos_boot_shapes(R, N, H, d, width):
    """name -> (shape, dtype) of the outputs of demos_bootstrap: those of demos_from_logs (but order) with a leading R."""
    return {n: ((R,) + s, t) for n, (s, t) in demos_shapes(N, H, 1, d, width).items() if n != 'order'}


def demos_bootstrap_workspace_bytes(R, N, H, C, width):
    """mfg_demos_bootstrap_workspace_bytes: needs the library, no GPU."""
    nbytes = int(L.lib().mfg_demos_bootstrap_workspace_bytes(int(R), int(N), int(H), int(C), int(width)))
    if nbytes == 0:
        raise ValueError('demos_bootstrap_workspace_bytes: R=%d, N=%d, H=%d, C=%d, width=%d outside the limits of '
                         'mfg_demos_bootstrap' % (R, N, H, C, width))
    return nbytes


def demos_bootstrap(topic, rank, C, d, R, seed=0, *, width=None, unit='agent_day', day_offset=0, empty_row='uniform', groups=0,
                    out=None, workspace=None, want=None):
    """R Poisson-bootstrap replicates of the demonstrations of a log (mfg_demos_bootstrap; the definitions are in
    include/mfg_hip.h): topic [N, H, U] int32 as demos_from_logs, rank [N, C] or [1, C] int32 the ranks of the categories (the
    recorded sample's, -1 drops).  In replicate r agent u of day n counts w ~ Poisson(1) times at every hour, w from the
    counter-based generator under `seed`; unit 'agent_day' draws per (day_offset + n, u), 'agent' per u for all days.  Returns a
    dict of device tensors with a leading R: state, action, counts, moves, present, left, entered, status [R, N].  want / out /
    workspace as demos_from_logs; groups changes no output."""
    import ctypes as C_
    _chk_i32(topic, 'topic')
    if rank is not None:
        _chk_i32(rank, 'rank')
    N, H, U, C, d, width = check_demos_boot_args(topic.shape, None if rank is None else rank.shape, C, d, R, width, unit, day_offset,
                                                 empty_row, groups)
    R = int(R)
    if want is not None and not set(want) <= set(DEMOS_BOOT_OUTPUTS):
        raise ValueError('want: unknown outputs %s' % sorted(set(want) - set(DEMOS_BOOT_OUTPUTS)))
    dev = topic.device
    nbytes = demos_bootstrap_workspace_bytes(R, N, H, C, width)
    if workspace is None:
        workspace = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=dev)
    res = _demos_outputs(demos_boot_shapes(R, N, H, d, width), DEMOS_BOOT_OUTPUTS, out, want, dev)
    f = L.DemosBootStruct()
    f.topic, f.rank = topic.data_ptr(), rank.data_ptr()
    for name in DEMOS_BOOT_OUTPUTS:
        setattr(f, name, _ptr(res[name]))
    f.workspace, f.workspace_bytes, f.stream = workspace.data_ptr(), workspace.numel() * workspace.element_size(), _stream()
    f.U, f.seed, f.day_offset = U, int(seed) & (2 ** 64 - 1), int(day_offset)
    f.N, f.H, f.C, f.d, f.width, f.R = N, H, C, d, width, R
    f.rank_rows, f.unit, f.empty_row, f.groups = int(rank.shape[0]), L.DEMOS_UNITS[unit], L.DEMOS_EMPTY_ROWS[empty_row], int(groups)
    L.check(L.lib().mfg_demos_bootstrap(C_.byref(f)), 'mfg_demos_bootstrap')
    return res


def check_replicate_bands_args(x_shape, ranks):
    """The argument rules of replicate_bands that need no GPU: x [R, ...] with 1 <= R <= 1024, at most FORECAST_MAX_RANKS
    ranks, each in [0, R).  Returns (R, cells, ranks)."""
    if len(x_shape) < 1:
        raise ValueError('x: expected [R, ...]')
    R = int(x_shape[0])
    if not 1 <= R <= L.DEMOS_BOOT_MAX_R:
        raise ValueError('R=%d replicates outside [1, %d]' % (R, L.DEMOS_BOOT_MAX_R))
    ranks = [int(q) for q in ranks]
    if len(ranks) > L.FORECAST_MAX_RANKS:
        raise ValueError('%d ranks: at most %d order statistics per call (MFG_FORECAST_MAX_RANKS)' % (len(ranks), L.FORECAST_MAX_RANKS))
    if any(not 0 <= q < R for q in ranks):
        raise ValueError('ranks %s outside [0, %d)' % (ranks, R))
    cells = 1
    for s in x_shape[1:]:
        cells *= int(s)
    return R, cells, ranks


def replicate_bands(x, ranks=()):
    """Bands over the leading axis of x [R, ...] fp32 on the device (mfg_replicate_bands): (mean [...] fp64, std [...] fp64 with
    ddof 0, quant [Q, ...] fp32) per cell over its R values.  mean and std are sums in the order r = 0 .. R - 1 in fp64, every
    operation rounded on its own; quant[q] is the element of 0-based rank ranks[q] (not an interpolation; ranks may repeat and
    need not be sorted).  A cell with a NaN in any replicate is NaN in all three."""
    import ctypes as C_
    _chk_f32(x, 'x')
    R, cells, ranks = check_replicate_bands_args(tuple(x.shape), ranks)
    rest = tuple(x.shape[1:])
    mean = torch.empty(rest, dtype=torch.float64, device=x.device)
    std = torch.empty(rest, dtype=torch.float64, device=x.device)
    quant = torch.empty((len(ranks),) + rest, dtype=torch.float32, device=x.device)
    b = L.ReplicateBandsStruct()
    b.x, b.mean, b.std, b.quant, b.stream = x.data_ptr(), mean.data_ptr(), std.data_ptr(), quant.data_ptr() if ranks else None, _stream()
    b.cells, b.R, b.Q = cells, R, len(ranks)
    for q, rank in enumerate(ranks):
        b.ranks[q] = rank
    L.check(L.lib().mfg_replicate_bands(C_.byref(b)), 'mfg_replicate_bands')
    return mean, std, quant


MOVES_LOGLIK_OUTPUTS = ('ll', 'll_day', 'grad', 'grad_day', 'status')


def check_moves_loglik_args(state_shape, moves_shape, K, d, set_index_len=None):
    """The argument rules of moves_loglik_pop that need no GPU (ValueError), the limits of mfg_moves_loglik_pop: state [N, H, d]
    with moves [N, H-1, width, width], or both with a leading S (the data sets); 1 <= d <= 64, d <= width, H >= 2,
    1 <= K <= POP_MAX_K, set_index of K entries.  Returns (S, N, H, d, width)."""
    state_shape, moves_shape = tuple(int(s) for s in state_shape), tuple(int(s) for s in moves_shape)
    if len(state_shape) not in (3, 4) or len(moves_shape) != len(state_shape) + 1:
        raise ValueError('state %s / moves %s: expected [N, H, d] with [N, H-1, width, width], or both with a leading S'
                         % (state_shape, moves_shape))
    if len(state_shape) == 3:
        state_shape, moves_shape = (1,) + state_shape, (1,) + moves_shape
    S, N, H, ds = state_shape
    d, width, K = int(d), moves_shape[-1], int(K)
    if not 1 <= d <= L.MOVES_LOGLIK_MAX_D:
        raise ValueError('d=%d outside [1, %d]' % (d, L.MOVES_LOGLIK_MAX_D))
    if S < 1 or N < 1 or H < 2:
        raise ValueError('S=%d, N=%d, H=%d: at least one data set, one day and two hours' % (S, N, H))
    if ds != d:
        raise ValueError('state %s: the last axis is the policy\'s input, d=%d' % (state_shape, d))
    if moves_shape != (S, N, H - 1, width, width):
        raise ValueError('moves %s: expected %s' % (moves_shape, (S, N, H - 1, width, width)))
    if d > width:
        raise ValueError('d=%d > width=%d' % (d, width))
    if not 1 <= K <= L.POP_MAX_K:
        raise ValueError('K=%d policies: at least 1, at most %d in one call' % (K, L.POP_MAX_K))
    if N * (H - 1) > 2 ** 31 - 1:
        raise ValueError('N (H - 1) = %d > 2^31 - 1' % (N * (H - 1)))
    if set_index_len is not None and int(set_index_len) != K:
        raise ValueError('set_index: %d entries for K=%d policies' % (set_index_len, K))
    return S, N, H, d, width


def moves_loglik_workspace_bytes(K, S, N, H, d):
    """mfg_moves_loglik_workspace_bytes: needs the library, no GPU."""
    nbytes = int(L.lib().mfg_moves_loglik_workspace_bytes(int(K), int(S), int(N), int(H), int(d)))
    if nbytes == 0:
        raise ValueError('moves_loglik_workspace_bytes: K=%d, S=%d, N=%d, H=%d, d=%d outside the limits of mfg_moves_loglik_pop'
                         % (K, S, N, H, d))
    return nbytes


def moves_loglik_shapes(K, N, H):
    """name -> (shape, dtype) of the outputs of moves_loglik_pop."""
    return {'ll': ((K, N, H - 1), torch.float64), 'll_day': ((K, N), torch.float64), 'grad': ((K, N, H - 1, 3), torch.float64),
            'grad_day': ((K, N, 3), torch.float64), 'status': ((K, N), torch.int32)}


def moves_loglik_pop(state, moves, thetas, shifts, alpha_scales, d, set_index=None, grad=True, *, out=None, workspace=None):
    """The Dirichlet-multinomial log-likelihood of counted moves under K policies (mfg_moves_loglik_pop; the definitions are in
    include/mfg_hip.h): state [N, H, d] fp32 and moves [N, H-1, width, width] int32 (one data set), or [S, N, H, d] and
    [S, N, H-1, width, width] with set_index [K] int32, the data set of each policy (None: all 0; an entry outside [0, S) is
    marked on the device, status bit 3, and reads nothing).  thetas, shifts, alpha_scales [K] fp64 device tensors.  Returns a
    dict of device tensors: ll [K, N, H-1], ll_day [K, N], grad [K, N, H-1, 3], grad_day [K, N, 3] in the order (theta, shift,
    ln alpha_scale) -- both None with grad=False --, status [K, N] int32.  out: a dict of tensors to write into; workspace: a
    device buffer of at least moves_loglik_workspace_bytes bytes.  Nothing is synchronised."""
    import ctypes as C_
    _chk_f32(state, 'state')
    _chk_i32(moves, 'moves')
    for name, t in (('thetas', thetas), ('shifts', shifts), ('alpha_scales', alpha_scales)):
        _chk_f64(t, name)
    K = int(thetas.numel())
    if shifts.numel() != K or alpha_scales.numel() != K:
        raise ValueError('thetas, shifts, alpha_scales: %d, %d, %d entries' % (K, shifts.numel(), alpha_scales.numel()))
    if set_index is not None:
        _chk_i32(set_index, 'set_index')
    S, N, H, d, width = check_moves_loglik_args(state.shape, moves.shape, K, d, None if set_index is None else set_index.numel())
    dev = state.device
    nbytes = moves_loglik_workspace_bytes(K, S, N, H, d)
    if workspace is None:
        workspace = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=dev)
    res = {}
    for name, (shape, dtype) in moves_loglik_shapes(K, N, H).items():
        if not grad and name in ('grad', 'grad_day'):
            res[name] = None
            continue
        t = None if out is None else out.get(name)
        if t is None:
            t = torch.empty(shape, dtype=dtype, device=dev)
        elif not (t.is_cuda and t.dtype == dtype and t.is_contiguous() and tuple(t.shape) == shape):
            raise ValueError('out[%r]: expected a contiguous %s CUDA tensor of shape %s' % (name, dtype, shape))
        res[name] = t
    f = L.MovesLoglikStruct()
    f.state, f.moves, f.set_index = state.data_ptr(), moves.data_ptr(), _ptr(set_index)
    f.theta, f.shift, f.alpha_scale = thetas.data_ptr(), shifts.data_ptr(), alpha_scales.data_ptr()
    for name in MOVES_LOGLIK_OUTPUTS:
        setattr(f, name, _ptr(res[name]))
    f.workspace, f.workspace_bytes, f.stream = workspace.data_ptr(), workspace.numel() * workspace.element_size(), _stream()
    f.state_stride, f.moves_stride = N * H * d, N * (H - 1) * width * width
    f.N, f.H, f.d, f.width, f.sets, f.policies = N, H, d, width, S, K
    L.check(L.lib().mfg_moves_loglik_pop(C_.byref(f)), 'mfg_moves_loglik_pop')
    return res
