"""How probable the recorded moves are under a policy: the Dirichlet-multinomial (Polya) likelihood of the integer moves of a
Demonstrations (demos.from_logs, demos.from_moves) or of the replicates of a BootstrapDemonstrations, for K policies in one
call of the device kernel (ops.moves_loglik_pop, C ABI mfg_moves_loglik_pop: the definitions are in include/mfg_hip.h).

Under (theta, shift, alpha_scale) row i of the action is Dirichlet(a_i.) and the n_i agents of topic i each draw from that
row, so the moves of a row are Dirichlet-multinomial in closed form: no sampling, no p_floor (zeros are ordinary outcomes), the
finite-population noise is in the model, and the value is differentiable in theta, shift and alpha_scale.  On it stand
  loglik         the value, per transition and per day, with its gradient and the status bits;
  gridsearch     a deterministic grid search in the point order of population.grid_points, one call;
  fit            maximum likelihood for K starts in lock-step (Adam ascent on the device): the behaviour-cloning arm next to
                 the MFG, VAR and RNN arms;
  fit_bootstrap  one fit per bootstrap replicate: an error bar on the fitted parameters.
This is the project's, not the reference's: the reference has only the Dirichlet density of proportions (calc_pdf_action)."""
import numpy as np

from . import _lib as L

PARAMS = ('theta', 'shift', 'log_alpha_scale')       # the order of every gradient and of fit's parameter rows
ADAM_BETA1, ADAM_BETA2, ADAM_EPS = 0.9, 0.999, 1e-8
FIT_LR = 0.05
GRID_CHUNK = L.POP_MAX_K                             # policies of one call (more go in chunks: no output depends on it)


class LogLik:
    """The result of loglik (NumPy): ll [K, N, H-1] per transition, ll_day [K, N], grad_day [K, N, 3] in the order PARAMS,
    status [K, N] (bits _lib.MOVES_LOGLIK_*; 0 = a clean day), and `days`, the days of the demonstrations that the N columns
    are."""

    def __init__(self, ll, ll_day, grad_day, status, days):
        self.ll, self.ll_day, self.grad_day, self.status, self.days = ll, ll_day, grad_day, status, list(days)

    def _columns(self, days):
        if days is None:
            return list(range(len(self.days)))
        try:
            return [self.days.index(int(n)) for n in days]
        except ValueError:
            raise ValueError('days %s: not all among the evaluated days %s' % (list(days), self.days))

    def total(self, days=None):
        """[K]: the log-likelihood of the given days (None: all evaluated), the days' values added in order in fp64."""
        out = np.zeros(self.ll_day.shape[0])
        for c in self._columns(days):
            out = out + self.ll_day[:, c]
        return out

    def grad_total(self, days=None):
        """[K, 3]: the gradient of total(days) with respect to PARAMS."""
        out = np.zeros((self.ll_day.shape[0], 3))
        for c in self._columns(days):
            out = out + self.grad_day[:, c]
        return out


def _device(device):
    import torch
    return torch.device('cuda' if device is None else device)


def check_policy_args(thetas, shifts, alpha_scales):
    """thetas, shifts, alpha_scales as three fp64 arrays of one length K >= 1 (scalars broadcast); ValueError otherwise.  Needs
    no GPU.  Values are not judged here: a NaN or alpha_scale <= 0 is marked per policy by the device (status bit 2)."""
    arrs = [np.asarray(a, dtype=np.float64).reshape(-1) for a in (thetas, shifts, alpha_scales)]
    K = max(a.size for a in arrs)
    if K < 1 or any(a.size not in (1, K) for a in arrs):
        raise ValueError('thetas, shifts, alpha_scales: %s entries, expected one length K >= 1 (or scalars)'
                         % [a.size for a in arrs])
    return [np.broadcast_to(a, (K,)).copy() for a in arrs]


def check_data_args(demos, K, days=None, set_index=None):
    """The rules that need no GPU.  demos: a Demonstrations (one data set; set_index must be None) or a
    BootstrapDemonstrations (R data sets; set_index [K] with entries in [0, R), None: K = R and policy k is held against
    replicate k).  Returns (state [S, N, H, d] fp32, moves [S, N, H-1, width, width] int32, set_index [K] int32 or None, days)."""
    from .demos import BootstrapDemonstrations, Demonstrations
    if isinstance(demos, BootstrapDemonstrations):
        days = demos.sample._days(days)
        if set_index is None:
            if K != demos.R:
                raise ValueError('K=%d policies for R=%d replicates: one policy per replicate, or give set_index' % (K, demos.R))
            set_index = np.arange(K)
        set_index = np.asarray(set_index, dtype=np.int64).reshape(-1)
        if set_index.size != K or (set_index < 0).any() or (set_index >= demos.R).any():
            raise ValueError('set_index: expected %d entries in [0, %d)' % (K, demos.R))
        state, moves = demos.state[:, days], demos.moves[:, days]
        set_index = set_index.astype(np.int32)
    elif isinstance(demos, Demonstrations):
        days = demos._days(days)
        if set_index is not None:
            raise ValueError('set_index is read with a BootstrapDemonstrations only: a Demonstrations is one data set')
        state, moves = demos.state[None, days], demos.moves[None, days]
    else:
        raise ValueError('demos: a Demonstrations or a BootstrapDemonstrations, got %s' % type(demos).__name__)
    if not days:
        raise ValueError('days: at least one day')
    return np.ascontiguousarray(state, dtype=np.float32), np.ascontiguousarray(moves, dtype=np.int32), set_index, days


def _upload(demos, K, days, set_index, dev):
    import torch
    state, moves, set_index, days = check_data_args(demos, K, days, set_index)
    return (torch.as_tensor(state, device=dev), torch.as_tensor(moves, device=dev),
            None if set_index is None else torch.as_tensor(set_index, device=dev), days)


def loglik(demos, thetas, shifts, alpha_scales, days=None, *, set_index=None, device=None):
    """The log-likelihood of the moves of `demos` under K policies: thetas, shifts, alpha_scales [K] (NumPy, scalars, or fp64
    device tensors).  demos: a Demonstrations, or a BootstrapDemonstrations with one policy per replicate (or set_index [K]:
    the replicate of each policy).  days: the days to evaluate (None: all).  More than POP_MAX_K policies go in chunks.
    Returns a LogLik."""
    import torch
    from . import ops
    par = [a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a for a in (thetas, shifts, alpha_scales)]
    th, sh, al = check_policy_args(*par)
    K = th.size
    dev = _device(device)
    state, moves, index, days = _upload(demos, K, days, set_index, dev)
    if index is None:
        state, moves = state[0], moves[0]
    parts = []
    for k0 in range(0, K, GRID_CHUNK):
        sl = slice(k0, k0 + GRID_CHUNK)
        res = ops.moves_loglik_pop(state, moves, torch.as_tensor(th[sl], device=dev), torch.as_tensor(sh[sl], device=dev),
                                   torch.as_tensor(al[sl], device=dev), demos.d,
                                   None if index is None else index[sl].contiguous())
        parts.append({name: res[name].cpu().numpy() for name in ('ll', 'll_day', 'grad_day', 'status')})
    cat = {name: np.concatenate([p[name] for p in parts]) for name in parts[0]}
    return LogLik(cat['ll'], cat['ll_day'], cat['grad_day'], cat['status'], days)


def best_point(points, total, status):
    """(index, point, value) of the FIRST maximum of `total` in grid order among the points whose status is 0 on every day and
    whose value is finite; (None, None, -inf) when there is none."""
    best, at = -np.inf, None
    for p in range(len(points)):
        if not np.any(status[p]) and np.isfinite(total[p]) and total[p] > best:
            best, at = float(total[p]), p
    return at, (None if at is None else tuple(points[at])), best


def gridsearch(theta_range, shift_range, alpha_range, demos, days=None, outfile=None, *, device=None):
    """A deterministic grid search: every point of population.grid_points(theta_range, shift_range, alpha_range) (theta
    outermost, alpha innermost) a policy of one loglik call.  Returns (table, best): table [P, 2] fp64 of (total
    log-likelihood over the days, OR of the days' status bits) per point in grid order, best = (theta, shift, alpha_scale,
    value) of the first maximum among the clean points (None without one).  outfile: appends one CSV line per point,
    theta,shift,alpha_scale,loglik,status."""
    from .population import grid_points
    points = grid_points(theta_range, shift_range, alpha_range)
    if not points:
        return np.zeros((0, 2)), None
    par = np.array(points, dtype=np.float64).reshape(-1, 3)
    res = loglik(demos, par[:, 0], par[:, 1], par[:, 2], days, device=device)
    total = res.total()
    status = np.bitwise_or.reduce(res.status, axis=1)
    table = np.stack([total, status.astype(np.float64)], axis=1)
    if outfile is not None:
        with open(outfile, 'a') as f:
            for (theta, shift, alpha_scale), value, st in zip(points, total, status):
                f.write('%r,%r,%r,%r,%d\n' % (float(theta), float(shift), float(alpha_scale), float(value), int(st)))
    at, point, value = best_point(points, total, res.status)
    return table, (None if at is None else point + (value,))


def free_mask(free):
    """[3] of 0 / 1 over PARAMS for the names in `free`."""
    free = (free,) if isinstance(free, str) else tuple(free)
    if not free or any(name not in PARAMS for name in free):
        raise ValueError('free=%r: a non-empty subset of %s' % (free, PARAMS))
    return np.array([1.0 if name in free else 0.0 for name in PARAMS])


class Fit:
    """The result of fit (NumPy).  params [K, 3]: (theta, shift, alpha_scale) of the last good iterate; trace [steps, K]: the
    log-likelihood of the iterate each step evaluated (row t: the parameters after t updates), NaN from the step at which a
    start was frozen; best_params [K, 3] and best_ll [K]: the best evaluated iterate, the final one included; final_ll [K]:
    the value at params; status [K]: the OR of every status word the start has met (non-zero: it was frozen); frozen_at [K]:
    the step at which it was frozen, -1 for none."""

    def __init__(self, params, trace, best_params, best_ll, final_ll, status, frozen_at):
        self.params, self.trace, self.best_params, self.best_ll = params, trace, best_params, best_ll
        self.final_ll, self.status, self.frozen_at = final_ll, status, frozen_at


def ascent(evaluate, p0, mask, steps, lr):
    """The update rule of fit, on torch fp64 tensors of any device, with no host read inside the loop.
    evaluate(p) -> (value [K], grad [K, 3], status [K] integer) for the parameter rows p [K, 3] = (theta, shift,
    ln alpha_scale).  With p_0 = p0, m_0 = v_0 = 0, for t = 1 .. steps:
        value, g, status = evaluate(p_{t-1});  bad = status != 0 or value not finite
        a start that is bad, or was at an earlier step, is frozen: p_t = the last iterate of it that was not bad (p0 if none),
          its trace is NaN from row t - 1 on, its m and v no longer matter
        else  g = g * mask
              m_t = 0.9 m_{t-1} + 0.1 g;   v_t = 0.999 v_{t-1} + 0.001 g g
              p_t = p_{t-1} + lr (m_t / (1 - 0.9^t)) / (sqrt(v_t / (1 - 0.999^t)) + 1e-8)        (Adam, ascending)
    and one more evaluation scores p_steps (a bad one freezes the start at p_{steps-1} likewise).  Returns a dict of tensors:
    p, trace [steps, K], best_p, best_value, final_value, status, frozen_at."""
    import torch
    K = p0.shape[0]
    kw = dict(dtype=torch.float64, device=p0.device)
    p, good = p0.clone(), p0.clone()
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    mask = torch.as_tensor(mask, **kw)
    trace = torch.full((steps, K), float('nan'), **kw)
    best_p, best = p0.clone(), torch.full((K,), float('-inf'), **kw)
    frozen = torch.zeros(K, dtype=torch.bool, device=p0.device)
    status_all = torch.zeros(K, dtype=torch.int32, device=p0.device)
    frozen_at = torch.full((K,), -1, dtype=torch.int32, device=p0.device)
    final = torch.full((K,), float('nan'), **kw)
    for t in range(1, steps + 2):
        value, g, status = evaluate(p)
        status = status.to(torch.int32)
        bad = (status != 0) | ~torch.isfinite(value)
        status_all = torch.where(frozen, status_all, status_all | status)
        frozen_at = torch.where(bad & ~frozen, torch.full_like(frozen_at, t - 1), frozen_at)
        frozen = frozen | bad
        better = ~frozen & (value > best)
        best = torch.where(better, value, best)
        best_p = torch.where(better[:, None], p, best_p)
        good = torch.where(frozen[:, None], good, p)
        if t == steps + 1:
            final = torch.where(bad, final, value)         # (a start frozen earlier sits at `good`: the same value as then)
            p = good
            break
        trace[t - 1] = torch.where(frozen, torch.full_like(value, float('nan')), value)
        final = torch.where(frozen, final, value)
        g = g * mask
        m = ADAM_BETA1 * m + (1.0 - ADAM_BETA1) * g
        v = ADAM_BETA2 * v + (1.0 - ADAM_BETA2) * (g * g)
        step = lr * (m / (1.0 - ADAM_BETA1 ** t)) / (torch.sqrt(v / (1.0 - ADAM_BETA2 ** t)) + ADAM_EPS)
        p = torch.where(frozen[:, None], good, p + step)
    return dict(p=p, trace=trace, best_p=best_p, best_value=best, final_value=final, status=status_all, frozen_at=frozen_at)


def _sum_in_order(x):
    """x [K, N, ...] -> [K, ...]: the N slices added in order (the same bits for a policy whatever K is)."""
    out = x[:, 0].clone()
    for n in range(1, x.shape[1]):
        out = out + x[:, n]
    return out


def fit(demos, theta0, shift0, alpha_scale0, *, days=None, free=PARAMS, steps=200, lr=FIT_LR, set_index=None, device=None):
    """Maximum likelihood by Adam ascent, K starts in lock-step: theta0, shift0, alpha_scale0 [K] (scalars broadcast).  The
    parameters are (theta, shift, ln alpha_scale); `free` names those that move, the others keep their start values to the
    bit.  Each step is one call of the kernel (value and gradient of every start on the given days, the days added in order)
    followed by the update of `ascent` in torch fp64 on the device; nothing is read back inside the loop.  A start whose status
    becomes non-zero (or whose value is not finite) is frozen at its last good iterate.  demos / set_index as loglik: with a
    BootstrapDemonstrations start k is fitted to replicate set_index[k].  Returns a Fit."""
    import torch
    from . import ops
    th, sh, al = check_policy_args(theta0, shift0, alpha_scale0)
    mask = free_mask(free)
    steps = int(steps)
    if steps < 1 or not float(lr) > 0.0:
        raise ValueError('steps=%r, lr=%r: at least one step and a positive rate' % (steps, lr))
    if (al <= 0).any():
        raise ValueError('alpha_scale0: the start values must be positive (the parameter is ln alpha_scale)')
    K = th.size
    if K > L.POP_MAX_K:
        raise ValueError('K=%d starts: at most %d in one fit' % (K, L.POP_MAX_K))
    dev = _device(device)
    state, moves, index, _ = _upload(demos, K, days, set_index, dev)
    if index is None:
        state, moves = state[0], moves[0]
    S = 1 if index is None else state.shape[0]
    N, H = state.shape[-3], state.shape[-2]
    workspace = torch.empty((ops.moves_loglik_workspace_bytes(K, S, N, H, demos.d) + 7) // 8, dtype=torch.int64, device=dev)
    out = {name: torch.empty(shape, dtype=dtype, device=dev) for name, (shape, dtype) in ops.moves_loglik_shapes(K, N, H).items()}

    alpha_fixed = torch.as_tensor(al, device=dev) if mask[2] == 0.0 else None      # (a fixed alpha_scale keeps its bits)

    def evaluate(p):
        alpha = alpha_fixed if alpha_fixed is not None else torch.exp(p[:, 2])
        res = ops.moves_loglik_pop(state, moves, p[:, 0].contiguous(), p[:, 1].contiguous(), alpha, demos.d, index, out=out,
                                   workspace=workspace)
        status = res['status'][:, 0].clone()
        for n in range(1, N):
            status = status | res['status'][:, n]
        return _sum_in_order(res['ll_day']), _sum_in_order(res['grad_day']), status

    p0 = torch.as_tensor(np.stack([th, sh, np.log(al)], axis=1), device=dev)
    r = ascent(evaluate, p0, mask, steps, float(lr))

    def natural(p):
        p = p.cpu().numpy().copy()
        p[:, 2] = al if mask[2] == 0.0 else np.exp(p[:, 2])
        return p

    return Fit(natural(r['p']), r['trace'].cpu().numpy(), natural(r['best_p']), r['best_value'].cpu().numpy(),
               r['final_value'].cpu().numpy(), r['status'].cpu().numpy(), r['frozen_at'].cpu().numpy())


class BootstrapFit:
    """fit_bootstrap's result: `fit`, the Fit of the R replicates (start r on replicate r); estimates [R, 3] = fit.params;
    mean, std [3] (ddof 0) over the replicates that were not frozen; interval [2, 3]: per parameter the order statistics of
    ranks floor(a (M - 1)) and ceil((1 - a) (M - 1)), a = (1 - level) / 2, among those M replicates; used [R] bool."""

    def __init__(self, fit_result, level):
        self.fit, self.level = fit_result, float(level)
        self.estimates = fit_result.params
        self.used = fit_result.status == 0
        est = self.estimates[self.used]
        M = est.shape[0]
        if M == 0:
            self.mean = self.std = np.full(3, np.nan)
            self.interval = np.full((2, 3), np.nan)
            return
        self.mean, self.std = est.mean(0), est.std(0)
        a = (1.0 - self.level) / 2.0
        lo, hi = int(np.floor(a * (M - 1))), int(np.ceil((1.0 - a) * (M - 1)))
        ordered = np.sort(est, axis=0)
        self.interval = np.stack([ordered[lo], ordered[hi]])


def fit_bootstrap(boot, theta0, shift0, alpha_scale0, *, days=None, free=PARAMS, steps=200, lr=FIT_LR, level=0.9, device=None):
    """One maximum-likelihood fit per bootstrap replicate, all R in lock-step in the calls of one fit (set_index[r] = r): the
    spread of the estimates is the error bar that the resampling of the recorded agents puts on the fitted parameters.
    theta0, shift0, alpha_scale0: scalars (every replicate starts there) or [R].  Replicate r's row equals
    fit(boot.replicate(r), ...) on the same start bit for bit.  Returns a BootstrapFit."""
    from .demos import BootstrapDemonstrations
    if not isinstance(boot, BootstrapDemonstrations):
        raise ValueError('boot: a BootstrapDemonstrations (demos.bootstrap), got %s' % type(boot).__name__)
    if not 0.0 < float(level) < 1.0:
        raise ValueError('level=%r outside (0, 1)' % (level,))
    th, sh, al = check_policy_args(theta0, shift0, alpha_scale0)
    if th.size not in (1, boot.R):
        raise ValueError('start values: scalars or one per replicate (R=%d), got %d' % (boot.R, th.size))
    th, sh, al = (np.broadcast_to(a, (boot.R,)).copy() for a in (th, sh, al))
    res = fit(boot, th, sh, al, days=days, free=free, steps=steps, lr=lr, set_index=np.arange(boot.R), device=device)
    return BootstrapFit(res, level)
