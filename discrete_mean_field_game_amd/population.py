"""A population of K independent actor-critic learners trained in the launches of one (mfg_train_episodes_pop /
mfg_train_rollouts_pop, include/mfg_hip.h).

The reference trains such learners one after another: mfg_ac2.gridsearch sweeps theta, shift and alpha (mfg_ac2.py:673-689),
and every result is a choice among several seeds and learning rates.  ActorCriticPopulation holds K learners, each with its own
theta, critic weights w, shift, alpha_scale, learning rates, Philox seed and `batch` trajectories, and trains them in lock-step:
learner k ends with exactly (bit for bit) what `actor_critic(theta_k, shift_k, alpha_k, d, batch=batch, seed=seed_k)` with
the same w gives after the same train() calls.

Start states are drawn on the device, as actor_critic does for batch > 1 (hence batch >= 2 here).  Single GPU, d <= 64,
in-kernel rewards ('mfg_ac2', 'synthetic'); IRL and several GPUs are out of scope.

The instance owns one ops.Context: its sticky mixed-range status word (include/mfg_hip.h, mfg_status) is shared by the K
learners, so by default ONE learner whose policy leaves the fp32 range of mixed-precision sampling stops the population's next
launch (train() raises MfgError; clear_status() resets it; precision='f64' has no such range).

Small learners in step mode: ActorCriticPopulation(..., resident=None) runs the episodes of learners of a few tiles through
mfg_train_episodes_pop_resident -- one workgroup per learner for the whole call instead of 1 + 2 T launches per episode,
the same bits -- where resident_rule(K, d, batch) measured it faster; resident=True / False force / forbid it.

Retiring learners on the device: train(..., stop_criteria=c, isolate=True) runs under a population control block
(mfg_ctx_set_pop_control, include/mfg_hip.h) -- an activity state per learner in device memory that every launch of the call
carries.  A learner whose |theta_e - theta_{e-1}| falls below its criterion stops after that episode (AC_IRL.train's early
stop, ac_irl.py:726), a learner whose theta leaves the mixed-precision range or whose theta / w stop being finite is marked
failed at the episode boundary at which that is seen; either way its blocks leave the remaining launches at once, the other
learners run on with the same bits, and the host reads nothing back inside the call.  With isolate=True a failed learner does
not raise and does not touch the context's status word: `learner_state` (0 active, 1 stopped, 2 failed), `episodes_run` and
`learner_status` tell what happened, failed learners are skipped (NaN rows) by everything after training, and
clear_status(k) revives one.  The Philox step (and an IRL population's reward-call counters) advance by the whole call for
every learner, stopped or not.

Population-based training on the device: train(..., validate=Validation(...), evolve=Evolution(...)) runs an exploit / explore
step behind every evolve.every-th held-out check (mfg_ctx_set_pop_evolve, include/mfg_hip.h): the worst active learners take
over theta, w and the best iterate of a random one of the best and go on with perturbed learning rates, ranked, copied and
perturbed by two small kernels inside the call; `evolution` (an EvolutionTrace) tells what happened.
"""
from __future__ import annotations

import os

import numpy as np
import torch

from . import _lib as L
from . import ops
from .mfg_ac2 import EPISODE_STEPS, _with_ctx, actor_critic

REWARDS = {'mfg_ac2': L.REWARD_MFG_AC2, 'synthetic': L.REWARD_SYNTHETIC}


def broadcast(name, value, K, dtype=np.float64):
    """`value` (a scalar or K values) as a NumPy array [K] of `dtype`."""
    a = np.asarray(value, dtype=dtype)
    if a.ndim == 0:
        return np.full(K, a, dtype=dtype)
    a = a.reshape(-1)
    if a.shape[0] != K:
        raise ValueError('%s: expected a scalar or %d values (one per learner), got %d' % (name, K, a.shape[0]))
    return a.copy()


def stop_criteria_array(stop_criteria, K):
    """train()'s stop_criteria (a scalar or K values) as a NumPy fp64 array [K]; a negative entry (the default -1, as in
    AC_IRL.train) means no early stop for that learner.  ValueError for a wrong count or a NaN."""
    a = broadcast('stop_criteria', stop_criteria, K)
    if np.any(np.isnan(a)):
        raise ValueError('stop_criteria: NaN')
    return a


ACTIVE, STOPPED, FAILED = 0, 1, 2      # mfg_pop_control_t::state


class LearnerActivity:
    """The host mirror of a population's control block: per learner the state (ACTIVE / STOPPED / FAILED), the episodes it
    completed in the last train() call and its own status bits.  All zero until a call reports otherwise."""

    def __init__(self, K):
        self.state = np.zeros(K, dtype=np.int32)
        self.episodes = np.zeros(K, dtype=np.int32)
        self.status = np.zeros(K, dtype=np.int32)

    def healthy(self):
        """The learners that have not failed, in order."""
        return [k for k in range(self.state.shape[0]) if self.state[k] != FAILED]

    def clear(self, k=None):
        """Revive the failed learner k (None: all): state and status bits back to 0; a stopped learner stays as it is."""
        K = self.state.shape[0]
        if k is None:
            sel = slice(None)
        else:
            if not 0 <= int(k) < K:
                raise IndexError('learner %d of %d' % (k, K))
            sel = slice(int(k), int(k) + 1)
        self.state[sel] = np.where(self.state[sel] == FAILED, ACTIVE, self.state[sel])
        self.status[sel] = 0


def needs_control(stop, isolate, state):
    """True when a train() call runs under the population control block: a stop criterion >= 0 (`stop`: the array of
    stop_criteria_array), isolate=True, or a learner that failed earlier (`state`: LearnerActivity.state)."""
    return bool(isolate) or bool(np.any(stop >= 0)) or bool(np.any(state == FAILED))


# ------------------------------------------------------------------------------- the resident step-mode path
# mfg_train_episodes_pop_resident (include/mfg_hip.h): one workgroup holds a learner for a whole launch -- no launch per env
# step -- and gives the bits of the per-step launches.  It serves d = 21 / 15 up to RESIDENT_MAX_TILES tiles per learner.
RESIDENT_TILE = {21: 12, 15: 16}      # trajectories per tile of the packed step kernel (4 waves x floor(64 / d))
RESIDENT_MAX_TILES = L.POP_RESIDENT_MAX_TILES


def resident_supported(d, batch):
    """mfg_pop_resident_supported for the in-kernel rewards of a population, restated on the host (no library call)."""
    tb = RESIDENT_TILE.get(int(d))
    return tb is not None and 1 <= -(-int(batch) // tb) <= RESIDENT_MAX_TILES


# Measured on one MI355X (tools/pop_resident_probe.py -> profiles/pop_resident_ab.txt; mixed precision, T = 15, five alternating
# repetitions per side, every difference far outside the sides' spreads): per d and measured tiles per learner, the ratio
# per-step / resident of the medians at K = 16, at K = 256, and the smaller of those at K = 512 and K = 4 096.
RESIDENT_AB = {21: {1: (1.89, 3.95, 5.05), 4: (0.53, 1.59, 2.25), 8: (0.27, 1.19, 1.72), 16: (0.14, 0.97, 1.41), 64: (0.07, 0.78, 1.17)},
               15: {1: (1.94, 2.89, 3.12), 4: (0.54, 1.32, 1.75), 16: (0.14, 0.89, 1.31), 64: (0.07, 0.76, 1.16)}}
RESIDENT_BLOCKS = 512     # workgroups of the resident kernel the card holds at once: 256 CUs x 2


def resident_rule(K, d, batch):
    """Whether ActorCriticPopulation(resident=None) trains K learners of `batch` trajectories through the resident kernel:
    where it beat the per-step launches in RESIDENT_AB (DESIGN.md "Populations" has the table), never for a shape the library
    does not serve.  Off the measured grid the rule only moves to the less favourable measured neighbour: the next measured
    tile count up (the gain falls with the tiles a workgroup serialises) and the next measured K down (below 512 learners
    the gain rises with K in every row); K < 16 was not measured: per-step.  From 512 learners on the workgroups run in rounds
    of RESIDENT_BLOCKS, and the gain measured at full rounds (K = 512, 4 096) is discounted by the fill of the last round --
    arithmetic, not a measurement, so it has to clear 1.1."""
    K, d, batch = int(K), int(d), int(batch)
    if not resident_supported(d, batch) or K < 16:
        return False
    tiles = -(-batch // RESIDENT_TILE[d])
    at16, at256, full = RESIDENT_AB[d][min(t for t in RESIDENT_AB[d] if t >= tiles)]
    if K < 256:
        return at16 > 1.0
    if K < RESIDENT_BLOCKS:
        return at256 > 1.0
    rounds = -(-K // RESIDENT_BLOCKS)
    return full * K / (RESIDENT_BLOCKS * rounds) > 1.1


def check_resident(resident, d, batch, update_every):
    """Validation of the constructor's `resident` (no GPU needed): None, True or False; True needs update_every='step' and a
    shape the resident kernel serves."""
    if resident not in (None, True, False):
        raise ValueError('resident must be None (the measured rule), True or False')
    if resident is True:
        if update_every != 'step':
            raise ValueError("resident=True: the resident kernel runs update_every='step' only")
        if not resident_supported(d, batch):
            raise ValueError('resident=True: d=%d, batch=%d is outside the resident kernel\'s shapes (d = 21 / 15, at most %d '
                             'tiles of %s trajectories per learner)' % (d, batch, RESIDENT_MAX_TILES, RESIDENT_TILE.get(int(d), '-')))


def use_resident(resident, rule, control):
    """Whether a step-mode train() call takes the resident path.  resident: the constructor's argument; rule:
    resident_rule(K, d, batch); control: needs_control(...) of the call.  A forced resident=True refuses a controlled call
    (ValueError: retiring learners inside the resident kernel is not supported); under None such a call takes the per-step
    launches."""
    if resident is True:
        if control:
            raise ValueError('resident=True: this call runs under the population control block (a stop criterion, isolate=True '
                             'or a learner that failed earlier), which the resident kernel does not serve; use resident=None '
                             'or False')
        return True
    return resident is None and bool(rule) and not control


def check_args(K, d, batch, update_every, reward, precision, episode_steps, resident=None):
    """Validation of the constructor's arguments (no GPU needed)."""
    if K < 1 or K > L.POP_MAX_K:
        raise ValueError('population size %d outside [1, %d]' % (K, L.POP_MAX_K))
    if not 1 <= d <= 64:
        raise ValueError('d=%d: populations cover d <= 64 (one wave per trajectory already fills the machine beyond)' % d)
    if batch < 2:
        raise ValueError('batch=%d: a population draws its start states on the device, which actor_critic does from batch 2 '
                         'on' % batch)
    if update_every not in ('step', 'rollout'):
        raise ValueError("update_every must be 'step' or 'rollout'")
    if reward not in REWARDS:
        raise ValueError("reward must be 'mfg_ac2' or 'synthetic' (in-kernel rewards; IRL is not supported)")
    if precision not in ('mixed', 'f64'):
        raise ValueError("precision must be 'mixed' or 'f64'")
    if episode_steps < 1:
        raise ValueError('episode_steps must be >= 1')
    check_resident(resident, d, batch, update_every)


def resolve_start_table(d, pi0=None, path_to_dir=None):
    """The start-state table [num_start, d] (fp64) as actor_critic resolves it: `pi0`, else the reference's directory, else
    actor_critic's synthetic table."""
    if pi0 is not None:
        return np.array(pi0, dtype=np.float64)[:, 0:d]
    if path_to_dir is None:
        path_to_dir = os.getcwd() + '/train_normalized_round2'
    if os.path.isdir(path_to_dir):
        holder = type('_Table', (), {})()
        holder.d = d
        actor_critic.init_pi0(holder, path_to_dir=path_to_dir)
        return holder.mat_pi0
    rs = np.random.RandomState(0)   # actor_critic's synthetic table: Dirichlet(1) rows via '%.3e' text
    m = rs.dirichlet(np.ones(d), size=64)
    return np.array([[float('%.3e' % v) for v in row] for row in m])


# ---------------------------------------------------------------------------------------------------------- evaluation
# The selection step (evaluate / gridsearch, mfg_ac2.py:595-689, ac_irl.py:1495-1590) for K policies at once: one
# mfg_evaluate_pop call rolls every policy over every test file and reduces the eight metrics on the device.
GRID_CHUNK = L.POP_MAX_K    # grid points per evaluate_pop call of gridsearch (a grid beyond goes in chunks)


def load_empirical(indir, d, episode_length):
    """Every file of cwd/indir, in listdir order, as actor_critic._load_empirical reads them: a NumPy [N, L, d] fp64 array of
    each file's first `episode_length` rows and `d` columns.  ValueError for an unusable argument or directory."""
    if not 1 <= int(d) <= 64:
        raise ValueError('d=%d: population evaluation covers d <= 64 (as the populations do)' % d)
    if int(episode_length) < 2:
        raise ValueError('episode_length=%d: an evaluation rolls at least one step (episode_length >= 2)' % episode_length)
    path_to_dir = os.getcwd() + '/' + indir
    names = os.listdir(path_to_dir)
    if not names:
        raise ValueError('%s: no test files' % path_to_dir)
    emp = []
    for filename in names:
        with open(path_to_dir + '/' + filename, 'r') as f:
            m = np.loadtxt(f, delimiter=' ', ndmin=2)[:, 0:d]
        if m.shape[0] < episode_length or m.shape[1] < d:
            raise ValueError('%s: %d rows of %d entries, the evaluation needs %d rows of %d'
                             % (filename, m.shape[0], m.shape[1], episode_length, d))
        emp.append(m[:episode_length])
    return np.array(emp)


# ---------------------------------------------------------------------------------------- validation inside train()
# The held-out checks of a population training call (mfg_ctx_set_pop_validate, include/mfg_hip.h): every `period` episodes the
# call itself enqueues the evaluate_pop launches on the learners' current theta (and the forecast-score launches), keeps the
# curve row and the best iterate on the device and -- with patience -- stops a learner whose metric no longer improves.
# The columns of a curve row: the CSV's eight (actor_critic._EVAL_HEADER) and the two hour means of the proper scores.
VALIDATION_COLUMNS = tuple(actor_critic._EVAL_HEADER.strip().split(',')[3:]) + ('crps', 'energy')


def validation_column(metric):
    """Index of `metric` in VALIDATION_COLUMNS: a column's name, or for the four means its short form ('JSD_mean' is
    'mean_JSD_mean', the names of the table evaluate() returns).  ValueError for anything else."""
    if metric in VALIDATION_COLUMNS:
        return VALIDATION_COLUMNS.index(metric)
    if isinstance(metric, str) and 'mean_' + metric in VALIDATION_COLUMNS:
        return VALIDATION_COLUMNS.index('mean_' + metric)
    raise ValueError('metric=%r: expected one of %s (or l1_final, l1_mean, JSD_final, JSD_mean for the means)'
                     % (metric, ', '.join(VALIDATION_COLUMNS)))


class Validation:
    """What train(..., validate=Validation(...)) checks on held-out days, on the device, every `period` episodes.
    emp [N, L, d] (NumPy; the held-out rows) or indir (read by load_empirical with episode_length, at the first call: its d is
    the population's) -- exactly one of them; repeats: rollouts per held-out file; metric: the column of VALIDATION_COLUMNS the
    best iterate is selected by (smaller is better; 'crps' / 'energy' need score=True); patience > 0: a learner whose metric
    has not improved in `patience` consecutive checks stops (learner_state STOPPED); score=True: also the proper scores of
    the members (columns 'crps', 'energy').  Every argument is checked here, on the host."""

    def __init__(self, emp=None, indir=None, period=1, repeats=1, metric='JSD_mean', patience=0, score=False, episode_length=16):
        if (emp is None) == (indir is None):
            raise ValueError('Validation: give exactly one of emp (an [N, L, d] array) and indir (a directory of held-out files)')
        for name, v, lo in (('period', period, 1), ('repeats', repeats, 1), ('patience', patience, 0),
                            ('episode_length', episode_length, 2)):
            if int(v) != v or int(v) < lo:
                raise ValueError('Validation: %s=%r, expected an integer >= %d' % (name, v, lo))
        self.column = validation_column(metric)
        self.score = bool(score)
        if self.column >= 8 and not self.score:
            raise ValueError('Validation: metric=%r needs score=True' % (metric,))
        if self.score and int(repeats) > L.FORECAST_MAX_REPEATS:
            raise ValueError('Validation: repeats=%d > %d with score=True' % (repeats, L.FORECAST_MAX_REPEATS))
        if emp is not None:
            emp = np.array(emp, dtype=np.float64)
            if emp.ndim != 3 or emp.shape[0] < 1 or emp.shape[1] < 2 or not 1 <= emp.shape[2] <= 64:
                raise ValueError('Validation: emp must be [N >= 1, L >= 2, 1 <= d <= 64], got %s' % (emp.shape,))
        self.emp, self.indir = emp, indir
        self.metric, self.period, self.repeats, self.patience = metric, int(period), int(repeats), int(patience)
        self.episode_length = int(episode_length)

    def rows(self, d):
        """The held-out rows [N, L, d] fp64 for a population of dimension d (ValueError when emp has another d)."""
        if self.emp is None:
            self.emp = load_empirical(self.indir, d, self.episode_length)
        if self.emp.shape[2] != d:
            raise ValueError('Validation: emp has d=%d, the population d=%d' % (self.emp.shape[2], d))
        return self.emp


class ValidationTrace:
    """The held-out checks of one train(..., validate=...) call (NumPy): curve [K, C, 10] (VALIDATION_COLUMNS; NaN past
    checks[k]), checks [K], episodes [C] (the call-episode number after which check c ran, 1-based), and the best iterate per
    learner: best_value, best_check (-1: none), best_episode (0: none), best_theta, best_w."""

    def __init__(self, curve, checks, period, best_value, best_check, best_theta, best_w, column):
        self.curve, self.checks, self.column = curve, checks, column
        self.episodes = (np.arange(curve.shape[1]) + 1) * int(period)
        self.best_value, self.best_check, self.best_theta, self.best_w = best_value, best_check, best_theta, best_w
        self.best_episode = np.where(best_check >= 0, (best_check + 1) * int(period), 0)


# -------------------------------------------------------------------------- population-based training inside train()
# The exploit / explore steps of a population training call (mfg_ctx_set_pop_evolve, include/mfg_hip.h; Jaderberg et al. 2017,
# truncation selection): behind every `every`-th held-out check the worst learners take over theta, w and the best iterate of
# one of the best and go on with perturbed learning rates -- ranked, copied and perturbed on the device.
PERTURB_BITS = {'lr_critic': 1, 'lr_actor': 2}


def _evolve_count(name, v, K):
    """`v` as a number of learners out of K: an integer count as it is, a fraction f in (0, 1) as max(1, floor(f K))."""
    if isinstance(v, (int, np.integer)) and not isinstance(v, bool):
        return int(v)
    return max(1, int(np.floor(float(v) * K)))


class Evolution:
    """What train(..., validate=V, evolve=Evolution(...)) does behind every `every`-th check of V: the `bottom` worst active
    learners (by V's metric) are replaced by copies of random members of the `top` best and continue with the donor's learning
    rates times factors[0] or factors[1] (a fair coin per rate), clamped to the bounds.  top / bottom: fractions in (0, 1)
    (max(1, floor(f K)) learners) or integer counts >= 1; perturb: the rates that are perturbed, a subset of ('lr_critic',
    'lr_actor') -- the others are copied from the donor; seed: key of the donor and coin draws.  Every argument is checked
    here, on the host; counts(K) raises ValueError when top + bottom exceed the population."""

    def __init__(self, every=1, top=0.25, bottom=0.25, factors=(0.8, 1.25), perturb=('lr_critic', 'lr_actor'),
                 lr_critic_bounds=(1e-6, 10.0), lr_actor_bounds=(1e-8, 1.0), seed=0):
        if isinstance(every, bool) or int(every) != every or int(every) < 1:
            raise ValueError('Evolution: every=%r, expected an integer >= 1' % (every,))
        for name, v in (('top', top), ('bottom', bottom)):
            if isinstance(v, bool):
                raise ValueError('Evolution: %s=%r' % (name, v))
            if isinstance(v, (int, np.integer)):
                if v < 1:
                    raise ValueError('Evolution: %s=%r, a count is >= 1' % (name, v))
            elif not 0.0 < float(v) < 1.0:           # (a NaN fails both comparisons)
                raise ValueError('Evolution: %s=%r, a fraction lies in (0, 1)' % (name, v))
        factors = tuple(float(f) for f in factors)
        if len(factors) != 2 or not all(np.isfinite(f) and f > 0 for f in factors):
            raise ValueError('Evolution: factors=%r, expected two finite factors > 0' % (factors,))
        if isinstance(perturb, str):
            perturb = (perturb,)
        perturb = tuple(perturb)
        if any(n not in PERTURB_BITS for n in perturb) or len(set(perturb)) != len(perturb):
            raise ValueError("Evolution: perturb=%r, expected a subset of ('lr_critic', 'lr_actor')" % (perturb,))
        bounds = []
        for name, b in (('lr_critic_bounds', lr_critic_bounds), ('lr_actor_bounds', lr_actor_bounds)):
            b = tuple(float(x) for x in b)
            if len(b) != 2 or not (0.0 < b[0] <= b[1] and np.isfinite(b[1])):
                raise ValueError('Evolution: %s=%r, expected 0 < min <= max, finite' % (name, b))
            bounds.append(b)
        if isinstance(seed, bool) or int(seed) != seed or not 0 <= int(seed) < 2 ** 64:
            raise ValueError('Evolution: seed=%r, expected an integer in [0, 2^64)' % (seed,))
        self.every, self.top, self.bottom, self.factors, self.perturb = int(every), top, bottom, factors, perturb
        self.lr_critic_bounds, self.lr_actor_bounds, self.seed = bounds[0], bounds[1], int(seed)
        self.perturb_bits = sum(PERTURB_BITS[n] for n in perturb)

    def counts(self, K):
        """(n_top, n_bottom) for a population of K learners; ValueError when they exceed it."""
        n_top, n_bottom = _evolve_count('top', self.top, K), _evolve_count('bottom', self.bottom, K)
        if n_top + n_bottom > int(K):
            raise ValueError('Evolution: top=%d + bottom=%d learners exceed the population (K=%d)' % (n_top, n_bottom, K))
        return n_top, n_bottom


class EvolutionTrace:
    """The exploit / explore steps of one train(..., evolve=...) call (NumPy): rank [K, S] (learner k's rank among the active
    learners at step s, 0 the best; -1: not active), parent [K, S] (the learner whose parameters k continued with: itself, or
    its donor; -1: not active), lr [K, S, 2] (critic, actor rate after the step; NaN: not active), and lr_critic, lr_actor [K],
    the rates the call ended on -- ready to pass to the next train()."""

    def __init__(self, rank, parent, lr, lr_critic, lr_actor, every):
        self.rank, self.parent, self.lr, self.lr_critic, self.lr_actor, self.every = rank, parent, lr, lr_critic, lr_actor, int(every)

    def lineage(self, k):
        """[S + 1] learners: entry S is k, entry s < S the learner that held, before step s, the parameters learner k went on
        with (a step at which the holder was not active changes nothing)."""
        S = self.parent.shape[1]
        out = np.empty(S + 1, dtype=np.int64)
        out[S] = int(k)
        for s in range(S - 1, -1, -1):
            p = int(self.parent[out[s + 1], s])
            out[s] = p if p >= 0 else out[s + 1]
        return out


def evaluate_policies(emp, thetas, shifts, alpha_scales, seeds, first_step, repeats, precision, device, ctx):
    """The eight metrics [K, 8] (NumPy) of K policies on the test rows `emp` [N, L, d]: one ops.evaluate_pop call.  `thetas`,
    `shifts`, `alpha_scales` fp64 and `seeds` int64 device tensors [K].  MfgError when a mixed-precision policy left the
    fp32 range (ctx: the bound context whose status word the launch reports into)."""
    emp64 = torch.as_tensor(emp, dtype=torch.float64, device=device)
    emp32 = torch.as_tensor(emp.astype(np.float32), device=device)
    metrics = ops.evaluate_pop(emp32, emp64, thetas, shifts, alpha_scales, seeds, first_step=first_step, repeats=repeats,
                               precision=precision).cpu().numpy()
    if precision == 'mixed' and ctx.status(synchronize=True):
        raise L.MfgError('a mixed-precision evaluation ran a policy with |theta| (1 + |shift|) > 86 (or theta not finite): '
                         'its metrics are NaN; use precision=\'f64\'')
    return metrics


def write_eval_rows(outfile, write_header, points, table):
    """Append one CSV line per (theta, shift, alpha_scale) point, in the format of actor_critic.evaluate."""
    with open(outfile, 'a') as f:
        if write_header:
            f.write(actor_critic._EVAL_HEADER)
        for (theta, shift, alpha_scale), res in zip(points, table):
            f.write(actor_critic._EVAL_FMT % ((theta, shift, alpha_scale) + tuple(res)))


def grid_points(theta_range, shift_range, alpha_range):
    """The grid in the reference's loop order (theta outermost, alpha innermost, mfg_ac2.py:680-683)."""
    return [(theta, shift, alpha_scale) for theta in theta_range for shift in shift_range for alpha_scale in alpha_range]


def best_points(points, table):
    """The reference's list_tuples (mfg_ac2.py:684-688): per metric (mean l1_final, l1_mean, JSD_final, JSD_mean) the
    value and the point of the LAST minimum in grid order (its `<=`), starting from [100, 0, 0, 0]."""
    list_tuples = [[100, 0, 0, 0], [100, 0, 0, 0], [100, 0, 0, 0], [100, 0, 0, 0]]
    for (theta, shift, alpha_scale), res in zip(points, table):
        result = (res[0], res[2], res[4], res[6])
        for idx in range(4):
            if result[idx] <= list_tuples[idx][0]:
                list_tuples[idx] = [float(result[idx]), theta, shift, alpha_scale]
    return list_tuples


def gridsearch(theta_range, shift_range, alpha_range, indir, outfile, *, d=21, seed=0, episode_length=16, repeats=1,
               precision='mixed', device=None, verbose=0):
    """mfg_ac2.gridsearch (mfg_ac2.py:673-689) with every grid point a policy of one evaluate_pop call (GRID_CHUNK points per
    call).  Appends one CSV line per point in the reference's theta-major order and returns its list_tuples.
    Unlike actor_critic.gridsearch, every point uses the same seed and the same Philox step (0): common random numbers, so
    the points are compared on the same noise, and point p equals a fresh actor_critic(theta, shift, alpha_scale, d,
    seed=seed).evaluate(theta, shift, alpha_scale, d, episode_length, indir, ...).  repeats = R rolls R trajectories per test
    file.  Runs on a context of its own: a diverged mixed-precision point raises MfgError, writes no line and leaves the
    caller's status word alone."""
    if precision not in ('mixed', 'f64'):
        raise ValueError("precision must be 'mixed' or 'f64'")
    if int(repeats) < 1:
        raise ValueError('repeats=%d: at least one rollout per test file' % repeats)
    emp = load_empirical(indir, int(d), int(episode_length))
    points = grid_points(theta_range, shift_range, alpha_range)
    if verbose:
        for theta, shift, alpha_scale in points:
            print('Theta %f, shift %f, alpha %d' % (theta, shift, alpha_scale))
    if not points:
        return best_points(points, [])
    if not torch.cuda.is_available():
        raise L.MfgError('gridsearch needs a ROCm GPU: the HIP hot path has no CPU fallback')
    L.lib()
    ops.init()
    dev = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
    ctx = ops.Context(dev)
    prev = ctx.bind_scoped()
    try:
        par = np.array(points, dtype=np.float64).reshape(-1, 3)
        tables = []
        for c0 in range(0, len(points), GRID_CHUNK):
            p = par[c0:c0 + GRID_CHUNK]
            n = p.shape[0]
            seeds = torch.full((n,), int(np.array(seed, dtype=np.uint64).view(np.int64)), dtype=torch.int64, device=dev)
            tables.append(evaluate_policies(emp, torch.as_tensor(p[:, 0].copy(), device=dev),
                                            torch.as_tensor(p[:, 1].copy(), device=dev), torch.as_tensor(p[:, 2].copy(), device=dev),
                                            seeds, 0, int(repeats), precision, dev, ctx))
        table = np.concatenate(tables)
    finally:
        ctx.restore(prev)
        ctx.close()
    write_eval_rows(outfile, 0, points, table)
    list_tuples = best_points(points, table)
    if verbose:
        print(list_tuples)
    return list_tuples


# ------------------------------------------------------------------------------------------------------------ forecast
# The forecast the project exists for, with its uncertainty: R rollouts per start state under each policy, reduced on the device
# (mfg_forecast_pop) to the expected histogram per hour, its spread, quantile bands per topic and -- against held-out rows --
# the growth of the error with the horizon.  The reference plots one sample path by hand (visualize_test, mfg_ac2.py:763,
# ac_irl.py:1663); its VAR baseline returns a forecast with intervals (var.py:294-327).
FORECAST_CHUNK = L.POP_MAX_K    # policies per forecast_pop call of forecast() (more go in chunks)
FORECAST_PROBS = (0.05, 0.5, 0.95)


def forecast_ranks(probs, R):
    """The 0-based ranks floor(p (R - 1)) among R ascending ensemble members for the probabilities `probs` (each in [0, 1], at
    most FORECAST_MAX_RANKS of them): the order statistics a forecast returns as its quantiles -- members of the ensemble,
    not interpolations.  ValueError outside those rules.  Needs no GPU."""
    R = int(R)
    if R < 1:
        raise ValueError('R=%d: an ensemble has at least one member' % R)
    probs = [float(p) for p in np.asarray(probs, dtype=np.float64).reshape(-1)]
    if len(probs) > L.FORECAST_MAX_RANKS:
        raise ValueError('%d probabilities: at most %d quantiles per forecast' % (len(probs), L.FORECAST_MAX_RANKS))
    for p in probs:
        if not 0.0 <= p <= 1.0:        # (a NaN fails both comparisons)
            raise ValueError('probability %r outside [0, 1]' % p)
    return [int(np.floor(p * (R - 1))) for p in probs]


class Forecast:
    """The result of a forecast (NumPy): mean, std [K, N, H, d] over the ensemble of each start state; quantiles
    [K, N, H, Q, d], the order statistics of ranks[q] = floor(probs[q] (R - 1)); curves [K, H, 4] = (l1_mean, l1_std, jsd_mean,
    jsd_std) per hour against the held-out rows, or None without them; traj [K, N R, H, d], the members, only when asked for.
    A single-policy forecast (actor_critic.forecast) drops the leading K.  counts [K, N R, H, d] int32: the members' agent
    counts, from a finite-population forecast (forecast_agents) that was asked for them; None otherwise."""

    def __init__(self, mean, std, quantiles, probs, ranks, curves, repeats, traj=None, counts=None):
        self.mean, self.std, self.quantiles, self.curves, self.traj = mean, std, quantiles, curves, traj
        self.probs, self.ranks, self.repeats = tuple(probs), tuple(ranks), int(repeats)
        self.counts = counts

    def learner(self, k):
        """Row k as a Forecast of its own."""
        pick = lambda a: None if a is None else a[k]
        return Forecast(pick(self.mean), pick(self.std), pick(self.quantiles), self.probs, self.ranks, pick(self.curves),
                        self.repeats, pick(self.traj), pick(self.counts))


def forecast_policies(start, emp, thetas, shifts, alpha_scales, seeds, horizon, first_step, repeats, ranks, precision, device, ctx,
                      want_traj=False):
    """One ops.forecast_pop call as NumPy arrays (mean, std, quant, curves, traj): `start` [N, d] fp64 rows, `emp` [N, H, d] or
    None; `thetas`, `shifts`, `alpha_scales` fp64 and `seeds` int64 device tensors [K].  MfgError when a mixed-precision policy
    left the fp32 range (ctx: the bound context whose status word the launch reports into)."""
    start32 = torch.as_tensor(np.ascontiguousarray(start, dtype=np.float32), device=device)
    emp64 = emp32 = None
    if emp is not None:
        emp64 = torch.as_tensor(np.ascontiguousarray(emp, dtype=np.float64), device=device)
        emp32 = torch.as_tensor(np.ascontiguousarray(emp, dtype=np.float64).astype(np.float32), device=device)
    out = ops.forecast_pop(start32, thetas, shifts, alpha_scales, seeds, horizon, first_step=first_step, repeats=repeats,
                           ranks=ranks, precision=precision, emp32=emp32, emp64=emp64, want_traj=want_traj)
    host = {k: None if v is None else v.cpu().numpy() for k, v in out.items()}
    if precision == 'mixed' and ctx.status(synchronize=True):
        raise L.MfgError('a mixed-precision forecast ran a policy with |theta| (1 + |shift|) > 86 (or theta not finite): '
                         'its rows are NaN; use precision=\'f64\'')
    if host['quant'] is None:
        K, N = host['mean'].shape[:2]
        host['quant'] = np.zeros((K, N, int(horizon), 0, host['mean'].shape[-1]), dtype=np.float32)
    return host


def _forecast_inputs(pi0, emp, d, horizon):
    """(start [N, d] fp64, emp [N, H, d] fp64 or None) of a forecast: the start rows are `pi0` ((d,) or [N, d]) or, without it,
    row 0 of each emp matrix.  ValueError for unusable shapes."""
    d, horizon = int(d), int(horizon)
    if not 1 <= d <= 64:
        raise ValueError('d=%d: the ensemble forecast covers d <= 64 (as the populations do)' % d)
    if horizon < 2:
        raise ValueError('horizon=%d: a forecast rolls at least one step (horizon >= 2)' % horizon)
    if emp is not None:
        emp = np.asarray(emp, dtype=np.float64)
        if emp.ndim == 2:
            emp = emp[None]
        if emp.ndim != 3 or emp.shape[1] < horizon or emp.shape[2] < d:
            raise ValueError('emp: expected [N, >= %d, >= %d], got %s' % (horizon, d, emp.shape))
        emp = np.ascontiguousarray(emp[:, :horizon, :d])
    if pi0 is None:
        if emp is None:
            raise ValueError('a forecast needs start rows: pi0, or emp whose row 0 they are')
        start = emp[:, 0].copy()
    else:
        start = np.asarray(pi0, dtype=np.float64)
        if start.ndim == 1:
            start = start[None]
        if start.ndim != 2 or start.shape[1] < d:
            raise ValueError('pi0: expected (d,) or [N, d] with d >= %d, got %s' % (d, start.shape))
        start = np.ascontiguousarray(start[:, :d])
    if emp is not None and emp.shape[0] != start.shape[0]:
        raise ValueError('pi0 has %d rows, emp %d matrices' % (start.shape[0], emp.shape[0]))
    return start, emp


def forecast(thetas, shifts, alpha_scales, pi0, horizon, *, d, seed=0, repeats=256, probs=FORECAST_PROBS, emp=None,
             precision='mixed', device=None, first_step=0, want_traj=False):
    """The ensemble forecast of K policies (thetas, shifts, alpha_scales: scalars or K values) from the start rows `pi0`
    ((d,) or [N, d]; None: row 0 of each `emp` matrix) over `horizon` hours: `repeats` rollouts per start state and policy,
    reduced on the device.  Every policy uses the same seed and the Philox steps first_step .. first_step + horizon - 2: common
    random numbers, so policies are compared on the same noise, and with first_step = 0 policy k's members are the
    generate_trajectory rows of a fresh actor_critic(theta_k, shift_k, alpha_k, d, seed=seed) over the repeats-fold tiled start
    rows.  (seed may also be K values, one per policy: a trained population's learners at their own seeds.)  emp [N, >= horizon, >= d]
    (held-out rows): the error curves are returned too.  More than FORECAST_CHUNK policies go in chunks.  Returns a Forecast.
    Runs on a context of its own: a diverged mixed-precision policy raises MfgError and leaves the caller's status word alone."""
    if precision not in ('mixed', 'f64'):
        raise ValueError("precision must be 'mixed' or 'f64'")
    th = np.asarray(thetas, dtype=np.float64).reshape(-1)
    K = th.shape[0]
    if K < 1:
        raise ValueError('no policies')
    sh, al = broadcast('shifts', shifts, K), broadcast('alpha_scales', alpha_scales, K)
    sd = broadcast('seed', seed, K, np.uint64).view(np.int64)
    ranks = forecast_ranks(probs, repeats)
    start, emp = _forecast_inputs(pi0, emp, d, horizon)
    ops.check_forecast_args(start.shape, horizon, repeats, ranks, precision)
    if not torch.cuda.is_available():
        raise L.MfgError('forecast needs a ROCm GPU: the HIP hot path has no CPU fallback')
    L.lib()
    ops.init()
    dev = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
    ctx = ops.Context(dev)
    prev = ctx.bind_scoped()
    try:
        parts = []
        for c0 in range(0, K, FORECAST_CHUNK):
            n = min(FORECAST_CHUNK, K - c0)
            f = lambda a: torch.as_tensor(a[c0:c0 + n].copy(), device=dev)
            parts.append(forecast_policies(start, emp, f(th), f(sh), f(al), f(sd), int(horizon), int(first_step), int(repeats),
                                           ranks, precision, dev, ctx, want_traj))
    finally:
        ctx.restore(prev)
        ctx.close()
    cat = lambda key: None if parts[0][key] is None else np.concatenate([p[key] for p in parts])
    return Forecast(cat('mean'), cat('std'), cat('quant'), probs, ranks, cat('curves'), repeats, cat('traj'))


# ------------------------------------------------------------------------------------------------ scoring the forecast
# Whether the ensemble is any good: the proper scoring rules of a forecast distribution against the held-out rows (Gneiting &
# Raftery, JASA 2007) -- CRPS per topic, the energy score per histogram, and the rank of the observation among the members
# (PIT, band coverage) -- on the device (mfg_forecast_score), the members never leaving it.  The reference has no such scorer:
# its forecast is one sample path, scored by L1 / JSD (evaluate, mfg_ac2.py:595-670; the VAR baseline, var.py:330-416).
SCORE_HEADER = 'theta,shift,alpha_scale,crps_mean,crps_final,energy_mean,energy_final\n'
SCORE_FMT = '%f,%f,%f,%.6e,%.6e,%.6e,%.6e\n'


class ForecastScore:
    """The scores of a forecast (NumPy): crps [K, N, H, d]; less, equal [K, N, H, d] int32, the members below / equal to the
    fp32 observation (-1 where the cell holds a non-finite value or the learner failed); energy [K, N, H] or None; summary
    [K, H, 2], the mean CRPS over start rows and topics and the mean energy score over start rows, per hour.  A single-policy
    score (actor_critic.forecast_score) drops the leading K."""

    def __init__(self, crps, less, equal, energy, summary, repeats):
        self.crps, self.less, self.equal, self.energy, self.summary = crps, less, equal, energy, summary
        self.repeats = int(repeats)

    def learner(self, k):
        """Row k as a ForecastScore of its own."""
        pick = lambda a: None if a is None else a[k]
        return ForecastScore(pick(self.crps), pick(self.less), pick(self.equal), pick(self.energy), pick(self.summary),
                             self.repeats)


def pit(less, equal, repeats):
    """The probability integral transform of the observation among `repeats` members, ties split evenly:
    (less + equal / 2) / repeats.  Uniform on [0, 1] for a calibrated forecast.  Needs no GPU."""
    R = int(repeats)
    if R < 1:
        raise ValueError('repeats=%d: an ensemble has at least one member' % R)
    return (np.asarray(less, dtype=np.float64) + np.asarray(equal, dtype=np.float64) / 2.0) / R


def covered(less, equal, lo_rank, hi_rank):
    """Whether the observation lies inside the band of the ascending order statistics lo_rank .. hi_rank (0-based, as
    forecast_ranks names them): x_(lo) <= y <= x_(hi), i.e. (less + equal > lo_rank) & (less <= hi_rank).  Needs no GPU."""
    less, equal = np.asarray(less, dtype=np.int64), np.asarray(equal, dtype=np.int64)
    return (less + equal > int(lo_rank)) & (less <= int(hi_rank))


def forecast_score_bytes(N, horizon, d, repeats):
    """Device bytes one policy takes in a forecast_score chunk: its members, the forecast's and the score's workspaces and
    outputs (the byte counts of the library; needs no GPU)."""
    N, H, d, R = int(N), int(horizon), int(d), int(repeats)
    lib = L.lib()
    outputs = N * H * d * (8 + 8 + 8 + 4 + 4) + N * H * 8 + H * 2 * 8
    return (N * R * H * d * 4 + int(lib.mfg_forecast_pop_workspace_bytes(N, H, d, 1, R, 1))
            + int(lib.mfg_forecast_score_workspace_bytes(N, H, d, 1, R)) + outputs)


def forecast_score_policies(start, emp, thetas, shifts, alpha_scales, seeds, horizon, first_step, repeats, precision, device, ctx,
                            want_energy=True):
    """One ops.forecast_pop call for the members and one ops.forecast_score call on them, as NumPy arrays (crps, less, equal,
    energy, summary): `start` [N, d], `emp` [N, H, d] fp64 rows; `thetas`, `shifts`, `alpha_scales` fp64 and `seeds` int64
    device tensors [K].  Only the scores come to the host.  MfgError when a mixed-precision policy left the fp32 range."""
    start32 = torch.as_tensor(np.ascontiguousarray(start, dtype=np.float32), device=device)
    emp64 = torch.as_tensor(np.ascontiguousarray(emp, dtype=np.float64), device=device)
    emp32 = torch.as_tensor(np.ascontiguousarray(emp, dtype=np.float64).astype(np.float32), device=device)
    traj = ops.forecast_pop(start32, thetas, shifts, alpha_scales, seeds, horizon, first_step=first_step, repeats=repeats,
                            precision=precision, want_traj=True)['traj']
    out = ops.forecast_score(traj, emp32, emp64, start32.shape[0], repeats, want_energy=want_energy)
    host = {k: None if v is None else v.cpu().numpy() for k, v in out.items()}
    if precision == 'mixed' and ctx.status(synchronize=True):
        raise L.MfgError('a mixed-precision forecast ran a policy with |theta| (1 + |shift|) > 86 (or theta not finite): '
                         'its rows are NaN; use precision=\'f64\'')
    return host


def _score_inputs(pi0, emp, d, horizon):
    """(start, emp, horizon) of a forecast_score: `emp` is needed, `horizon` defaults to its rows.  ValueError otherwise."""
    if emp is None:
        raise ValueError('a forecast is scored against held-out rows: emp is needed')
    if horizon is None:
        e = np.asarray(emp)
        if e.ndim not in (2, 3):
            raise ValueError('emp: expected [N, H, >= d] or [H, >= d], got %s' % (e.shape,))
        horizon = e.shape[-2]
    start, emp = _forecast_inputs(pi0, emp, d, horizon)
    return start, emp, int(horizon)


def forecast_score(thetas, shifts, alpha_scales, emp, *, d, pi0=None, horizon=None, seed=0, repeats=256, precision='mixed',
                   device=None, first_step=0, want_energy=True, budget=None):
    """The proper scores of the ensemble forecast of K policies against the held-out rows `emp` [N, >= horizon, >= d]
    (horizon None: all its rows): the members are those of forecast() for the same arguments (start rows pi0, or row 0 of each
    emp matrix; common random numbers), scored on the device without coming to the host.  Policies go in chunks whose members,
    workspaces and outputs stay within `budget` bytes (None: CONSISTENCY_BUDGET; consistency_chunks) -- chunking changes no bit.
    want_energy=False skips the O(repeats^2 d) energy score.  Returns a ForecastScore.  Runs on a context of its own: a diverged
    mixed-precision policy raises MfgError and leaves the caller's status word alone."""
    if precision not in ('mixed', 'f64'):
        raise ValueError("precision must be 'mixed' or 'f64'")
    th = np.asarray(thetas, dtype=np.float64).reshape(-1)
    K = th.shape[0]
    if K < 1:
        raise ValueError('no policies')
    sh, al = broadcast('shifts', shifts, K), broadcast('alpha_scales', alpha_scales, K)
    sd = broadcast('seed', seed, K, np.uint64).view(np.int64)
    start, emp, H = _score_inputs(pi0, emp, d, horizon)
    ops.check_forecast_args(start.shape, H, repeats, (), precision)
    N, R = start.shape[0], int(repeats)
    chunks = consistency_chunks(K, forecast_score_bytes(N, H, int(d), R), budget)
    if not torch.cuda.is_available():
        raise L.MfgError('forecast_score needs a ROCm GPU: the HIP hot path has no CPU fallback')
    ops.init()
    dev = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
    ctx = ops.Context(dev)
    prev = ctx.bind_scoped()
    try:
        parts = []
        for c0, n in chunks:
            f = lambda a: torch.as_tensor(a[c0:c0 + n].copy(), device=dev)
            parts.append(forecast_score_policies(start, emp, f(th), f(sh), f(al), f(sd), H, int(first_step), R, precision, dev,
                                                 ctx, want_energy))
    finally:
        ctx.restore(prev)
        ctx.close()
    cat = lambda key: None if parts[0][key] is None else np.concatenate([p[key] for p in parts])
    return ForecastScore(cat('crps'), cat('less'), cat('equal'), cat('energy'), cat('summary'), R)


def score_columns(summary):
    """[K, 4] = (crps_mean, crps_final, energy_mean, energy_final) from a ForecastScore.summary [K, H, 2]: the means over the
    hours 1 .. H - 1 (hour 0 is the start row, which every member shares) and the last hour."""
    summary = np.asarray(summary, dtype=np.float64)
    return np.stack([summary[:, 1:, 0].mean(axis=1), summary[:, -1, 0], summary[:, 1:, 1].mean(axis=1), summary[:, -1, 1]], axis=1)


def best_score_points(points, table):
    """Per column of `table` [len(points), 4] the value and the point of the LAST minimum in grid order (best_points' `<=`),
    starting from [inf, 0, 0, 0]; a NaN never wins."""
    best = [[float('inf'), 0, 0, 0] for _ in range(4)]
    for (theta, shift, alpha_scale), res in zip(points, table):
        for idx in range(4):
            if res[idx] <= best[idx][0]:
                best[idx] = [float(res[idx]), theta, shift, alpha_scale]
    return best


def gridsearch_score(theta_range, shift_range, alpha_range, indir, outfile, *, d=21, seed=0, episode_length=16, repeats=64,
                     precision='mixed', device=None):
    """gridsearch with proper scores: every grid point's ensemble forecast (`repeats` members per test file of cwd/indir, from
    the file's row 0, common random numbers) is scored against the file's first `episode_length` rows by forecast_score.
    Appends one CSV line per point in the reference's theta-major order (SCORE_FMT; SCORE_HEADER first when the file is new or
    empty): the mean CRPS and energy score over hours 1 .. L - 1 and at hour L - 1, over all test files (and topics).  Returns,
    per column, [value, theta, shift, alpha_scale] of the last minimum in grid order.  gridsearch itself is unchanged."""
    if precision not in ('mixed', 'f64'):
        raise ValueError("precision must be 'mixed' or 'f64'")
    if not 1 <= int(repeats) <= L.FORECAST_MAX_REPEATS:
        raise ValueError('repeats=%d outside [1, %d]' % (repeats, L.FORECAST_MAX_REPEATS))
    emp = load_empirical(indir, int(d), int(episode_length))
    points = grid_points(theta_range, shift_range, alpha_range)
    if not points:
        return best_score_points(points, [])
    par = np.array(points, dtype=np.float64).reshape(-1, 3)
    score = forecast_score(par[:, 0].copy(), par[:, 1].copy(), par[:, 2].copy(), emp, d=int(d), horizon=int(episode_length),
                           seed=seed, repeats=int(repeats), precision=precision, device=device)
    table = score_columns(score.summary)
    header = not os.path.exists(outfile) or os.path.getsize(outfile) == 0
    with open(outfile, 'a') as f:
        if header:
            f.write(SCORE_HEADER)
        for point, res in zip(points, table):
            f.write(SCORE_FMT % (tuple(point) + tuple(res)))
    return best_score_points(points, table)


# ------------------------------------------------------------------------------------------ finite-population forecasts
# The members above follow pi' = P^T pi, the dynamics of infinitely many agents, and their only noise is the Dirichlet draw of P.
# Here a member is ONE population of `agents` agents (mfg_forecast_agents_pop): every agent of topic i picks its next topic from
# row P[i,:], so the histogram carries the sampling noise of order 1 / sqrt(agents) on top.  The same reductions and scores
# apply, which makes `agents` a parameter one can fit with them -- and the N-player check of the mean-field model: how large a
# population must be before the mean-field forecast holds.  The reference has no such path.
def apportion(pi, agents):
    """The start counts of a population of `agents` agents on the histogram rows `pi` ((d,) or [N, d]): int32, every row
    summing to `agents` (largest-remainder rounding).  With x = (double)(float)pi and s the sequential sum of a row in column
    order, q_i = x_i agents / s and c_i = floor(q_i); the agents - sum c_i left over go to the largest fractional parts q_i - c_i,
    ties to the lower index.  A row whose agents pi is integral (pi fp32-representable) is reproduced exactly.  NumPy, needs no
    GPU.  ValueError for agents outside [1, AGENTS_MAX], a negative or non-finite entry or a row that sums to 0."""
    agents = ops.check_agents(agents)
    x = np.asarray(pi, dtype=np.float64).astype(np.float32).astype(np.float64)
    if x.ndim not in (1, 2) or x.shape[-1] < 1:
        raise ValueError('pi: expected (d,) or [N, d], got %s' % (x.shape,))
    rows = x.reshape(-1, x.shape[-1])
    if not np.all(np.isfinite(rows)) or np.any(rows < 0):
        raise ValueError('pi: a histogram row holds a negative or non-finite entry')
    s = np.cumsum(rows, axis=1)[:, -1:]                  # (cumsum adds in column order)
    if np.any(s <= 0):
        raise ValueError('pi: a histogram row sums to 0')
    q = rows * float(agents) / s
    c = np.floor(q)
    counts = c.astype(np.int64)
    for r in range(rows.shape[0]):
        left = agents - int(counts[r].sum())
        frac = q[r] - c[r]
        # the q_i add up to agents within agents d 2^-51 < 1 (three roundings per term, d - 1 in s; agents <= 2^24, d < 2^27), and
        # sum floor(q_i) is a whole number not above that sum: never more than agents, and fewer than d short of it
        assert 0 <= left <= rows.shape[1], (left, agents)
        if left > 0:
            counts[r, np.argsort(-frac, kind='stable')[:left]] += 1
    return counts.astype(np.int32).reshape(x.shape)


def _agents_emp(emp, device):
    if emp is None:
        return None, None
    e64 = np.ascontiguousarray(emp, dtype=np.float64)
    return torch.as_tensor(e64.astype(np.float32), device=device), torch.as_tensor(e64, device=device)


def forecast_agents_policies(start, emp, agents, thetas, shifts, alpha_scales, seeds, horizon, first_step, repeats, ranks, precision,
                             device, ctx, want_traj=False, want_counts=False):
    """forecast_policies with finite-population members: one ops.forecast_agents_pop call from the counts apportion(start,
    agents), as NumPy arrays (mean, std, quant, curves, traj, counts)."""
    counts0 = torch.as_tensor(apportion(start, agents), device=device)
    emp32, emp64 = _agents_emp(emp, device)
    out = ops.forecast_agents_pop(counts0, agents, thetas, shifts, alpha_scales, seeds, horizon, first_step=first_step,
                                  repeats=repeats, ranks=ranks, precision=precision, emp32=emp32, emp64=emp64,
                                  want_traj=want_traj, want_counts=want_counts)
    host = {k: None if v is None else v.cpu().numpy() for k, v in out.items() if k != 'actions'}
    if precision == 'mixed' and ctx.status(synchronize=True):
        raise L.MfgError('a mixed-precision forecast ran a policy with |theta| (1 + |shift|) > 86 (or theta not finite): '
                         'the rows of its members are unspecified; use precision=\'f64\'')
    if host['quant'] is None:
        K, N = host['mean'].shape[:2]
        host['quant'] = np.zeros((K, N, int(horizon), 0, host['mean'].shape[-1]), dtype=np.float32)
    return host


def forecast_agents(thetas, shifts, alpha_scales, pi0, horizon, *, d, agents, seed=0, repeats=256, probs=FORECAST_PROBS, emp=None,
                    precision='mixed', device=None, first_step=0, want_traj=False, want_counts=False):
    """forecast() for populations of `agents` agents (one value for the call, 1 <= agents <= AGENTS_MAX): every member starts
    from the counts apportion(pi0 row, agents), draws its action as forecast()'s member does from its own histogram row (the
    same seed, Philox steps and member ids: common random numbers across policies) and then moves each agent by a draw from the
    action's row of the agent's topic.  As agents grows the members approach forecast()'s.  Returns a Forecast whose rows are
    the histogram rows counts / agents; want_counts adds Forecast.counts [K, N repeats, horizon, d] int32.  Chunks, context and
    errors as forecast()."""
    if precision not in ('mixed', 'f64'):
        raise ValueError("precision must be 'mixed' or 'f64'")
    th = np.asarray(thetas, dtype=np.float64).reshape(-1)
    K = th.shape[0]
    if K < 1:
        raise ValueError('no policies')
    sh, al = broadcast('shifts', shifts, K), broadcast('alpha_scales', alpha_scales, K)
    sd = broadcast('seed', seed, K, np.uint64).view(np.int64)
    ranks = forecast_ranks(probs, repeats)
    start, emp = _forecast_inputs(pi0, emp, d, horizon)
    agents = ops.check_forecast_agents_args(start.shape, agents, horizon, repeats, ranks, precision)[-1]
    apportion(start, agents)                             # (its ValueErrors ahead of the GPU)
    if not torch.cuda.is_available():
        raise L.MfgError('forecast_agents needs a ROCm GPU: the HIP hot path has no CPU fallback')
    L.lib()
    ops.init()
    dev = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
    ctx = ops.Context(dev)
    prev = ctx.bind_scoped()
    try:
        parts = []
        for c0 in range(0, K, FORECAST_CHUNK):
            n = min(FORECAST_CHUNK, K - c0)
            f = lambda a: torch.as_tensor(a[c0:c0 + n].copy(), device=dev)
            parts.append(forecast_agents_policies(start, emp, agents, f(th), f(sh), f(al), f(sd), int(horizon), int(first_step),
                                                  int(repeats), ranks, precision, dev, ctx, want_traj, want_counts))
    finally:
        ctx.restore(prev)
        ctx.close()
    cat = lambda key: None if parts[0][key] is None else np.concatenate([p[key] for p in parts])
    return Forecast(cat('mean'), cat('std'), cat('quant'), probs, ranks, cat('curves'), repeats, cat('traj'), counts=cat('counts'))


def forecast_agents_score_bytes(N, horizon, d, repeats):
    """forecast_score_bytes with the finite-population forecast's workspace (the members given, the counts in the workspace)."""
    N, H, d, R = int(N), int(horizon), int(d), int(repeats)
    lib = L.lib()
    outputs = N * H * d * (8 + 8 + 8 + 4 + 4) + N * H * 8 + H * 2 * 8
    return (N * R * H * d * 4 + int(lib.mfg_forecast_agents_pop_workspace_bytes(N, H, d, 1, R, 1, 0))
            + int(lib.mfg_forecast_score_workspace_bytes(N, H, d, 1, R)) + outputs)


def forecast_agents_score_policies(start, emp, agents, thetas, shifts, alpha_scales, seeds, horizon, first_step, repeats, precision,
                                   device, ctx, want_energy=True):
    """forecast_score_policies with finite-population members: one ops.forecast_agents_pop call for the members and one
    ops.forecast_score call on them; only the scores come to the host."""
    counts0 = torch.as_tensor(apportion(start, agents), device=device)
    emp32, emp64 = _agents_emp(emp, device)
    traj = ops.forecast_agents_pop(counts0, agents, thetas, shifts, alpha_scales, seeds, horizon, first_step=first_step,
                                   repeats=repeats, precision=precision, want_traj=True)['traj']
    out = ops.forecast_score(traj, emp32, emp64, counts0.shape[0], repeats, want_energy=want_energy)
    host = {k: None if v is None else v.cpu().numpy() for k, v in out.items()}
    if precision == 'mixed' and ctx.status(synchronize=True):
        raise L.MfgError('a mixed-precision forecast ran a policy with |theta| (1 + |shift|) > 86 (or theta not finite): '
                         'the rows of its members are unspecified; use precision=\'f64\'')
    return host


def forecast_agents_score(thetas, shifts, alpha_scales, emp, *, d, agents, pi0=None, horizon=None, seed=0, repeats=256,
                          precision='mixed', device=None, first_step=0, want_energy=True, budget=None):
    """forecast_score() of forecast_agents()'s members: the proper scores of the finite-population ensemble of K policies
    against the held-out rows `emp`, scored by the same ops.forecast_score without the members coming to the host.  Chunks under
    `budget` as forecast_score (chunking changes no bit).  Returns a ForecastScore."""
    if precision not in ('mixed', 'f64'):
        raise ValueError("precision must be 'mixed' or 'f64'")
    th = np.asarray(thetas, dtype=np.float64).reshape(-1)
    K = th.shape[0]
    if K < 1:
        raise ValueError('no policies')
    sh, al = broadcast('shifts', shifts, K), broadcast('alpha_scales', alpha_scales, K)
    sd = broadcast('seed', seed, K, np.uint64).view(np.int64)
    start, emp, H = _score_inputs(pi0, emp, d, horizon)
    agents = ops.check_forecast_agents_args(start.shape, agents, H, repeats, (), precision)[-1]
    apportion(start, agents)
    N, R = start.shape[0], int(repeats)
    chunks = consistency_chunks(K, forecast_agents_score_bytes(N, H, int(d), R), budget)
    if not torch.cuda.is_available():
        raise L.MfgError('forecast_agents_score needs a ROCm GPU: the HIP hot path has no CPU fallback')
    ops.init()
    dev = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
    ctx = ops.Context(dev)
    prev = ctx.bind_scoped()
    try:
        parts = []
        for c0, n in chunks:
            f = lambda a: torch.as_tensor(a[c0:c0 + n].copy(), device=dev)
            parts.append(forecast_agents_score_policies(start, emp, agents, f(th), f(sh), f(al), f(sd), H, int(first_step), R,
                                                        precision, dev, ctx, want_energy))
    finally:
        ctx.restore(prev)
        ctx.close()
    cat = lambda key: None if parts[0][key] is None else np.concatenate([p[key] for p in parts])
    return ForecastScore(cat('crps'), cat('less'), cat('equal'), cat('energy'), cat('summary'), R)


# --------------------------------------------------------------------------------------------- backward-equation check
# The scoring half of the reference's synthetic sweep (evaluate_synthetic / evaluate_synthetic_JSD, mfg_synthetic.py:741-899,
# once per learner in its __main__, :902-925) for K policies at once: one mfg_consistency_pop call rolls every policy from
# every start row, runs the backward recursion over the actions and reduces both metrics on the device.
CONSISTENCY_BUDGET = 1 << 30    # workspace bytes of one consistency_pop call of consistency() (more policies go in chunks)
SYNTHETIC_HOURS = 16            # rows per trajectory of evaluate_synthetic (mfg_synthetic.py:759, :838)


def consistency_chunks(K, bytes_per_policy, budget=None):
    """[(first, count), ...]: the K policies in order, in chunks whose workspace (count x bytes_per_policy, an upper bound of
    mfg_consistency_pop_workspace_bytes at that count) stays within `budget` (None: CONSISTENCY_BUDGET), at most POP_MAX_K per chunk.  ValueError when
    one policy alone exceeds the budget.  Needs no GPU."""
    K, per, budget = int(K), int(bytes_per_policy), int(CONSISTENCY_BUDGET if budget is None else budget)
    if K < 1:
        raise ValueError('no policies')
    if per < 1:
        raise ValueError('bytes_per_policy=%d' % per)
    if per > budget:
        raise ValueError('one policy needs %d bytes of workspace, the budget is %d: fewer start rows, repeats or hours'
                         % (per, budget))
    n = min(budget // per, L.POP_MAX_K)
    return [(c0, min(n, K - c0)) for c0 in range(0, K, n)]


class Consistency:
    """The result of a backward-equation check (NumPy): l1_mean, l1_std, jsd_mean, jsd_std, each [K] -- mean and std (ddof = 0)
    over the policy's N R (hours - 1) values of sum_ij |P_ij - value_ij| and of sum_i JSD(P_i, implied row i); steps
    [K, N R, hours - 1, 2] (l1, jsd per trajectory and hour) when asked for, else None."""

    def __init__(self, metrics, steps=None):
        self.metrics = metrics
        self.l1_mean, self.l1_std, self.jsd_mean, self.jsd_std = (metrics[:, q].copy() for q in range(4))
        self.steps = steps


def consistency_policies(start, thetas, shifts, alpha_scales, seeds, hours, first_step, repeats, precision, device, ctx,
                         want_steps=False):
    """One ops.consistency_pop call as NumPy arrays (metrics [K, 4], steps or None): `start` [N, d] fp64 rows; `thetas`,
    `shifts`, `alpha_scales` fp64 and `seeds` int64 device tensors [K].  MfgError when a mixed-precision policy left the fp32
    range (ctx: the bound context whose status word the launch reports into)."""
    start32 = torch.as_tensor(np.ascontiguousarray(start, dtype=np.float32), device=device)
    out = ops.consistency_pop(start32, thetas, shifts, alpha_scales, seeds, hours, first_step=first_step, repeats=repeats,
                              precision=precision, want_steps=want_steps)
    metrics = out['metrics'].cpu().numpy()
    steps = out['steps'].cpu().numpy() if want_steps else None
    if precision == 'mixed' and ctx.status(synchronize=True):
        raise L.MfgError('a mixed-precision backward-equation check ran a policy with |theta| (1 + |shift|) > 86 (or theta not '
                         'finite): its metrics are NaN; use precision=\'f64\'')
    return metrics, steps


def _consistency_start(pi0, d):
    """The start rows [N, d] fp64 of a backward-equation check from `pi0` ((d,) or [N, >= d]).  ValueError otherwise."""
    d = int(d)
    if not 1 <= d <= 64:
        raise ValueError('d=%d: the backward-equation check covers d <= 64 (as the populations do)' % d)
    if pi0 is None:
        raise ValueError('a backward-equation check needs start rows (pi0)')
    start = np.asarray(pi0, dtype=np.float64)
    if start.ndim == 1:
        start = start[None]
    if start.ndim != 2 or start.shape[0] < 1 or start.shape[1] < d:
        raise ValueError('pi0: expected (d,) or [N, d] with d >= %d, got %s' % (d, start.shape))
    return np.ascontiguousarray(start[:, :d])


def consistency(thetas, shifts, alpha_scales, pi0, *, d, seed=0, hours=SYNTHETIC_HOURS, repeats=1, precision='mixed', device=None,
                first_step=0, want_steps=False):
    """The backward-equation check of K policies (thetas, shifts, alpha_scales: scalars or K values) from the start rows `pi0`
    ((d,) or [N, d]): `repeats` rollouts of `hours` rows per start row and policy, V^n = r^n + P^n V^{n+1} over their actions
    and the two consistency metrics, reduced on the device.  Every policy uses the same seed and the Philox steps first_step ..
    first_step + hours - 2: common random numbers, and with first_step = 0 policy k's actions are those a fresh
    mfg_synthetic.actor_critic(theta_k, shift_k, alpha_k, d, seed=seed, pi0=...) returns from generate_trajectory over the
    repeats-fold tiled start rows.  (seed may also be K values, one per policy.)  Policies go in chunks whose workspace stays
    within CONSISTENCY_BUDGET (consistency_chunks).  Returns a Consistency.  Runs on a context of its own: a diverged
    mixed-precision policy raises MfgError and leaves the caller's status word alone."""
    th = np.asarray(thetas, dtype=np.float64).reshape(-1)
    K = th.shape[0]
    if K < 1:
        raise ValueError('no policies')
    sh, al = broadcast('shifts', shifts, K), broadcast('alpha_scales', alpha_scales, K)
    sd = broadcast('seed', seed, K, np.uint64).view(np.int64)
    start = _consistency_start(pi0, d)
    N, d, H, R = ops.check_consistency_args(start.shape, hours, repeats, precision, 1, first_step)
    if not torch.cuda.is_available():
        raise L.MfgError('consistency needs a ROCm GPU: the HIP hot path has no CPU fallback')
    L.lib()
    ops.init()
    chunks = consistency_chunks(K, ops.consistency_pop_workspace_bytes(N, H, d, 1, R, want_steps, False, False))
    dev = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
    ctx = ops.Context(dev)
    prev = ctx.bind_scoped()
    try:
        parts = []
        for c0, n in chunks:
            f = lambda a: torch.as_tensor(a[c0:c0 + n].copy(), device=dev)
            parts.append(consistency_policies(start, f(th), f(sh), f(al), f(sd), H, int(first_step), R, precision, dev, ctx,
                                              want_steps))
    finally:
        ctx.restore(prev)
        ctx.close()
    return Consistency(np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]) if want_steps else None)


def check_synthetic_eval(reward, num_start, day_first, day_last, repeats=1):
    """The argument rules of evaluate_synthetic / evaluate_synthetic_JSD of a population (ValueError; no GPU needed): the
    synthetic reward, start rows day_first .. day_last inside the table of `num_start` rows, repeats >= 1.  Returns (day_first,
    day_last, repeats) as ints."""
    if reward != 'synthetic':
        raise ValueError("evaluate_synthetic checks the backward equation of the synthetic reward: the population has "
                         "reward=%r" % (reward,))
    day_first, day_last, repeats = int(day_first), int(day_last), int(repeats)
    if not 1 <= day_first <= day_last <= int(num_start):
        raise ValueError('days %d .. %d outside the start table\'s rows 1 .. %d' % (day_first, day_last, num_start))
    if repeats < 1:
        raise ValueError('repeats=%d: at least one rollout per start row' % repeats)
    return day_first, day_last, repeats


class _Population:
    """What ActorCriticPopulation and AC_IRLPopulation share: the K learners' theta, w, shifts, alpha_scales and seeds (host
    and device copies), the start-state table, the Philox step counter and the instance's own ops.Context.  Subclasses say
    whether their buffers hold the actions P (_WITH_P) and build their learner's single-learner object (_new_learner)."""
    _WITH_P = False

    def __init__(self, th, d, batch, episode_steps, shifts, alpha_scales, seeds, w0, pi0, path_to_dir, update_every, precision,
                 device, verbose):
        K = th.shape[0]
        if not torch.cuda.is_available():
            raise L.MfgError('%s needs a ROCm GPU: the HIP hot path has no CPU fallback' % type(self).__name__)
        L.lib()
        ops.init()
        self.device = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
        self._ctx = ops.Context(self.device)
        self.d, self.batch, self.episode_steps = int(d), int(batch), int(episode_steps)
        self.update_every, self.precision, self.verbose = update_every, precision, verbose
        F = ops.num_features(self.d)
        self.shifts = broadcast('shifts', shifts, K)
        self.alpha_scales = broadcast('alpha_scales', alpha_scales, K)
        self.seeds = broadcast('seeds', np.arange(K) if seeds is None else seeds, K, np.uint64)
        dev = self.device
        self._theta = torch.as_tensor(th.copy(), device=dev)
        # critic weights first, start states second: actor_critic's np.random consumption order, learner by learner
        if w0 is None:
            w = np.stack([np.asarray(actor_critic.init_w(None, self.d), dtype=np.float64).reshape(-1) for _ in range(K)])
        else:
            w = np.asarray(w0, dtype=np.float64)
            w = np.broadcast_to(w.reshape(1, -1), (K, F)) if w.size == F else w.reshape(K, F)
        self._w = torch.as_tensor(np.array(w, dtype=np.float64, order='C'), device=dev)   # (a C-ordered copy of a broadcast view)
        # the start-state table, resolved as actor_critic resolves it, shared by all learners
        self.mat_pi0 = resolve_start_table(self.d, pi0, path_to_dir)
        self._mat_pi0_dev = torch.as_tensor(np.ascontiguousarray(self.mat_pi0, dtype=np.float32), device=dev)
        self._seeds_dev = torch.as_tensor(self.seeds.view(np.int64), device=dev)
        self._shifts_dev = torch.as_tensor(self.shifts, device=dev)
        self._alphas_dev = torch.as_tensor(self.alpha_scales, device=dev)
        self._rng_step = 0  # Philox step counter, shared by the learners (they advance in lock-step)
        self._bufs = None
        # per-learner activity (the population control block): host mirrors, read back with train()'s one synchronisation
        self._act = LearnerActivity(K)
        self._ctl = None     # the block's device tensors, made by the first train() call that needs one
        self.validation = None     # the ValidationTrace of the last train(..., validate=...) call
        self._val_dev = None       # its snapshots (best_theta, best_w) on the device, for restore_best
        self.evolution = None      # the EvolutionTrace of the last train(..., evolve=...) call

    # ------------------------------------------------------------------ state
    @property
    def K(self):
        return int(self._theta.shape[0])

    @property
    def thetas(self):
        return self._theta.cpu().numpy().copy()

    @property
    def w(self):
        return self._w.cpu().numpy().copy()

    @property
    def learner_state(self):
        """[K] of 0 (active), 1 (stopped early in the last train() call) or 2 (failed, until clear_status)."""
        return self._act.state.copy()

    @property
    def episodes_run(self):
        """[K] episodes each learner completed while active in the last train() call (a call without a control block: all of
        its episodes)."""
        return self._act.episodes.copy()

    @property
    def learner_status(self):
        """[K] status bits of each learner's own word (_lib.STATUS_MIXED_RANGE, _lib.STATUS_POP_NONFINITE; 0 = healthy)."""
        return self._act.status.copy()

    def _healthy(self):
        """The learners that have not failed, in order."""
        return self._act.healthy()

    def loglik(self, demos, days=None):
        """The Dirichlet-multinomial log-likelihood of the moves of `demos` (a demos.Demonstrations; days: None for all) under
        the K learners' current policies (theta_k, shift_k, alpha_scale_k), in one call: a likelihood.LogLik with ll [K, N, H-1],
        ll_day [K, N], grad_day [K, N, 3], status [K, N] and total(days)."""
        from . import likelihood
        return likelihood.loglik(demos, self._theta.reshape(-1), self.shifts, self.alpha_scales, days, device=self.device)

    def _buffers(self):
        K, B, d, T = self.K, self.batch, self.d, self.episode_steps
        if self._bufs is None:
            dev, F = self.device, ops.num_features(d)
            b = {'G': torch.zeros(K, F + 3, dtype=torch.float64, device=dev),
                 'ws': torch.zeros(K, ops.pop_workspace_slice(B, d, T) // 8, dtype=torch.float64, device=dev)}
            step = self.update_every == 'step'
            n = (K, B) if step else (K, B, T)      # reward / delta / g: one entry per env step of a learner
            if step:
                b['pi'] = torch.empty(K, B, d, dtype=torch.float32, device=dev)
                run = {'scratch': torch.empty(K, B, d, dtype=torch.float32, device=dev)}
            else:
                run = {'pi_traj': torch.empty(K, B, T + 1, d, dtype=torch.float32, device=dev),
                       'pi_last': torch.empty(K, B, d, dtype=torch.float32, device=dev)}
            if self._WITH_P:
                run['P'] = torch.empty(*n, d, d, dtype=torch.float32, device=dev)
            run.update(reward=torch.empty(*n, dtype=torch.float32, device=dev),
                       delta=torch.empty(*n, dtype=torch.float64, device=dev),
                       g=torch.empty(*n, dtype=torch.float64, device=dev))
            b['run'] = run
            self._bufs = b
        return self._bufs

    # ------------------------------------------------------------------ training
    def _validated(self, validate, num_episodes, run):
        """`run` wrapped in the validation block of `validate` for one train() call: reserves the checks' Philox steps
        (first_step = the counter, which moves on by L - 1 BEFORE the first training episode), makes the block's device arrays
        -- curve sized to exactly num_episodes // period rows --, binds the block around run() and leaves the results on
        self.validation (finish(), called once the call's one synchronisation has happened)."""
        K, dev, F = self.K, self.device, ops.num_features(self.d)
        emp = validate.rows(self.d)
        N, Lr, _ = emp.shape
        C = int(num_episodes) // validate.period
        first_step = self._rng_step
        if first_step + Lr - 1 + int(num_episodes) * self.episode_steps > 0xFFFFFFFF:
            raise ValueError('validate: the Philox step counter would wrap')
        self._rng_step += Lr - 1
        v = {'curve': torch.full((K, max(C, 1), L.POP_VALIDATE_COLUMNS), float('nan'), dtype=torch.float64, device=dev),
             'ints': torch.zeros(3, K, dtype=torch.int32, device=dev),       # checks | best_check | since_best
             'best_value': torch.full((K,), float('inf'), dtype=torch.float64, device=dev),
             'best_theta': torch.full((K,), float('nan'), dtype=torch.float64, device=dev),
             'best_w': torch.full((K, F), float('nan'), dtype=torch.float64, device=dev)}
        v['ints'][1].fill_(-1)

        def bound_run(*args):
            if C == 0:                               # (no check falls into this call: nothing to bind)
                return run(*args)
            emp64 = torch.as_tensor(emp, dtype=torch.float64, device=dev)
            emp32 = torch.as_tensor(emp.astype(np.float32), device=dev)
            ws = ops.pop_validate_workspace(N, Lr, self.d, K, validate.repeats, validate.score, dev)
            self._ctx.set_pop_validate(emp32, emp64, period=validate.period, column=validate.column, with_score=validate.score,
                                       patience=validate.patience, first_step=first_step, repeats=validate.repeats,
                                       curve=v['curve'], checks=v['ints'][0], best_value=v['best_value'],
                                       best_check=v['ints'][1], since_best=v['ints'][2], best_theta=v['best_theta'],
                                       best_w=v['best_w'], workspace=ws)
            try:
                return run(*args)
            except L.MfgError as e:
                if e.code:                           # refused by the library before anything was launched
                    self._rng_step = first_step
                raise
            finally:
                self._ctx.set_pop_validate()

        def finish():
            ints = v['ints'].cpu().numpy()
            self._val_dev = (v['best_theta'], v['best_w'])
            self.validation = ValidationTrace(v['curve'][:, :C].cpu().numpy(), ints[0].copy(), validate.period,
                                              v['best_value'].cpu().numpy(), ints[1].copy(), v['best_theta'].cpu().numpy(),
                                              v['best_w'].cpu().numpy(), validate.column)
        return bound_run, finish

    def _evolved(self, evolve, validate, num_episodes, run):
        """`run` wrapped in the evolve block of `evolve` for one train() call: makes the logs -- sized to exactly
        (num_episodes // period) // every steps --, binds the block to the call's own learning-rate tensors around run() and
        leaves the results on self.evolution (finish(), called once the call's one synchronisation has happened)."""
        K, dev = self.K, self.device
        n_top, n_bottom = evolve.counts(K)
        S = (int(num_episodes) // validate.period) // evolve.every
        e = {'ints': torch.full((2, K, max(S, 1)), -1, dtype=torch.int32, device=dev),          # rank | parent
             'lr_log': torch.full((K, max(S, 1), 2), float('nan'), dtype=torch.float64, device=dev),
             'scratch': torch.zeros(K + 1, dtype=torch.int32, device=dev)}                      # order | active
        rates = []

        def bound_run(b, lrc, lra, acc):
            rates[:] = [lrc, lra]
            if S == 0:                               # (no step falls into this call: nothing to bind)
                return run(b, lrc, lra, acc)
            self._ctx.set_pop_evolve(lrc, lra, every=evolve.every, n_top=n_top, n_bottom=n_bottom, perturb=evolve.perturb_bits,
                                     factors=evolve.factors, lr_critic_bounds=evolve.lr_critic_bounds,
                                     lr_actor_bounds=evolve.lr_actor_bounds, seed=evolve.seed, order=e['scratch'][:K],
                                     active=e['scratch'][K:], rank=e['ints'][0], parent=e['ints'][1], lr_log=e['lr_log'])
            try:
                return run(b, lrc, lra, acc)
            finally:
                self._ctx.set_pop_evolve()

        def finish():
            ints = e['ints'][:, :, :S].cpu().numpy()
            self.evolution = EvolutionTrace(ints[0].copy(), ints[1].copy(), e['lr_log'][:, :S].cpu().numpy(),
                                            rates[0].cpu().numpy(), rates[1].cpu().numpy(), evolve.every)
        return bound_run, finish

    def restore_best(self, k=None):
        """Copy the best held-out iterate of the last train(..., validate=...) call -- theta and w as they were at the check
        validation.best_check -- back into learner k (None: every learner that recorded one).  ValueError for a learner
        without one (k given), or when no validated call has run."""
        if self.validation is None:
            raise ValueError('restore_best: no train(..., validate=...) call has run')
        have = self.validation.best_check >= 0
        if k is not None:
            if not 0 <= int(k) < self.K:
                raise IndexError('learner %d of %d' % (k, self.K))
            if not have[int(k)]:
                raise ValueError('restore_best: learner %d has no recorded best iterate' % int(k))
            have = np.arange(self.K) == int(k)
        sel = torch.as_tensor(np.flatnonzero(have), device=self.device)
        best_theta, best_w = self._val_dev
        self._theta[sel] = best_theta[sel]
        self._w[sel] = best_w[sel]

    def _train(self, num_episodes, lr_critic, lr_actor, run, stop_criteria=-1, isolate=False, validate=None, evolve=None):
        """The frame of train(): checks, learning rates as device arrays [K], run(buffers, lrc, lra, acc) -- the native calls
        -- and the Philox step; returns acc [K, num_episodes] as a NumPy array.  MfgError when a mixed-precision launch left the
        fp32 range.  A stop criterion, isolate=True or a learner that failed earlier: the call runs under the population's
        control block (set on the context for the call only) and the per-learner states are read back with acc."""
        K = self.K
        num_episodes = int(num_episodes)
        if num_episodes < 0:
            raise ValueError('num_episodes < 0')
        lrc = torch.as_tensor(broadcast('lr_critic', lr_critic, K), device=self.device)
        lra = torch.as_tensor(broadcast('lr_actor', lr_actor, K), device=self.device)
        stop = stop_criteria_array(stop_criteria, K)
        control = needs_control(stop, isolate, self._act.state)
        finish = None
        if evolve is not None:
            if not isinstance(evolve, Evolution):
                raise TypeError('evolve: expected a population.Evolution or None')
            if validate is None:
                raise ValueError('evolve: the exploit / explore steps follow held-out checks; give validate= too')
            evolve.counts(K)
        if validate is not None:
            if not isinstance(validate, Validation):
                raise TypeError('validate: expected a population.Validation or None')
            control = control or validate.patience > 0     # (the patience stop moves the control block's states)
            if num_episodes > 0:
                if evolve is not None:
                    run, finish_evolve = self._evolved(evolve, validate, num_episodes, run)
                run, finish_validate = self._validated(validate, num_episodes, run)
                finish = finish_validate if evolve is None else (lambda: (finish_validate(), finish_evolve()))
        if not control:
            # (no learner has failed here, or the call would be a controlled one: everybody is active for the whole call)
            self._act.state[:] = ACTIVE
            self._act.episodes[:] = num_episodes
        if num_episodes == 0 and not control:
            return np.zeros((K, 0))
        acc = torch.zeros(K, num_episodes, dtype=torch.float64, device=self.device)
        if not control:
            run(self._buffers(), lrc, lra, acc)
            self._rng_step += num_episodes * self.episode_steps
            out = acc.cpu().numpy()
            if finish:
                finish()
            if self.precision == 'mixed' and self._ctx.status(synchronize=True):
                raise L.MfgError('a mixed-precision sampling launch of this population ran with |theta| (1 + |shift|) > 86 '
                                 '(or theta not finite): its outputs are NaN; use precision=\'f64\', then clear_status()')
            return out
        if self._ctl is None:
            self._ctl = {'ints': torch.zeros(3, K, dtype=torch.int32, device=self.device),     # state | status | episodes_run
                         'theta_prev': torch.zeros(K, dtype=torch.float64, device=self.device),
                         'stop': torch.zeros(K, dtype=torch.float64, device=self.device)}
        c = self._ctl
        # `stopped` is reset by every call, `failed` (with its status bits) persists until clear_status
        failed = self._act.state == 2
        host = np.zeros((3, K), dtype=np.int32)
        host[0, failed] = 2
        host[1, failed] = self._act.status[failed]
        c['ints'].copy_(torch.from_numpy(host))
        c['stop'].copy_(torch.from_numpy(stop))
        self._ctx.set_pop_control(c['ints'][0], c['ints'][1], c['theta_prev'], c['ints'][2], c['stop'])
        try:
            run(self._buffers(), lrc, lra, acc)
        finally:
            self._ctx.set_pop_control()
        self._rng_step += num_episodes * self.episode_steps
        out = acc.cpu().numpy()
        if finish:
            finish()
        ints = c['ints'].cpu().numpy()
        self._act.state, self._act.status, self._act.episodes = ints[0].copy(), ints[1].copy(), ints[2].copy()
        if self.precision == 'mixed' and self._ctx.status(synchronize=False):
            raise L.MfgError('a mixed-precision sampling launch of this population ran with |theta| (1 + |shift|) > 86 '
                             '(or theta not finite): its outputs are NaN; use precision=\'f64\', then clear_status()')
        if not isolate and np.any(self._act.state == 2):
            raise L.MfgError('learner(s) %s of this population failed (theta outside |theta| (1 + |shift|) <= 86 in mixed '
                             'precision, or theta / w not finite; learner_status has the bits): they are frozen, the others '
                             'trained on; isolate=True does not raise, clear_status() revives them'
                             % np.flatnonzero(self._act.state == 2).tolist())
        return out

    def status(self, synchronize=True) -> int:
        """Bits of this population's status word (0 = healthy), shared by its K learners."""
        return self._ctx.status(synchronize)

    def clear_status(self, k=None):
        """Reset the context's status word and revive the failed learner k (None: all of them): its state and status bits go
        back to 0 -- give it a theta (and w) it can train with first."""
        self._ctx.clear_status()
        self._act.clear(k)

    def _evaluate(self, episode_length, indir, outfile, write_header, repeats):
        """The body of evaluate() (the population's context bound)."""
        if int(repeats) < 1:
            raise ValueError('repeats=%d: at least one rollout per test file' % repeats)
        emp = load_empirical(indir, self.d, int(episode_length))
        first_step = self._rng_step
        self._rng_step += int(episode_length) - 1    # (a diverged launch has run: its step is spent, as in train())
        live = self._healthy()                       # failed learners are not launched: NaN rows, no CSV line
        sub = (lambda t: t) if len(live) == self.K else (lambda t: t[torch.as_tensor(live, device=self.device)].contiguous())
        table = np.full((self.K, 8), np.nan)
        try:
            if live:
                table[live] = evaluate_policies(emp, sub(self._theta), sub(self._shifts_dev), sub(self._alphas_dev),
                                                sub(self._seeds_dev), first_step, int(repeats), self.precision, self.device,
                                                self._ctx)
        except L.MfgError as e:
            if e.code:                               # refused by the library before anything was launched
                self._rng_step = first_step
            raise
        thetas = self.thetas
        write_eval_rows(outfile, write_header, [(float(thetas[k]), float(self.shifts[k]), float(self.alpha_scales[k]))
                                                for k in live], table[live])
        return table[:, 0::2].copy()

    @_with_ctx
    def forecast(self, pi0=None, indir=None, horizon=16, repeats=256, probs=FORECAST_PROBS, *, want_traj=False):
        """The ensemble forecast of every learner's current policy in one forecast_pop call (a Forecast with a leading K):
        learner k rolls `repeats` members per start row with its own seed from the population's Philox step.  Start rows: `pi0`
        ((d,) or [N, d]), or row 0 of each file of cwd/indir; with indir the files' first `horizon` rows are the held-out rows
        and the error curves are returned.  Advances the Philox step by horizon - 1, as each learner's own forecast() would
        (restored when the library refuses the call).  Failed learners are not launched: NaN rows.  MfgError when a
        mixed-precision policy left the fp32 range."""
        emp = load_empirical(indir, self.d, int(horizon)) if indir is not None else None
        ranks = forecast_ranks(probs, repeats)
        start, emp = _forecast_inputs(pi0, emp, self.d, horizon)
        ops.check_forecast_args(start.shape, horizon, repeats, ranks, self.precision)
        H, R = int(horizon), int(repeats)
        first_step = self._rng_step
        self._rng_step += H - 1                      # (a diverged launch has run: its step is spent, as in train())
        live = self._healthy()
        sub = (lambda t: t) if len(live) == self.K else (lambda t: t[torch.as_tensor(live, device=self.device)].contiguous())
        N, Q = start.shape[0], len(ranks)
        res = {'mean': np.full((self.K, N, H, self.d), np.nan), 'std': np.full((self.K, N, H, self.d), np.nan),
               'quant': np.full((self.K, N, H, Q, self.d), np.nan, dtype=np.float32),
               'curves': None if emp is None else np.full((self.K, H, 4), np.nan),
               'traj': np.full((self.K, N * R, H, self.d), np.nan, dtype=np.float32) if want_traj else None}
        try:
            if live:
                got = forecast_policies(start, emp, sub(self._theta), sub(self._shifts_dev), sub(self._alphas_dev),
                                        sub(self._seeds_dev), H, first_step, R, ranks, self.precision, self.device, self._ctx,
                                        want_traj)
                for key, a in res.items():
                    if a is not None:
                        a[live] = got[key]
        except L.MfgError as e:
            if e.code:                               # refused by the library before anything was launched
                self._rng_step = first_step
            raise
        return Forecast(res['mean'], res['std'], res['quant'], probs, ranks, res['curves'], R, res['traj'])

    @_with_ctx
    def forecast_score(self, pi0=None, indir=None, horizon=16, repeats=256, *, emp=None, want_energy=True):
        """The proper scores (a ForecastScore with a leading K) of every learner's ensemble forecast against held-out rows: the
        first `horizon` rows of each file of cwd/indir, or `emp` [N, >= horizon, >= d].  The members are those forecast() rolls
        from the same state (start rows `pi0`, or row 0 of each held-out matrix; learner k's own seed, the population's Philox
        step) and stay on the device.  Advances the Philox step by horizon - 1, as forecast() does (restored when the library
        refuses the call).  Failed learners are not launched: NaN rows, counts -1.  MfgError when a mixed-precision policy left
        the fp32 range."""
        if (indir is None) == (emp is None):
            raise ValueError('a forecast is scored against held-out rows: give indir or emp (not both)')
        if indir is not None:
            emp = load_empirical(indir, self.d, int(horizon))
        start, emp, H = _score_inputs(pi0, emp, self.d, horizon)
        ops.check_forecast_args(start.shape, H, repeats, (), self.precision)
        R, N = int(repeats), start.shape[0]
        first_step = self._rng_step
        self._rng_step += H - 1                      # (a diverged launch has run: its step is spent, as in train())
        live = self._healthy()
        sub = (lambda t: t) if len(live) == self.K else (lambda t: t[torch.as_tensor(live, device=self.device)].contiguous())
        res = {'crps': np.full((self.K, N, H, self.d), np.nan), 'less': np.full((self.K, N, H, self.d), -1, dtype=np.int32),
               'equal': np.full((self.K, N, H, self.d), -1, dtype=np.int32),
               'energy': np.full((self.K, N, H), np.nan) if want_energy else None, 'summary': np.full((self.K, H, 2), np.nan)}
        try:
            if live:
                got = forecast_score_policies(start, emp, sub(self._theta), sub(self._shifts_dev), sub(self._alphas_dev),
                                              sub(self._seeds_dev), H, first_step, R, self.precision, self.device, self._ctx,
                                              want_energy)
                for key, a in res.items():
                    if a is not None:
                        a[live] = got[key]
        except L.MfgError as e:
            if e.code:                               # refused by the library before anything was launched
                self._rng_step = first_step
            raise
        return ForecastScore(res['crps'], res['less'], res['equal'], res['energy'], res['summary'], R)

    def _run_live(self, res, steps, run):
        """res[key][live learners] = run(sub)[key] with the Philox step advanced by `steps` (restored when the library refuses
        the call); failed learners keep the fill of `res`."""
        first_step = self._rng_step
        self._rng_step += steps                      # (a diverged launch has run: its step is spent, as in train())
        live = self._healthy()
        sub = (lambda t: t) if len(live) == self.K else (lambda t: t[torch.as_tensor(live, device=self.device)].contiguous())
        try:
            if live:
                got = run(sub, first_step)
                for key, a in res.items():
                    if a is not None:
                        a[live] = got[key]
        except L.MfgError as e:
            if e.code:                               # refused by the library before anything was launched
                self._rng_step = first_step
            raise
        return res

    @_with_ctx
    def forecast_agents(self, pi0=None, indir=None, horizon=16, repeats=256, probs=FORECAST_PROBS, *, agents, want_traj=False,
                        want_counts=False):
        """forecast() with finite-population members of `agents` agents each (population.forecast_agents at the learners'
        parameters, seeds and Philox step): a Forecast with a leading K, with want_counts its counts.  Start rows, held-out rows,
        the Philox step, failed learners (NaN rows, counts -1) and errors as forecast()."""
        emp = load_empirical(indir, self.d, int(horizon)) if indir is not None else None
        ranks = forecast_ranks(probs, repeats)
        start, emp = _forecast_inputs(pi0, emp, self.d, horizon)
        agents = ops.check_forecast_agents_args(start.shape, agents, horizon, repeats, ranks, self.precision)[-1]
        apportion(start, agents)
        H, R, N, Q = int(horizon), int(repeats), start.shape[0], len(ranks)
        res = {'mean': np.full((self.K, N, H, self.d), np.nan), 'std': np.full((self.K, N, H, self.d), np.nan),
               'quant': np.full((self.K, N, H, Q, self.d), np.nan, dtype=np.float32),
               'curves': None if emp is None else np.full((self.K, H, 4), np.nan),
               'traj': np.full((self.K, N * R, H, self.d), np.nan, dtype=np.float32) if want_traj else None,
               'counts': np.full((self.K, N * R, H, self.d), -1, dtype=np.int32) if want_counts else None}
        self._run_live(res, H - 1, lambda sub, first_step: forecast_agents_policies(
            start, emp, agents, sub(self._theta), sub(self._shifts_dev), sub(self._alphas_dev), sub(self._seeds_dev), H, first_step,
            R, ranks, self.precision, self.device, self._ctx, want_traj, want_counts))
        return Forecast(res['mean'], res['std'], res['quant'], probs, ranks, res['curves'], R, res['traj'], counts=res['counts'])

    @_with_ctx
    def forecast_agents_score(self, pi0=None, indir=None, horizon=16, repeats=256, *, agents, emp=None, want_energy=True):
        """forecast_score() of forecast_agents()'s members (`agents` agents each): a ForecastScore with a leading K.  Held-out
        rows, start rows, the Philox step, failed learners and errors as forecast_score()."""
        if (indir is None) == (emp is None):
            raise ValueError('a forecast is scored against held-out rows: give indir or emp (not both)')
        if indir is not None:
            emp = load_empirical(indir, self.d, int(horizon))
        start, emp, H = _score_inputs(pi0, emp, self.d, horizon)
        agents = ops.check_forecast_agents_args(start.shape, agents, H, repeats, (), self.precision)[-1]
        apportion(start, agents)
        R, N = int(repeats), start.shape[0]
        res = {'crps': np.full((self.K, N, H, self.d), np.nan), 'less': np.full((self.K, N, H, self.d), -1, dtype=np.int32),
               'equal': np.full((self.K, N, H, self.d), -1, dtype=np.int32),
               'energy': np.full((self.K, N, H), np.nan) if want_energy else None, 'summary': np.full((self.K, H, 2), np.nan)}
        self._run_live(res, H - 1, lambda sub, first_step: forecast_agents_score_policies(
            start, emp, agents, sub(self._theta), sub(self._shifts_dev), sub(self._alphas_dev), sub(self._seeds_dev), H, first_step,
            R, self.precision, self.device, self._ctx, want_energy))
        return ForecastScore(res['crps'], res['less'], res['equal'], res['energy'], res['summary'], R)

    def learner(self, k):
        """An actor_critic holding learner k's parameters, table and Philox position (for evaluate / generate_trajectory
        / further single training).  Its construction leaves the global np.random stream as it was."""
        if not 0 <= k < self.K:
            raise IndexError('learner %d of %d' % (k, self.K))
        if self._act.state[k] == 2:
            raise L.MfgError('learner %d has failed (learner_status 0x%x): clear_status(%d) revives it'
                             % (k, int(self._act.status[k]), k))
        state = np.random.get_state()
        try:
            ac = self._new_learner(k)
        finally:
            np.random.set_state(state)
        ac.w = self.w[k]
        ac.theta = np.array([self.thetas[k]]) if self._rng_step else float(self.thetas[k])
        ac._rng_step = self._rng_step
        return ac


class ActorCriticPopulation(_Population):

    def __init__(self, thetas, shifts=0.16, alpha_scales=12000, d=21, *, batch, seeds=None, w0=None, pi0=None,
                 path_to_dir=None, update_every='step', reward='mfg_ac2', precision='mixed', episode_steps=EPISODE_STEPS,
                 device=None, verbose=0, resident=None):
        """resident (update_every='step' only): None -- the step-mode episodes take the resident kernel
        (mfg_train_episodes_pop_resident: one workgroup per learner, no launch per env step, the same bits) where
        resident_rule(K, d, batch) says it measured faster (mixed precision only: the rule was not measured in 'f64'), and
        the per-step launches otherwise and for every call under a control block; True -- always (ValueError here for a
        shape it does not serve or update_every='rollout', and from train() for a call under a control block); False --
        never."""
        th = np.asarray(thetas, dtype=np.float64).reshape(-1)
        check_args(th.shape[0], int(d), int(batch), update_every, reward, precision, int(episode_steps), resident)
        super().__init__(th, d, batch, episode_steps, shifts, alpha_scales, seeds, w0, pi0, path_to_dir, update_every,
                         precision, device, verbose)
        self.reward = reward
        self.reward_kind = REWARDS[reward]
        self.resident = resident

    @_with_ctx
    def train(self, num_episodes, gamma=1, constant=0, lr_critic=0.1, lr_actor=0.001, *, first_episode=0, stop_criteria=-1,
              isolate=False, validate=None, evolve=None):
        """`num_episodes` episodes of every learner (mfg_ac2.py:448-539; update per env step or per episode as chosen at
        construction).  lr_critic / lr_actor: scalars or [K].  Returns a NumPy array [K, num_episodes] of what
        actor_critic.train books per episode (step mode: the sum of the T updates' mean rewards; rollout mode: the one
        update's mean reward).  The Philox step counter carries over to the next call.
        stop_criteria (a scalar or [K]; negative: none): learner k stops after the first episode e with |theta_e - theta_{e-1}|
        < stop_criteria[k] (theta_0: its theta at the start of the call) and then holds exactly what the population holds
        after train(e); its row of the result is 0 beyond.  isolate=True: a learner that leaves the mixed-precision range or
        turns non-finite is frozen at the episode boundary at which that is seen (one that is out of range at the start never
        launches) instead of raising for everybody; see learner_state / episodes_run / learner_status.  The defaults issue the
        launches this method always issued.
        isolate=False under a control block -- a stop criterion is given, or a learner failed in an earlier call and was not
        cleared -- differs from the plain call in how a diverging learner is reported: it is booked to its own word and
        frozen, the context's status word stays 0, the other learners finish the call, and train() then raises MfgError
        naming the failed learners.  Later calls are not refused; they skip those learners (and raise again when
        isolate=False) until clear_status().
        validate (a Validation; None: nothing changes): every validate.period episodes the call checks every active learner on
        the held-out rows ON THE DEVICE -- the launches of evaluate() on its current theta, with score=True those of
        forecast_score() -- with no host round trip: the curve, the best iterate and (patience > 0) the stop are kept by the
        device and land on self.validation (a ValidationTrace); restore_best() puts the best iterate back.  Every check uses
        the same Philox steps (common random numbers along the curve): first_step = the counter at the call, which moves on
        by L - 1 before the first training episode.  The per-step launches run such a call (resident=True refuses it).
        evolve (an Evolution; needs validate): population-based training ON THE DEVICE -- behind every evolve.every-th check
        the worst active learners (by validate's metric) take over theta, w and the best iterate of a random one of the best
        and go on with perturbed learning rates, with no host round trip (mfg_ctx_set_pop_evolve).  The steps land on
        self.evolution (an EvolutionTrace); its lr_critic / lr_actor are the rates to pass to the next call.  A learner keeps
        its own seed, shift and alpha_scale.  ValueError without validate= or with resident=True."""
        T = self.episode_steps
        if evolve is not None and validate is None:
            raise ValueError('evolve: the exploit / explore steps follow held-out checks; give validate= too')
        if evolve is not None and self.resident is True:
            raise ValueError('resident=True: an evolved call runs the per-step launches; use resident=None or False')
        if validate is not None and self.resident is True:
            raise ValueError('resident=True: a validated call runs the per-step launches; use resident=None or False')
        resident = False
        if self.update_every == 'step':
            control = needs_control(stop_criteria_array(stop_criteria, self.K), isolate, self._act.state)
            # (the rule was measured in mixed precision; strict precision keeps the per-step launches unless forced)
            rule = self.precision == 'mixed' and resident_rule(self.K, self.d, self.batch)
            resident = validate is None and use_resident(self.resident, rule, control)
        step_call = ops.train_episodes_pop_resident if resident else ops.train_episodes_pop

        def run(b, lrc, lra, acc):
            if self.update_every == 'step':
                step_call(self._mat_pi0_dev, b['pi'], T, int(num_episodes), first_episode, constant == 1, self._theta,
                          self._shifts_dev, self._alphas_dev, self._w, gamma, lrc, lra, self._seeds_dev, b['G'], b['ws'],
                          b['run'], reward_kind=self.reward_kind, first_step=self._rng_step, reward_acc=acc,
                          precision=self.precision)
            else:
                ops.train_rollouts_pop(self._mat_pi0_dev, T, int(num_episodes), first_episode, constant == 1, self._theta,
                                       self._shifts_dev, self._alphas_dev, self._w, gamma, b['G'], b['ws'], b['run'], lrc, lra,
                                       self._seeds_dev, reward_kind=self.reward_kind, first_step=self._rng_step,
                                       reward_acc=acc, precision=self.precision)
        return self._train(num_episodes, lr_critic, lr_actor, run, stop_criteria, isolate, validate, evolve)

    @_with_ctx
    def evaluate(self, episode_length=16, indir='test_normalized_round2', outfile='eval_mfg_round2/test_eval_fixed_reward.csv',
                 write_header=0, *, repeats=1):
        """actor_critic.evaluate (mfg_ac2.py:595-670) for every learner's current policy in one evaluate_pop call: the test files
        are read once, learner k rolls with its own seed from the population's Philox step, and K CSV lines are appended in
        learner order.  Returns a NumPy [K, 4] array (mean l1_final, l1_mean, JSD_final, JSD_mean per learner) and advances the
        Philox step by episode_length - 1, as each learner's own evaluate() would.  With repeats=1 learner k gets what
        learner(k).evaluate(thetas[k], shifts[k], alpha_scales[k], d, episode_length, ...) gives; repeats = R rolls R
        trajectories per test file.  MfgError (and no CSV line) when a mixed-precision policy left the fp32 range."""
        return self._evaluate(episode_length, indir, outfile, write_header, repeats)

    @_with_ctx
    def _evaluate_synthetic(self, day_first, day_last, repeats, column):
        """The body of evaluate_synthetic (column 0: l1) / evaluate_synthetic_JSD (column 2: jsd)."""
        start = self.mat_pi0[day_first - 1:day_last]
        first_step = self._rng_step
        self._rng_step += SYNTHETIC_HOURS - 1        # (a diverged launch has run: its step is spent, as in train())
        live = self._healthy()                       # failed learners are not launched: NaN
        sub = (lambda t: t) if len(live) == self.K else (lambda t: t[torch.as_tensor(live, device=self.device)].contiguous())
        table = np.full((self.K, 4), np.nan)
        try:
            if live:
                table[live] = consistency_policies(start, sub(self._theta), sub(self._shifts_dev), sub(self._alphas_dev),
                                                   sub(self._seeds_dev), SYNTHETIC_HOURS, first_step, repeats, self.precision,
                                                   self.device, self._ctx)[0]
        except L.MfgError as e:
            if e.code:                               # refused by the library before anything was launched
                self._rng_step = first_step
            raise
        return table[:, column].copy(), table[:, column + 1].copy()

    def evaluate_synthetic(self, day_first=1, day_last=26, *, repeats=1):
        """mfg_synthetic.actor_critic.evaluate_synthetic (mfg_synthetic.py:741-812) for every learner's current policy in one
        consistency_pop call: (mean [K], std [K]) over (start row, hour) of sum_ij |P_ij - value_ij|.  Start rows
        mat_pi0[day_first-1:day_last]; learner k rolls with its own seed from the population's Philox step, which advances by
        15 as each learner's own call would (restored when the library refuses the call).  With repeats=1 learner k gets what
        learner(k).evaluate_synthetic(day_first, day_last) gives up to the summation order; repeats = R rolls R trajectories
        per start row.  Failed learners are not launched: NaN.  ValueError for a population whose reward is not 'synthetic' or
        days outside the table; MfgError when a mixed-precision policy left the fp32 range."""
        day_first, day_last, repeats = check_synthetic_eval(self.reward, self.mat_pi0.shape[0], day_first, day_last, repeats)
        return self._evaluate_synthetic(day_first, day_last, repeats, 0)

    def evaluate_synthetic_JSD(self, day_first=1, day_last=26, *, repeats=1):
        """evaluate_synthetic with the reference's second metric (mfg_synthetic.py:815-899): (mean [K], std [K]) over (start
        row, hour) of sum_i JSD(P_i, value-implied row i)."""
        day_first, day_last, repeats = check_synthetic_eval(self.reward, self.mat_pi0.shape[0], day_first, day_last, repeats)
        return self._evaluate_synthetic(day_first, day_last, repeats, 2)

    def _new_learner(self, k):
        return actor_critic(float(self.thetas[k]), float(self.shifts[k]), float(self.alpha_scales[k]), self.d,
                            pi0=self.mat_pi0, batch=self.batch, seed=int(self.seeds[k]), update_every=self.update_every,
                            reward=self.reward, precision=self.precision, device=self.device, verbose=self.verbose,
                            episode_steps=self.episode_steps)
