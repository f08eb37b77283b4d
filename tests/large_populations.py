"""Large populations: the call table and the procedures of tests/test_gpu_large_populations.py.

include/mfg_hip.h admits 1 <= K <= MFG_POP_MAX_K = 65535 learners in every population entry point and promises, in several
places, that learner k's outputs are bit for bit what it gives alone or among others.  That promise is the oracle here.

  P = 7 parameter SETS (coprime to the 64 lanes of a wave and to the 256 keys of a rank tile).  A set holds everything a
  learner owns.  A row's builder is written once in K: given a Cycled it declares the shared inputs, the per-learner inputs
  (data of shape [P, ...]; learner k gets the data of set k mod P, seeds included), the in/out buffers, the outputs and the
  workspaces, and returns a closure that issues the call.

  small(row)        the call with K = P, set p in position p (computed once per row, shared, left unchanged), after
                    assert_distinct: the P sets give pairwise different results, so a rebase that collapses learners
                    cannot pass.
  run(row, K)       the big call.  Outputs are NaN / negative before the call; outputs, in/out buffers and workspaces are
                    guard_bands.Guarded of exactly the advertised size (learner K - 1 ends at the last byte), and the
                    bands are checked.
  assert_cycled     slice k of the big result == slice k mod P of the small one, bit for bit, for all k: the first
                    P (K // P) slices viewed as [K // P, P, ...] against the broadcast small result, then the remainder.
                    Floats are compared as integers, so NaN equals NaN of the same bits.
  alone(row)        set s as the only learner of a call (K = 1) against slice s of the small call.
  evolved(K, ..)    procedure E: mfg_train_episodes_pop under a control, a validation and an evolve block, whose learners
                    interact (ranks depend on everyone, the draw is keyed by k): against the small call without the evolve
                    block followed by tests/pop_evolve_ref.step on the device's own check values.

No row hands a call a K outside the header's range or a buffer smaller than its query returns: nothing here can fault.
"""
import ctypes as C

import numpy as np
import torch

import guard_bands
import stream_order as S
from stream_order import F32, F64, I32, I64, U8, NAN, GAMMA, NUM_START, call, p

P = 7
# functions of the header with a parameter K (or a struct with a member K) that have no row, and why.
EXEMPT = {}


def _ops():
    from discrete_mean_field_game_amd import ops
    return ops


def _L():
    from discrete_mean_field_game_amd import _lib
    return _lib


# ---------------------------------------------------------------------------------------------------
# the comparison (works on CPU tensors as well: tests/test_large_populations_host.py)
# ---------------------------------------------------------------------------------------------------
def _bits(t):
    t = t.contiguous()
    if t.dtype.is_floating_point:
        return t.view(I32 if t.element_size() == 4 else I64)
    return t


def differing_learners(big, small, limit=8):
    """The learners k (ascending, at most `limit`) whose slice big[k] differs in any bit from small[k mod P]."""
    n_sets = small.shape[0]
    K = big.shape[0]
    assert big.shape[1:] == small.shape[1:] and big.dtype == small.dtype, (big.shape, small.shape, big.dtype, small.dtype)
    b, s = _bits(big).reshape(K, -1), _bits(small).reshape(n_sets, -1)
    whole = K // n_sets
    bad = []
    if whole:
        head = b[:whole * n_sets].view(whole, n_sets, -1)
        ne = (head != s.unsqueeze(0)).any(-1).reshape(-1)
        bad += ne.nonzero().reshape(-1)[:limit].tolist()
    rest = K - whole * n_sets
    if rest and len(bad) < limit:
        ne = (b[whole * n_sets:] != s[:rest]).any(-1)
        bad += (ne.nonzero().reshape(-1)[:limit] + whole * n_sets).tolist()
    return bad[:limit]


def assert_cycled(name, big, small):
    bad = differing_learners(big, small)
    if bad:
        k = bad[0]
        raise AssertionError('%s: learner %d (set %d) of %d differs from the small call; first differing learners %s'
                             % (name, k, k % small.shape[0], big.shape[0], bad))


def coinciding_sets(small):
    """Pairs (p, q), p < q, of sets whose slices agree bit for bit in EVERY buffer of `small` (name -> tensor [P, ...])."""
    n_sets = next(iter(small.values())).shape[0]
    same = torch.ones(n_sets, n_sets, dtype=torch.bool)
    for t in small.values():
        b = _bits(t).reshape(n_sets, -1)
        same &= (b.unsqueeze(0) == b.unsqueeze(1)).all(-1).cpu()
    return [(i, j) for i in range(n_sets) for j in range(i + 1, n_sets) if bool(same[i, j])]


def assert_distinct(name, small):
    pairs = coinciding_sets(small)
    if pairs:
        raise AssertionError('%s: the sets %s give the same bits in every output: the row cannot see learners collapse'
                             % (name, pairs))


# ---------------------------------------------------------------------------------------------------
# the buffers of one call
# ---------------------------------------------------------------------------------------------------
class Cycled:
    """The buffers of one call of K learners, learner k holding set k mod P.  guarded: outputs, in/out buffers and
    workspaces are Guarded (the big call)."""

    def __init__(self, dev, K, guarded, first=0):
        self.dev, self.K, self.guarded, self.first = dev, int(K), guarded, int(first)
        self.g = S.Bufs(dev, 0)                 # the seeded generators of valid data
        self.set_ids = (np.arange(self.K) + self.first) % P        # learner k holds set (first + k) mod P (first != 0: alone())
        self.idx = torch.as_tensor(self.set_ids, device=dev)
        self.cmp = {}                           # name -> (tensor, learner axis)
        self.bands = []                         # (name, Guarded)
        self.keep = []
        self.inputs = {}                        # inputs by name, for the tests that hold the small call against a restatement

    def sets(self, data):
        """A per-learner input from the data of the P sets [P, ...]: [K, ...]."""
        assert data.shape[0] == P, data.shape
        return data.to(self.dev).index_select(0, self.idx).contiguous()

    def host_sets(self, values):
        """K host values from the P of the sets."""
        assert len(values) == P
        return [values[s] for s in self.set_ids]

    def _alloc(self, name, shape, dtype, fill):
        if not self.guarded:
            if isinstance(fill, torch.Tensor):
                return fill.clone()
            return torch.full(shape, fill, dtype=dtype, device=self.dev)
        g = guard_bands.Guarded(shape, dtype, self.dev, fill=fill)
        self.bands.append((name, g))
        return g.t

    def io(self, name, data, axis=0):
        t = self.sets(data)
        t = self._alloc(name, tuple(t.shape), t.dtype, t)
        self.cmp[name] = (t, axis)
        return t

    def out(self, name, shape, dtype=F32, axis=0):
        """An output of per-learner shape `shape`: [K, *shape] (axis = 1: [shape[0], K, *shape[1:]])."""
        full = (self.K,) + tuple(shape) if axis == 0 else (shape[0], self.K) + tuple(shape[1:])
        t = self._alloc(name, full, dtype, NAN if dtype.is_floating_point else -7)
        self.cmp[name] = (t, axis)
        return t

    def ws(self, nbytes, dtype=U8, shape=None):
        item = torch.empty(0, dtype=dtype).element_size()
        assert nbytes % item == 0, (nbytes, item)
        t = self._alloc('workspace %d' % len(self.bands), (nbytes // item,), dtype, 0)
        return t if shape is None else t.view(shape)

    def policies(self):
        th = torch.tensor(np.linspace(6.5, 9.5, P), dtype=F64)
        sh = torch.tensor(np.linspace(0.1, 0.3, P), dtype=F64)
        al = torch.tensor(np.linspace(9000.0, 13000.0, P), dtype=F64)
        sd = torch.arange(P, dtype=I64) * 7919 + (1 << 33)
        return self.sets(th), self.sets(sh), self.sets(al), self.sets(sd)

    def compared(self):
        return {n: (t if ax == 0 else t.movedim(ax, 0)) for n, (t, ax) in self.cmp.items()}

    def check_bands(self):
        for name, g in self.bands:
            g.check(name)


class Row:
    def __init__(self, name, entries, build):
        self.name, self.entries, self.build = name, tuple(entries), build

    def __repr__(self):
        return self.name


ROWS = []


def row(name, *entries):
    def deco(build):
        ROWS.append(Row(name, entries, build))
        return build
    return deco


def covered_entries():
    return sorted({e for r in ROWS for e in r.entries} | set(PROCEDURE_E_ENTRIES))


# Procedure E (the calls whose learners interact) binds these three blocks to mfg_train_episodes_pop.
PROCEDURE_E_ENTRIES = ('mfg_ctx_set_pop_control', 'mfg_ctx_set_pop_validate', 'mfg_ctx_set_pop_evolve',
                       'mfg_pop_validate_workspace_bytes')


# ---------------------------------------------------------------------------------------------------
# training: mfg_train_episodes_pop, its resident form, mfg_train_rollouts_pop
# ---------------------------------------------------------------------------------------------------
B, T, E = 13, 2, 2


def _pop_common(a, d, seed, episodes=E, theta=None, mat=None):
    K = a.K
    F = _ops().num_features(d)
    sb = _ops().pop_workspace_slice(B, d, T)
    mat = a.g.simplex((NUM_START, d), seed) if mat is None else mat
    sh, al, sd = a.policies()[1:]
    th = a.io('theta', torch.tensor(np.linspace(6.5, 9.5, P) if theta is None else theta, dtype=F64))
    w = a.io('w', a.g.randn64((P, F), d).abs_() * 0.1)
    G = a.out('G', (F + 3,), F64)
    acc = a.io('reward_acc', torch.zeros(P, episodes, dtype=F64))
    lrc = a.sets(torch.tensor(np.linspace(0.05, 0.15, P), dtype=F64))
    lra = a.sets(torch.tensor(np.linspace(5e-4, 2e-3, P), dtype=F64))
    ws = a.ws(K * sb, F64, (K, sb // 8))
    a.keep += [mat, sh, al, sd, lrc, lra]
    a.inputs.update(mat_pi0=mat, shifts=sh, alphas=al, seeds=sd, lr_critic=lrc, lr_actor=lra)
    return mat, th, sh, al, sd, w, G, acc, lrc, lra, ws, sb


def _episode_bufs(a, d):
    return (a.ws(a.K * B * d * 4, F32), a.out('reward', (B,)), a.out('delta', (B,), F64), a.out('g', (B,), F64))


def _rollout_outs(a, d):
    return (a.out('pi_traj', (B, T + 1, d)), a.out('pi_last', (B, d)), a.out('reward', (B, T)), a.out('delta', (B, T), F64),
            a.out('g', (B, T), F64))


def _pop_step(entry, d):
    @row('%s-d%d' % (entry[4:], d), entry, 'mfg_workspace_bytes')
    def build(a):
        L = _L()
        if entry.endswith('_resident'):
            assert L.lib().mfg_pop_resident_supported(d, B, L.REWARD_MFG_AC2) == 1
        mat, th, sh, al, sd, w, G, acc, lrc, lra, ws, sb = _pop_common(a, d, 29)
        pi = a.out('pi_io', (B, d))
        scratch, r, delta, g = _episode_bufs(a, d)
        args = (p(mat), NUM_START, p(pi), p(scratch), B, a.K, d, T, E, 0, 0, p(th), p(sh), p(al), p(w), GAMMA, L.REWARD_MFG_AC2,
                p(sd), 3, 100, L.PRECISION_MIXED, p(lrc), p(lra), p(r), p(delta), p(g), p(G), p(acc), p(ws), sb)
        return lambda: call(entry, *args)


_pop_step('mfg_train_episodes_pop', 21)
_pop_step('mfg_train_episodes_pop', 5)
_pop_step('mfg_train_episodes_pop_resident', 21)


def _pop_rollouts(d):
    @row('train_rollouts_pop-d%d' % d, 'mfg_train_rollouts_pop')
    def build(a):
        L = _L()
        mat, th, sh, al, sd, w, G, acc, lrc, lra, ws, sb = _pop_common(a, d, 30)
        traj, last, r, delta, g = _rollout_outs(a, d)
        return lambda: call('mfg_train_rollouts_pop', p(mat), NUM_START, B, a.K, d, T, E, 0, 0, p(th), p(sh), p(al), p(w), GAMMA,
                            L.REWARD_MFG_AC2, p(sd), 3, 100, 0, p(lrc), p(lra), p(traj), p(last), p(r), p(delta), p(g), p(G),
                            p(acc), p(ws), sb)


_pop_rollouts(21)
_pop_rollouts(5)

# ---------------------------------------------------------------------------------------------------
# evaluation, forecasts, scores, finite populations, consistency, means
# ---------------------------------------------------------------------------------------------------
N, H, R = 2, 3, 2          # files / start rows, rows per file / hours, repeats: k N R is not k N


def _evaluate_pop(d):
    @row('evaluate_pop-d%d' % d, 'mfg_evaluate_pop', 'mfg_evaluate_pop_workspace_bytes')
    def build(a):
        emp = a.g.simplex((N, H, d), 48)
        e32, e64 = emp, emp.double()
        th, sh, al, sd = a.policies()
        metrics = a.out('metrics', (8,), F64)
        n = int(_L().lib().mfg_evaluate_pop_workspace_bytes(N, H, d, a.K, R, 0))
        ws = a.ws(n)
        a.keep += [e32, e64, th, sh, al, sd]
        a.inputs.update(emp32=e32, emp64=e64, policies=torch.stack([th, sh, al]), seeds=sd)
        return lambda: call('mfg_evaluate_pop', p(e32), p(e64), N, H, d, a.K, p(th), p(sh), p(al), p(sd), 37, R,
                            _L().PRECISION_MIXED, p(metrics), None, p(ws), n)


_evaluate_pop(21)
_evaluate_pop(5)


RANKS = (0, R - 1, R // 2, 1, 1)          # unsorted, with a repeat: the ranks of tests/test_gpu_forecast_pop.py


def _ranks(a):
    arr = (C.c_int32 * len(RANKS))(*RANKS)
    a.keep.append(arr)
    return arr


@row('forecast_pop', 'mfg_forecast_pop', 'mfg_forecast_pop_workspace_bytes')
def _forecast_pop(a):
    d = 21
    emp = a.g.simplex((N, H, d), 49)
    s32, e32, e64 = emp[:, 0].contiguous(), emp, emp.double()
    th, sh, al, sd = a.policies()
    ranks = _ranks(a)
    mean, std = a.out('mean', (N, H, d), F64), a.out('std', (N, H, d), F64)
    quant, curves = a.out('quant', (N, H, len(RANKS), d)), a.out('curves', (H, 4), F64)
    n = int(_L().lib().mfg_forecast_pop_workspace_bytes(N, H, d, a.K, R, 0))
    ws = a.ws(n)
    a.keep += [s32, e32, e64, th, sh, al, sd]
    a.inputs.update(start32=s32, emp32=e32, emp64=e64, policies=torch.stack([th, sh, al]), seeds=sd)
    return lambda: call('mfg_forecast_pop', p(s32), N, H, d, a.K, p(th), p(sh), p(al), p(sd), 37, R, _L().PRECISION_MIXED, ranks,
                        len(RANKS), p(e32), p(e64), p(mean), p(std), p(quant), p(curves), None, p(ws), n)


@row('forecast_score', 'mfg_forecast_score', 'mfg_forecast_score_workspace_bytes')
def _forecast_score(a):
    d = 21
    emp = a.g.simplex((N, H, d), 50)
    traj, e32, e64 = a.sets(a.g.simplex((P, N * R, H, d), 51)), emp, emp.double()
    crps, less, equal = a.out('crps', (N, H, d), F64), a.out('less', (N, H, d), I32), a.out('equal', (N, H, d), I32)
    en, summary = a.out('energy', (N, H), F64), a.out('summary', (H, 2), F64)
    n = int(_L().lib().mfg_forecast_score_workspace_bytes(N, H, d, a.K, R))
    ws = a.ws(n)
    a.keep += [traj, e32, e64]
    a.inputs.update(traj=traj, emp32=e32, emp64=e64)
    return lambda: call('mfg_forecast_score', p(traj), N, H, d, a.K, R, p(e32), p(e64), p(crps), p(less), p(equal), p(en),
                        p(summary), p(ws), n)


AGENTS = 257


def _counts(pi):
    """Rows of int32 counts that sum to AGENTS, apportioned from simplex rows."""
    c = torch.floor(pi.double() * AGENTS).to(I32)
    c[..., 0] += AGENTS - c.sum(-1).to(I32)
    return c


@row('agents_step_pop', 'mfg_agents_step_pop')
def _agents_step(a):
    d = 21
    counts, Pm = a.sets(_counts(a.g.simplex((P, B, d), 52))), a.sets(a.g.simplex((P, B, d, d), 53))
    sd = a.policies()[3]
    cn, pn, mv = a.out('counts_next', (B, d), I32), a.out('pi_next', (B, d)), a.out('moves', (B, d, d), I32)
    a.keep += [counts, Pm, sd]
    a.inputs.update(counts=counts, P=Pm, seeds=sd)
    return lambda: call('mfg_agents_step_pop', p(counts), p(Pm), B, d, a.K, AGENTS, p(sd), 5, 1000, p(cn), p(pn), p(mv))


@row('forecast_agents_pop', 'mfg_forecast_agents_pop', 'mfg_forecast_agents_pop_workspace_bytes')
def _forecast_agents(a):
    d = 21
    emp = a.g.simplex((N, H, d), 54)
    c0, e32, e64 = _counts(emp[:, 0]).contiguous(), emp, emp.double()
    th, sh, al, sd = a.policies()
    ranks = _ranks(a)
    mean, std = a.out('mean', (N, H, d), F64), a.out('std', (N, H, d), F64)
    quant, curves = a.out('quant', (N, H, len(RANKS), d)), a.out('curves', (H, 4), F64)
    ct, act = a.out('counts_traj', (N * R, H, d), I32), a.out('actions', (N * R, H - 1, d, d))
    n = int(_L().lib().mfg_forecast_agents_pop_workspace_bytes(N, H, d, a.K, R, 0, 1))
    ws = a.ws(n)
    a.keep += [c0, e32, e64, th, sh, al, sd]
    a.inputs.update(counts0=c0, emp32=e32, emp64=e64, policies=torch.stack([th, sh, al]), seeds=sd)
    return lambda: call('mfg_forecast_agents_pop', p(c0), N, H, d, a.K, AGENTS, p(th), p(sh), p(al), p(sd), 37, R,
                        _L().PRECISION_MIXED, ranks, len(RANKS), p(e32), p(e64), p(mean), p(std), p(quant), p(curves), None, p(ct), p(act),
                        p(ws), n)


@row('action_mean_pop', 'mfg_action_mean_pop', 'mfg_action_mean_pop_workspace_bytes')
def _action_mean(a):
    d, n_act = 21, 13
    act, mean = a.sets(a.g.simplex((P, n_act, d, d), 58)), a.out('mean', (d, d), F64)
    n = int(_L().lib().mfg_action_mean_pop_workspace_bytes(a.K, n_act, d))
    ws = a.ws(n)
    a.keep.append(act)
    a.inputs.update(action=act)
    return lambda: call('mfg_action_mean_pop', p(act), n_act * d * d, a.K, n_act, d, p(mean), p(ws), n)


@row('consistency_given', 'mfg_consistency_given', 'mfg_consistency_given_workspace_bytes')
def _consistency_given(a):
    """Without `steps` the per-hour values live in the workspace, which the second launch reads."""
    M, d = 2, 21
    Pm, metrics = a.sets(a.g.simplex((P, M, T, d, d), 55)), a.out('metrics', (4,), F64)
    n = int(_L().lib().mfg_consistency_given_workspace_bytes(a.K, M, T, 0))
    ws = a.ws(n)
    a.keep.append(Pm)
    a.inputs.update(P=Pm)
    return lambda: call('mfg_consistency_given', p(Pm), a.K, M, T, d, p(metrics), None, None, p(ws), n)


@row('consistency_pop', 'mfg_consistency_pop', 'mfg_consistency_pop_workspace_bytes')
def _consistency_pop(a):
    d = 21
    s32 = a.g.simplex((N, d), 56)
    th, sh, al, sd = a.policies()
    metrics, steps = a.out('metrics', (4,), F64), a.out('steps', (N * R, H - 1, 2), F64)
    n = int(_L().lib().mfg_consistency_pop_workspace_bytes(N, H, d, a.K, R, 1, 0, 0))
    ws = a.ws(n)
    a.keep += [s32, th, sh, al, sd]
    a.inputs.update(start32=s32, policies=torch.stack([th, sh, al]), seeds=sd)
    return lambda: call('mfg_consistency_pop', p(s32), N, H, d, a.K, p(th), p(sh), p(al), p(sd), 37, R, _L().PRECISION_MIXED,
                        p(metrics), p(steps), None, None, None, p(ws), n)


@row('row_distribution', 'mfg_row_distribution', 'mfg_row_distribution_workspace_bytes')
def _row_distribution(a):
    """R rows in the place of K learners ("the same bits whatever R is")."""
    n_val, bins, grid = 257, 16, 20
    stride = n_val + 3
    v = a.sets(a.g.randn64((P, stride), 57).float())
    moments, counts = a.out('moments', (6,), F64), a.out('counts', (bins,), I64)
    edges, status, density = a.out('edges', (bins + 1,), F64), a.out('status', (), I32), a.out('density', (grid,), F64)
    n = int(_L().lib().mfg_row_distribution_workspace_bytes(a.K, n_val, bins, grid))
    ws = a.ws(n) if n else None
    a.keep.append(v)
    a.inputs.update(values=v)
    return lambda: call('mfg_row_distribution', p(v), a.K, n_val, stride, bins, 0, 0.0, 0.0, grid, -3.0, 3.0, p(moments),
                        p(counts), p(edges), p(density), p(status), p(ws), n)


# ---------------------------------------------------------------------------------------------------
# the reward network and the IRL drivers
# ---------------------------------------------------------------------------------------------------
N3, N4 = 8, 4


def _net(a, d, per_learner, nets=None, keep_prob=0.8):
    """mfg_reward_net_t: P networks stacked learner-major (learner k the network of set k mod P), or one shared network.
    nets: the networks.RewardNet modules to take the weights from (default: oracle.reward_train_cases._net, seeds 7 ..)."""
    from oracle.reward_train_cases import _net as make
    if nets is None:
        nets = [make(d, 'dropout_l1l2', N3, N4, a.dev, seed=7 + s) for s in range(P if per_learner else 1)]
    nets = nets[:P if per_learner else 1]
    st = _L().RewardNetStruct()
    st.k1, st.f2, st.k2, st.n3, st.n4, st.keep_prob = 5, 2, 3, N3, N4, keep_prob
    for name, get in (('conv1_w', lambda n: n.conv1.weight), ('conv1_b', lambda n: n.conv1.bias), ('conv2_w', lambda n: n.conv2.weight),
                      ('conv2_b', lambda n: n.conv2.bias), ('fc3_w', lambda n: n.fc3.weight), ('fc3_b', lambda n: n.fc3.bias),
                      ('fc4_w', lambda n: n.fc4.weight), ('fc4_b', lambda n: n.fc4.bias), ('out_w', lambda n: n.out.weight),
                      ('out_b', lambda n: n.out.bias)):
        if per_learner:
            t = a.sets(torch.stack([get(n).detach().reshape(-1) for n in nets]))
        else:
            t = get(nets[0]).detach().reshape(-1).clone().contiguous().to(a.dev)
        a.keep.append(t)
        a.inputs['net_' + name] = t
        setattr(st, name, t.data_ptr())
    a.keep.append(st)
    return st


IRL_KEEP, IRL_RN_SEED = 0.8, 0x5EED        # the dropout keep probability; rn_seed = seed + IRL_RN_SEED, as AC_IRL keys its reward calls
_IRL_NETS = []


def irl_nets():
    """The P reward networks of the IRL rows (CPU modules, made once): those of tests/test_gpu_irl_population.py's _nets, whose
    _single then runs a set through the single-learner IRL calls."""
    if not _IRL_NETS:
        from discrete_mean_field_game_amd.networks import RewardNet
        for s in range(P):
            torch.manual_seed(40 + s)
            net = RewardNet(d=21, n_fc3=N3, n_fc4=N4, keep_prob=IRL_KEEP)
            with torch.no_grad():          # non-zero biases: every tensor of the network matters
                for q in net.parameters():
                    if q.dim() == 1:
                        q.uniform_(-0.2, 0.2)
            _IRL_NETS.append(net)
        st = _ops().reward_net_struct(_IRL_NETS[0])
        assert (st.k1, st.f2, st.k2, st.n3, st.n4) == (5, 2, 3, N3, N4) and abs(st.keep_prob - IRL_KEEP) < 1e-7
    return _IRL_NETS


def irl_table(d):
    """The start table of tests/test_gpu_irl_population.py (_table), fp32."""
    return torch.as_tensor(np.ascontiguousarray(np.random.RandomState(3).dirichlet(np.ones(d), size=9), dtype=np.float32))


def _irl_pop(step, per_learner):
    entry = 'mfg_train_episodes_irl_pop' if step else 'mfg_train_rollouts_irl_pop'

    @row('%s-%s' % (entry[4:], 'nets' if per_learner else 'shared_net'), entry)
    def build(a):
        L = _L()
        d = 21
        # first episode 1, Philox step 0, trajectory offset 0, no reward call made before, rn_seed = seed + IRL_RN_SEED: the call
        # as AC_IRLPopulation issues its first one, which tests/test_gpu_irl_population.py's _single restates per learner
        st = _net(a, d, per_learner, irl_nets(), IRL_KEEP)
        mat, th, sh, al, sd, w, G, acc, lrc, lra, ws, sb = _pop_common(a, d, 35, mat=irl_table(d).to(a.dev))
        NUM_START = int(mat.shape[0])
        rn_seed = sd + IRL_RN_SEED
        rn_call0 = torch.zeros(a.K, dtype=I64, device=a.dev)
        a.keep += [rn_seed, rn_call0]
        head = (p(th), p(sh), p(al), p(w), GAMMA, p(sd), 0, 0)
        net = (p(lrc), p(lra), C.byref(st), int(per_learner), 0, None, None, p(rn_seed), p(rn_call0))
        if step:
            pi, Pm = a.out('pi_out', (B, d)), a.out('P', (B, d, d))
            scratch, r, delta, g = _episode_bufs(a, d)
            return lambda: call(entry, p(mat), NUM_START, p(pi), p(scratch), B, a.K, d, T, E, 1, 0, *head, L.PRECISION_MIXED, *net,
                                p(Pm), p(r), p(delta), p(g), p(G), p(acc), p(ws), sb)
        traj, last, r, delta, g = _rollout_outs(a, d)
        Pm = a.out('P', (B, T, d, d))
        return lambda: call(entry, p(mat), NUM_START, B, a.K, d, T, E, 1, 0, *head, L.ROLLOUT_DISCOUNT_POW, *net, p(traj), p(last),
                            p(Pm), p(r), p(delta), p(g), p(G), p(acc), p(ws), sb)


_irl_pop(True, True)
_irl_pop(True, False)
_irl_pop(False, True)
_irl_pop(False, False)

RN_N = 5         # samples per learner of the forward rows


def _keys(a):
    return a.host_sets(grad_keys())


@row('reward_net_forward_pop', 'mfg_reward_net_forward_pop')
def _forward_pop(a):
    """Every learner listed, in descending order: slot s is learner K - 1 - s."""
    d = 21
    st = _net(a, d, True)
    s, act = a.sets(a.g.simplex((P, RN_N, d), 73)), a.sets(a.g.simplex((P, RN_N, d, d), 74))
    out, scratch = a.out('reward', (RN_N,)), a.ws(16 * a.K)
    learners, keys = list(range(a.K))[::-1], _keys(a)[::-1]
    a.inputs.update(state=s, action=act, keys=torch.tensor([k_ for k_ in keys[::-1]], dtype=I64))
    return lambda: _ops().reward_net_forward_pop(st, True, a.K, s, act, learners, keys, out=out, scratch=scratch)


GRAD_NET_SEEDS, GRAD_INPUT_SEED = (201, 202, 205, 204, 203, 206, 207), 11
GRAD_KEEP = 0.8
_GRAD_CASE = []


def grad_keys():
    return [77 + 1000003 * s + ((s % 2) << 40) for s in range(P)]


def grad_case():
    """(P networks on the CPU in eval mode, state [P, RN_N, d], action [P, RN_N, d, d] fp32) of the input-gradient row."""
    if not _GRAD_CASE:
        import reward_grad_ref as G
        nets = [G.make_net(21, 'dropout_l1l2', N3, N4, seed) for seed in GRAD_NET_SEEDS]
        for n in nets:
            n.keep_prob = GRAD_KEEP
        _GRAD_CASE.extend([nets, *G.make_inputs(21, RN_N, 7919 * 21 + GRAD_INPUT_SEED, P)])
    return tuple(_GRAD_CASE)


@row('rn_input_grad', 'mfg_ctx_set_rn_input_grad', 'mfg_rn_input_grad_workspace_bytes', 'mfg_reward_net_forward_pop')
def _input_grad(a):
    """The networks and inputs come from tests/reward_grad_ref.py (make_net, make_inputs), so that its restatement applies;
    tests/test_large_populations_host.py admits them as tests/test_reward_grad_host.py admits that module's own cases."""
    d = 21
    nets, state, action = grad_case()
    st = _net(a, d, True, nets, GRAD_KEEP)
    s, act = a.sets(torch.as_tensor(state)), a.sets(torch.as_tensor(action))
    out, scratch = a.out('reward', (RN_N,)), a.ws(16 * a.K)
    bufs = dict(grad_state=a.out('grad_state', (RN_N, d)), grad_action=a.out('grad_action', (RN_N, d, d)),
                mean_state=a.out('mean_state', (2, d), F64), mean_action=a.out('mean_action', (2, d, d), F64))
    n = _ops().rn_input_grad_workspace_bytes(a.K, RN_N, d)
    assert n > 0 and n % 8 == 0, n                       # (exactly the advertised bytes behind an fp64 view)
    ws = a.ws(n, F64)
    learners, keys = list(range(a.K)), _keys(a)
    return lambda: _ops().reward_input_grad_pop(st, True, a.K, s, act, learners, keys, out=out, scratch=scratch,
                                                want=tuple(bufs), bufs=bufs, workspace=ws, workspace_bytes=n)


RN = dict(d=15, rows=3, T=2, nd=2, ng=2, U=2)      # d = 15: three [K, NP] fp32 arrays of d = 21 would not leave room at 65 535


def _rn_dims():
    return (RN['d'], 5, 2, 3, N3, N4)


def _train_steps_pop(z):
    entry = 'mfg_reward_net_train_steps_pop' + ('_z' if z else '')

    @row(entry[4:], entry)
    def build(a):
        ops, K = _ops(), a.K
        d, rows, Tn, nd, ng, U = (RN[k] for k in ('d', 'rows', 'T', 'nd', 'ng', 'U'))
        NP = int(_L().lib().mfg_reward_net_num_params(*_rn_dims()))
        ld = (NP + 63) // 64 * 64
        prm = a.io('params', (a.g.rand32((P, ld), 36) - 0.5) * 0.4)
        m, v = a.io('adam_m', (a.g.rand32((P, ld), 37) - 0.5) * 1e-3), a.io('adam_v', a.g.rand32((P, ld), 38) * 1e-6)
        demo = (a.g.simplex((rows, Tn, d), 39), a.g.simplex((rows, Tn, d, d), 40))
        gen = (a.sets(a.g.simplex((P, rows, Tn, d), 41)), a.sets(a.g.simplex((P, rows, Tn, d, d), 42)))
        stats = a.out('stats', (4,))
        sl = (int(_L().lib().mfg_reward_net_train_workspace_bytes(*_rn_dims(), (nd + ng) * Tn)) + 255) // 256 * 256
        plan = ops.rn_train_plan(U * K)
        k = np.arange(K)
        for u in range(U):
            e = plan[u * K:(u + 1) * K]
            order = k[::-1] if u else k                       # the second update lists the learners in descending order
            so = a.set_ids[order]
            e['learner'], e['key'], e['lr'], e['adam_step'] = order, 1000 * u + so + (1 << 35), 2e-3 * (1 + so), u + 1
            for j in range(nd):
                e['demo_rows'][:, j] = (j + u + so) % rows
            for j in range(ng):
                e['gen_rows'][:, j] = (rows - 1 - j - u - so) % rows
        ws, plan_dev = a.ws(K * sl), a.ws(plan.nbytes)
        logz = a.sets(a.g.randn64((P, rows), 75)) if z else None
        a.keep += [demo, gen, logz, plan]
        a.plan = plan
        a.inputs.update(demo_state=demo[0], demo_action=demo[1], gen_state=gen[0], gen_action=gen[1], **({'gen_log_z': logz} if z else {}))
        return lambda: ops.reward_net_train_steps_pop(prm, m, v, ld, K, _rn_dims(), demo, gen, plan, U, K, nd, ng, Tn, 5, 0.8, True,
                                                      stats, ws, plan_dev, gen_log_z=logz)


_train_steps_pop(False)
_train_steps_pop(True)


LOGPDF = (0.05, 50.0, 0.0, 1e-6)          # shift, alpha_scale, alpha_floor, p_floor: a setting of tests/test_gpu_launch_once_kernels.py


@row('policy_logpdf', 'mfg_policy_logpdf')
def _policy_logpdf(a):
    """K thetas; out [N, K]: the learner is the inner index."""
    d, n = 21, 5
    pi, Pm = a.g.simplex((n, d), 59), a.g.simplex((n, d, d), 60)
    th, out = a.sets(torch.tensor(np.linspace(2.0, 8.64, P), dtype=F64)), a.out('logpdf', (n,), F64, axis=1)
    a.keep += [pi, Pm, th]
    # (no alpha floor: with calc_z's floor 1 + 1e-6 every alpha sits on the floor at these states and the sets would coincide)
    a.inputs.update(pi=pi, P=Pm, thetas=th)
    return lambda: call('mfg_policy_logpdf', p(pi), p(Pm), n, d, p(th), a.K, *LOGPDF, p(out))


LOGZ_STARTS = 9


def _traj_log_z(per_learner):
    @row('traj_log_z_pop-%s' % ('stores' if per_learner else 'shared_store'), 'mfg_traj_log_z_pop')
    def build(a):
        cap, Tn, d = 3, 2, 21
        lead = (P,) if per_learner else ()
        state, action = a.g.simplex(lead + (cap, Tn, d), 76), a.g.simplex(lead + (cap, Tn, d, d), 77)
        if per_learner:
            state, action = a.sets(state), a.sets(action)
        th = a.sets(torch.tensor(np.linspace(7.9, 8.8, 2 * P), dtype=F64).view(P, 2))
        sh = a.sets(torch.tensor(np.linspace(-0.02, 0.05, P), dtype=F64))
        out, scratch = a.out('log_z', (cap,), F64), a.ws(4 * cap, I32)
        a.keep += [state, action, th, sh]
        a.inputs.update(state=state, action=action, thetas=th, shifts=sh)
        # (calc_z's alpha_scale 1, but no alpha floor: with its floor 1 + 1e-6 two sets coincide on the shared store)
        return lambda: _ops().traj_log_z_pop(state, action, [2, 0, 1], th, sh, float(np.log(LOGZ_STARTS)), alpha_scale=1.0,
                                             alpha_floor=0.0, out=out, scratch=scratch)


_traj_log_z(True)
_traj_log_z(False)


# ---------------------------------------------------------------------------------------------------
# the baselines: VAR and RNN
# ---------------------------------------------------------------------------------------------------
BD, BHD = 3, 3           # topics and rows per day of the baselines


def _days(a, n_days, seed):
    import rnn_ref
    return torch.as_tensor(rnn_ref.dirichlet_days(n_days, BHD, BD, seed), dtype=F64, device=a.dev).contiguous()


def _day_table(a, rows):
    return a.sets(torch.tensor(rows, dtype=I32))


VAR_SETS = dict(lag=[1, 2, 1, 2, 1, 2, 2], ridge=[1e-3, 1e-3, 1e-2, 3e-2, 0.1, 0.3, 1.0], origin=[0, 0, 1, 1, 0, 1, 0],
                train=[[0, 1], [1, 2], [2, 3], [3, 4], [4, 5], [0, 5], [1, 4]], test=[[5], [0], [1], [2], [3], [4], [2]])


@row('var_fit_pop', 'mfg_var_fit_pop', 'mfg_var_fit_workspace_bytes')
def _var_fit(a):
    ops, K = _ops(), a.K
    days = _days(a, 6, 4001)
    lags, ridges, origins = a.host_sets(VAR_SETS['lag']), a.host_sets(VAR_SETS['ridge']), a.host_sets(VAR_SETS['origin'])
    tr, te = _day_table(a, VAR_SETS['train']), _day_table(a, VAR_SETS['test'])
    table, nbytes = ops.var_models(lags, ridges, [2] * K, [1] * K, origins, BD)
    models = (table, ops.var_models_device(table, a.dev), nbytes)
    M, S_max = 1 + 2 * BD, BHD
    out = {n: a.out(n, shape[1:], dt) for n, (shape, dt) in ops.var_fit_shapes(K, BD, M, S_max, 1).items()}
    assert nbytes % 8 == 0, nbytes                       # (exactly the advertised bytes behind an fp64 view)
    ws = a.ws(nbytes, F64)
    a.keep += [days, tr, te, models]
    return lambda: ops.var_fit_pop(days, lags, ridges, tr, [2] * K, te, [1] * K, origins, out=out, workspace=ws, models=models,
                                   M=M, S_max=S_max)


RNN_SETS = dict(hidden=[4, 8, 4, 8, 4, 8, 8], lr=[1e-2, 3e-3, 3e-2, 1e-2, 3e-3, 3e-2, 1e-3], wd=[0.0, 1e-3, 0.0, 1e-3, 1e-4, 0.0, 1e-2],
                clip=[0.0, 0.02, 0.0, 0.05, 0.0, 0.02, 0.1], train=[[0, 1], [1, 2], [2, 3], [3, 4], [4, 5], [0, 5], [1, 4]],
                val=[[2], [3], [4], [5], [0], [1], [0]], test=[[5], [0], [1], [2], [3], [4], [2]])
RNN_EPOCHS = 2


@row('rnn_fit_pop', 'mfg_rnn_fit_pop', 'mfg_rnn_fit_workspace_bytes')
def _rnn_fit(a):
    import rnn_ref
    ops, K = _ops(), a.K
    days = _days(a, 6, 4002)
    W_max = ops.rnn_weight_count(8, BD)
    w0 = np.zeros((P, W_max))
    for s, Hn in enumerate(RNN_SETS['hidden']):
        w = rnn_ref.init_weights(Hn, BD, [77, s])
        w0[s, :w.size] = w
    w0 = a.sets(torch.as_tensor(w0, dtype=F64))
    hid, lrs, wds, clips = (a.host_sets(RNN_SETS[n]) for n in ('hidden', 'lr', 'wd', 'clip'))
    tr, va, te = (_day_table(a, RNN_SETS[n]) for n in ('train', 'val', 'test'))
    ep, two, one = [RNN_EPOCHS] * K, [2] * K, [1] * K
    table, nbytes = ops.rnn_models(hid, ep, lrs, wds, clips, two, one, one, BD, BHD)
    models = (table, ops.rnn_models_device(table, a.dev), nbytes)
    shapes = ops.rnn_fit_shapes(K, BHD, BD, W_max, RNN_EPOCHS, RNN_EPOCHS, 1)
    out = {n: a.out(n, shape[1:], dt) for n, (shape, dt) in shapes.items()}
    assert nbytes % 8 == 0, nbytes                       # (exactly the advertised bytes behind an fp64 view)
    ws = a.ws(nbytes, F64)
    a.keep += [days, w0, tr, va, te, models]
    return lambda: ops.rnn_fit_pop(days, w0, hid, ep, lrs, wds, clips, tr, two, va, one, te, one, out=out, workspace=ws,
                                   models=models)


# ---------------------------------------------------------------------------------------------------
# procedure C
# ---------------------------------------------------------------------------------------------------
_SMALL, _SMALL_INPUTS = {}, {}


def run(r, dev, K, guarded=True, first=0):
    """The row's call with K learners, synchronised; the bands checked.  Returns the Cycled."""
    a = Cycled(dev, K, guarded, first)
    issue = r.build(a)
    torch.cuda.synchronize()
    issue()
    torch.cuda.synchronize()
    a.check_bands()
    return a


def small(r, dev):
    """name -> [P, ...] of the K = P call of the row: computed once, shared, left unchanged."""
    if r.name not in _SMALL:
        a = run(r, dev, P, guarded=False)
        got = {n: t.clone() for n, t in a.compared().items()}
        assert_distinct(r.name, got)
        _SMALL[r.name] = got
        _SMALL_INPUTS[r.name] = {n: t.clone() for n, t in a.inputs.items()}
    return _SMALL[r.name]


def small_inputs(r, dev):
    """The inputs the row's builder noted for the small call (name -> tensor)."""
    small(r, dev)
    return _SMALL_INPUTS[r.name]


def alone(r, dev):
    """"The same bits alone and among others": the names of the buffers in which set s, run as the ONLY learner of a call
    (K = 1), differs from slice s of the small call, as (name, s) pairs."""
    want = small(r, dev)
    bad = []
    for s in range(P):
        got = run(r, dev, 1, guarded=False, first=s).compared()
        bad += [(n, s) for n in sorted(got) if not S.same(got[n][0], want[n][s])]
    return bad


def built(r, dev):
    """The row's K = P buffers as its builder declares them, the call NOT issued: the start values of the in/out buffers
    (.cmp) and the noted inputs (.inputs), for the comparisons with single-learner entry points."""
    a = Cycled(dev, P, guarded=False)
    r.build(a)
    return a


def unwritten(t):
    """True when an output still holds nothing but its fill (NaN / -7): the call did not write it at all."""
    return bool(torch.isnan(t).all()) if t.dtype.is_floating_point else bool((t == -7).all())


def cycled(r, dev, K):
    """Procedure C for one row and one K."""
    want = small(r, dev)
    a = run(r, dev, K)
    got = a.compared()
    assert set(got) == set(want)
    for n in sorted(got):
        assert_cycled('%s %s' % (r.name, n), got[n], want[n])
    return a


# ---------------------------------------------------------------------------------------------------
# procedure E: mfg_train_episodes_pop under a control, a validation and an evolve block
# ---------------------------------------------------------------------------------------------------
# One episode, one held-out check, one exploit / explore step.  The cycled sets tie the check's values massively (every learner
# of a set has the same value, bit for bit), across every seam of the 256-key rank tiles, so the tie-break by k decides the order.
E_K = (255, 256, 257, 513)                    # and POP_MAX_K
RETIRED_SET, INACTIVE_SET = 3, 5              # theta outside the mixed range: retired by the call; state 1 set by the caller
THETA_OUT = 90.0                              # |theta| (1 + |shift|) > 86
E_COLUMN, E_SEED = 6, 0xC0FFEE1234567
E_D = 21
E_FIRST_STEP = 7                              # the Philox step of the check's rollouts


def caller_inactive(K):
    """The learners the caller hands over with state 1: those of INACTIVE_SET and, at K >= 513, one whole rank tile."""
    k = np.arange(K)
    off = k % P == INACTIVE_SET
    if K >= 513:
        off |= (k >= 256) & (k < 512)
    return off


def expected_active(K):
    return ~caller_inactive(K) & (np.arange(K) % P != RETIRED_SET)


def evolve_counts(K, replace):
    """(n_top, n_bottom): a quarter of the active learners each, or -- replace = False -- more than there are active ones."""
    A = int(expected_active(K).sum())
    return (max(A // 4, 1), max(A // 4, 1)) if replace else (A - 1, 2)


def order_with_tile_local_ties(values, active, tile=256):
    """rank [K] (-1: not active) of a rank kernel whose tie-break compared the positions inside a tile (j mod 256 < k mod 256)
    instead of the learners' indices: what the inputs of procedure E must tell from the header's order."""
    values = np.where(np.isfinite(values), values, np.inf)
    K = len(values)
    k = np.arange(K)
    lt = values[None, :] < values[:, None]
    eq = (values[None, :] == values[:, None]) & ((k % tile)[None, :] < (k % tile)[:, None])
    before = ((lt | eq) & active[None, :]).sum(1)
    return np.where(active, before, -1).astype(np.int32)


def evolve_call(dev, K, counts=None):
    """mfg_train_episodes_pop, one episode, under a control and a validation block and -- counts = (n_top, n_bottom) -- an
    evolve block.  Returns (start, end): name -> CPU tensor of every in/out buffer and output before and after the call."""
    L, ops = _L(), _ops()
    d = E_D
    a = Cycled(dev, K, guarded=False)
    F = ops.num_features(d)
    theta = np.linspace(8.2, 9.0, P)
    theta[RETIRED_SET] = THETA_OUT
    mat, th, sh, al, sd, w, G, acc, lrc, lra, ws, sb = _pop_common(a, d, 78, episodes=1, theta=theta)
    a.cmp['lr_critic'], a.cmp['lr_actor'] = (lrc, 0), (lra, 0)
    pi = a.out('pi_io', (B, d))
    scratch, r, delta, g = _episode_bufs(a, d)
    import test_gpu_pop_validate as TV         # its held-out rows, so that its restatement of a check applies (evolve_small)
    emp = TV._emp(d)
    emp32, emp64 = torch.as_tensor(emp.astype(np.float32), device=dev), torch.as_tensor(emp, dtype=F64, device=dev)
    full = lambda v, dt: torch.full((K,), v, dtype=dt, device=dev)

    def put(name, t):
        a.cmp[name] = (t, 0)
        return t
    state = put('state', torch.as_tensor(caller_inactive(K).astype(np.int32), device=dev))
    status, run = put('status', full(0, I32)), put('episodes_run', full(0, I32))
    prev, stop = full(NAN, F64), full(-1.0, F64)
    val = dict(curve=a.out('curve', (1, 10), F64), checks=put('checks', full(0, I32)),
               best_value=put('best_value', full(float('inf'), F64)), best_check=put('best_check', full(-1, I32)),
               since_best=put('since_best', full(0, I32)), best_theta=a.out('best_theta', (), F64), best_w=a.out('best_w', (F,), F64))
    nv = ops.pop_validate_workspace_bytes(TV.N, TV.LR, d, K, TV.R, False)
    vws = a.ws(nv)
    if counts is not None:
        # order is scratch that the apply kernel reads back as learner indices: it starts as a VALID index everywhere, so that a
        # rank kernel that left a slot unwritten would give a wrong donor (seen below: order[:A] is compared) and nothing else
        order, active = torch.zeros(K, dtype=I32, device=dev), torch.full((1,), -7, dtype=I32, device=dev)
        evo = dict(order=order, active=active, rank=put('rank', torch.full((K, 1), -1, dtype=I32, device=dev)),
                   parent=put('parent', torch.full((K, 1), -1, dtype=I32, device=dev)), lr_log=a.out('lr_log', (1, 2), F64))
    ctx = ops.Context(dev)
    args = (p(mat), NUM_START, p(pi), p(scratch), B, K, d, T, 1, 0, 0, p(th), p(sh), p(al), p(w), GAMMA, L.REWARD_MFG_AC2, p(sd),
            3, 100, L.PRECISION_MIXED, p(lrc), p(lra), p(r), p(delta), p(g), p(G), p(acc), p(ws), sb)
    start = {n: t.cpu().clone() for n, t in a.compared().items()}
    torch.cuda.synchronize()
    before = ctx.bind_scoped()
    try:
        ctx.set_pop_control(state, status, prev, run, stop)
        ctx.set_pop_validate(emp32, emp64, period=1, column=E_COLUMN, with_score=False, first_step=E_FIRST_STEP, repeats=TV.R, workspace=vws,
                             workspace_bytes=nv, **val)
        if counts is not None:
            ctx.set_pop_evolve(lrc, lra, n_top=counts[0], n_bottom=counts[1], seed=E_SEED, **evo)
        call('mfg_train_episodes_pop', *args)
        torch.cuda.synchronize()
        assert ctx.status() == 0               # (under a control block a learner's theta is booked to the learner)
    finally:
        ctx.set_pop_evolve()
        ctx.set_pop_validate()
        ctx.set_pop_control()
        ctx.restore(before)
    end = {n: t.cpu().clone() for n, t in a.compared().items()}
    if counts is not None:
        end['order'], end['active'] = order.cpu(), active.cpu()
    ctx.close()
    return start, end


_E_SMALL = {}


def evolve_small(dev):
    """The K = P call without an evolve block: what every learner of a set holds when the step begins."""
    if 'end' not in _E_SMALL:
        start, end = evolve_call(dev, P)
        for n in start:                        # the retired and the inactive set: not one array touched
            if n not in ('state', 'status'):
                for s in (RETIRED_SET, INACTIVE_SET):
                    assert torch.equal(_bits(end[n][s]), _bits(start[n][s])), (n, s)
        assert end['state'].tolist() == [2 if s == RETIRED_SET else int(s == INACTIVE_SET) for s in range(P)]
        assert end['status'].tolist() == [int(s == RETIRED_SET) for s in range(P)]         # MFG_STATUS_MIXED_RANGE
        live = [s for s in range(P) if s not in (RETIRED_SET, INACTIVE_SET)]
        assert end['checks'][live].tolist() == [1] * len(live) and end['episodes_run'][live].tolist() == [1] * len(live)
        assert bool(torch.isfinite(end['curve'][live][:, :, :8]).all()) and end['best_check'][live].tolist() == [0] * len(live)
        assert bool(torch.isnan(end['curve'][live][:, :, 8:]).all())                        # (no scores were asked for)
        assert len(set(end['curve'][live, 0, E_COLUMN].tolist())) == len(live)              # five different values
        # the check's rows against _check_rows of tests/test_gpu_pop_validate.py (ops.evaluate_pop, which
        # tests/test_gpu_evaluate_pop.py holds against NumPy) on the thetas the call ends on
        # (one episode, one check: the theta of the check), columns 0-7 bit for bit as the header promises
        import types
        import test_gpu_pop_validate as TV
        sh, al, sd = (t[live] for t in Cycled(dev, P, False).policies()[1:])
        pop = types.SimpleNamespace(d=E_D, precision='mixed', _theta=end['theta'][live].to(dev).contiguous(), _shifts_dev=sh.contiguous(),
                                    _alphas_dev=al.contiguous(), _seeds_dev=sd.contiguous())
        rows = torch.as_tensor(TV._check_rows(pop, E_FIRST_STEP))
        assert torch.equal(_bits(rows[:, :8]), _bits(end['curve'][live, 0, :8])), 'the check rows differ from the restatement'
        _E_SMALL['end'] = end
    return _E_SMALL['end']


def expected_before_step(K, start, small_end):
    """What the big call's arrays hold when the evolve step begins: the small call's for the learners that took part, the
    start values for the others."""
    idx = torch.arange(K) % P
    tile = torch.as_tensor(caller_inactive(K) & (np.arange(K) % P != INACTIVE_SET))
    exp = {}
    for n, t in small_end.items():
        e = t.index_select(0, idx).clone()
        e[tile] = start[n][tile]
        exp[n] = e
    return exp


def evolved(dev, K, replace):
    """Procedure E for one K: everything the call leaves, exactly, against the small call and tests/pop_evolve_ref.py."""
    import pop_evolve_ref as ref
    n_top, n_bottom = evolve_counts(K, replace)
    sm = evolve_small(dev)
    start, end = evolve_call(dev, K, (n_top, n_bottom))
    exp = expected_before_step(K, start, sm)
    active = expected_active(K)
    A = int(active.sum())
    assert np.array_equal(end['state'].numpy() == 0, active)
    # the check's rows: the small call's, which evolve_small holds against _check_rows of tests/test_gpu_pop_validate.py
    assert torch.equal(_bits(end['curve']), _bits(exp['curve'])), 'curve: %s' % differing_learners(end['curve'], sm['curve'])
    values = end['curve'][:, 0, E_COLUMN].numpy()                                       # the device's own check values
    best = [exp[n].numpy() for n in ('best_value', 'best_check', 'since_best', 'best_theta', 'best_w')]
    out = ref.step(values, active, exp['theta'].numpy(), exp['w'].numpy(), exp['lr_critic'].numpy(), exp['lr_actor'].numpy(), s=0,
                   seed=E_SEED, n_top=n_top, n_bottom=n_bottom, extra=best)
    assert out['replaced'] == replace
    want = dict(exp)
    want.update(theta=out['theta'], w=out['w'], lr_critic=out['lr_critic'], lr_actor=out['lr_actor'], rank=out['rank'][:, None],
                parent=out['parent'][:, None], lr_log=out['lr'][:, None, :])
    want.update(zip(('best_value', 'best_check', 'since_best', 'best_theta', 'best_w'), out['extra']))
    assert int(end['active'][0]) == A
    got_order = end['order'][:A].numpy()
    assert np.array_equal(got_order, np.asarray(out['order'], dtype=np.int32)), 'order'
    assert np.array_equal(np.sort(got_order), np.flatnonzero(active)), 'order is not a permutation of the active learners'
    for n in sorted(want):
        w_ = torch.as_tensor(np.ascontiguousarray(want[n])) if not isinstance(want[n], torch.Tensor) else want[n]
        assert w_.dtype == end[n].dtype and w_.shape == end[n].shape, (n, w_.dtype, end[n].dtype, w_.shape, end[n].shape)
        ne = (_bits(w_).reshape(K, -1) != _bits(end[n]).reshape(K, -1)).any(-1)
        assert not bool(ne.any()), '%s: learners %s differ' % (n, ne.nonzero().reshape(-1)[:8].tolist())
    if replace:
        moved = out['parent'] != np.where(active, np.arange(K), -1)
        assert moved.sum() == n_bottom and not np.array_equal(out['lr_critic'], exp['lr_critic'].numpy())
    return out
