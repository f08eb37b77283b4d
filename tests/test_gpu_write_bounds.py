"""-m gpu: no kernel writes outside its outputs or its workspace.

Every device buffer a call may write -- outputs, G, theta / w / reward_acc where the call updates them, the workspace -- and
every input is a tests/guard_bands.py Guarded: a view into the middle of one allocation with 1 MiB of 0xA5 on either side,
the back band starting at the very byte where the buffer ends.  Workspaces have EXACTLY the bytes the matching
*_workspace_bytes query returns.  After the call each case asserts
  1. both bands of every buffer are untouched,
  2. the interiors equal, bit for bit, what the plain call (ops.*, fresh exact-size 16-byte-aligned tensors, the same
     arguments) returns -- where misaligned buffers are handed in, this is the equivalence test of the fall-back forms,
  3. no output element still holds its NaN fill.
A stray store lands in a band of the same allocation: it is recorded and cannot fault.  No case hands a call a buffer smaller
than it needs.  Groups A and B also compare with the NumPy oracle, with the assertions of test_step_given_P
(tests/test_gpu_parity.py); no tolerance is new here.

Groups: A mfg_step_given_P at small batches over output / input alignments; B its burst-store forms at cap-derived sizes;
C mfg_sample_dirichlet and mfg_rollout; D mfg_train_rollout (MFG_TRAIN_APPLY) and mfg_train_rollout_deferred; E the batch sums
(mfg_td_pg_accumulate, mfg_grad_accumulate, mfg_grad_apply); F the launch-once kernels; G the calls with an advertised
workspace.
"""
import ctypes as C
import functools

import numpy as np
import pytest

torch = pytest.importorskip('torch')

from guard_bands import Guarded, check_all

pytestmark = pytest.mark.gpu

NAN = float('nan')
THETA, SHIFT, SCALE, GAMMA = 8.86349, 0.16, 12000.0, 0.9
F32, F64, I32, I64, U8 = torch.float32, torch.float64, torch.int32, torch.int64, torch.uint8
WAVES = 4                                           # wavefronts per block of the step kernels (BLOCK / WAVE, csrc/mfg_core.h)


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.fail('-m gpu tests need a GPU: the HIP path has no CPU fallback')
    _ops().init()
    return torch.device('cuda:0')


def _ops():
    from discrete_mean_field_game_amd import ops
    return ops


def _L():
    from discrete_mean_field_game_amd import _lib
    return _lib


def _O():
    from oracle import mfg_oracle
    return mfg_oracle


@functools.lru_cache(maxsize=None)
def _cus():
    cu = C.c_int(0)
    _L().check(_L().lib().mfg_device_info(C.byref(cu), None, 0), 'mfg_device_info')
    assert cu.value > 0
    return cu.value


def _call(name, *args):
    """One C ABI call on torch's current stream."""
    L = _L()
    L.check(getattr(L.lib(), name)(*args, torch.cuda.current_stream().cuda_stream), name)


def _out(dev, shape, dtype=F32, offset=0, fill=NAN):
    return Guarded(shape, dtype, dev, offset=offset, fill=fill)


def _in(t, offset=0):
    return Guarded(tuple(t.shape), t.dtype, t.device, offset=offset, fill=t)


def _ws(dev, nbytes, dtype=F64, zero=True):
    """A workspace of exactly nbytes bytes (zeroed where the header asks for it; 0xA5 otherwise: its contents are scratch)."""
    item = torch.empty(0, dtype=dtype).element_size()
    assert nbytes % item == 0, 'advertised workspace of %d bytes is no whole number of %s' % (nbytes, dtype)
    return Guarded((nbytes // item,), dtype, dev, fill=0 if zero else None)


def _p(g):
    return None if g is None else g.ptr()


def _simplex(dev, shape, seed):
    """Rows on the simplex, generated on the device (fp32, every entry > 0)."""
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    x = torch.rand(shape, device=dev, generator=g) + 1e-3
    return (x / x.sum(-1, keepdim=True)).contiguous()


def _randn64(dev, shape, seed):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    return torch.randn(shape, device=dev, generator=g, dtype=F64)


def _same(a, b):
    if a.dtype.is_floating_point:
        it = I32 if a.element_size() == 4 else I64
        return torch.equal(a.contiguous().view(it), b.contiguous().view(it))
    return torch.equal(a, b)


def _verify(bufs, want, ctx=''):
    """The three assertions of a case: bufs {name: Guarded | None}, want {name: tensor of the plain call} for the outputs."""
    torch.cuda.synchronize()
    check_all(*[('%s %s' % (ctx, name), g) for name, g in bufs.items()])
    for name, ref in want.items():
        got = bufs[name].t
        if got.dtype.is_floating_point:
            assert not bool(torch.isnan(got).any()), '%s %s: an element still holds its NaN fill' % (ctx, name)
        assert tuple(ref.shape) == tuple(got.shape), (ctx, name)
        assert _same(got, ref), '%s %s: differs from the plain call' % (ctx, name)


def _theta(dev):
    return torch.tensor([THETA], dtype=F64, device=dev)


# ---------------------------------------------------------------------------------------------------
# A. mfg_step_given_P, small batches
# ---------------------------------------------------------------------------------------------------
ALIGNMENTS = [(0, 0, 0, 0), (4, 0, 0, 0), (0, 4, 0, 0), (8, 8, 0, 0), (4, 4, 4, 4), (0, 0, 0, 4)]   # pi_next, reward, P, pi
STEP_SHAPES = ([(21, B) for B in (1, 11, 12, 13, 25)] + [(15, B) for B in (1, 3, 4, 5, 17)] + [(7, B) for B in (35, 36, 37)]
               + [(3, 257), (64, 3), (64, 5)] + [(d, B) for d in (65, 66, 68, 128, 256, 130, 320, 511, 512) for B in (1, 5)])


@functools.lru_cache(maxsize=None)
def _step_case(d, B):
    """Host inputs of a (d, B) and the oracle's outputs, shared by the cases of that shape (read only)."""
    rs = np.random.RandomState(d * 1000 + B)
    pi = rs.dirichlet(np.ones(d), size=B).astype(np.float32)
    P = rs.dirichlet(np.ones(d), size=(B, d)).astype(np.float32)
    O = _O()
    return pi, P, O.transition(P, pi).astype(np.float32), (O.calc_reward(P, pi), O.calc_reward_synthetic(P, pi))


def _rel(a, b, floor):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.max(np.abs(a - b) / np.maximum(np.abs(b), floor))


def _step_guarded(dev, pi, P, kind, align, ctx, want_pn, want_r):
    B, d = pi.shape
    bufs = {'pi_next': _out(dev, (B, d), offset=align[0]),
            'reward': _out(dev, (B,), offset=align[1]) if kind is not None else None,
            'P': _in(P, align[2]), 'pi': _in(pi, align[3])}
    _call('mfg_step_given_P', bufs['pi'].ptr(), bufs['P'].ptr(), B, d, kind or 0, bufs['pi_next'].ptr(), _p(bufs['reward']))
    want = {'pi_next': want_pn, 'P': P, 'pi': pi}
    if kind is not None:
        want['reward'] = want_r
    _verify(bufs, want, ctx)


@pytest.mark.parametrize('kind', [0, 1, None], ids=['kind0', 'kind1', 'no_reward'])
@pytest.mark.parametrize('d,B', STEP_SHAPES)
def test_step_given_P_small(dev, d, B, kind):
    """Every alignment of (pi_next, reward, P, pi): a misaligned pi_next or reward with an aligned P takes k_step_wave in place
    of the batched kernel and k_step_large<1, R> in place of k_step_rows / the vector forms (d = 128, 256, 66, 68, ...), which
    no Python caller reaches (ops.step_given_P allocates its outputs).  d = 21: B either side of the lcm(G, 4) = 12 unit the
    main launch covers; d = 15: of 4; d = 7: 9 per wave, 36 per block; B = 5 at d > 64 crosses the 4-wave block."""
    pi_h, P_h, ref_pn, ref_r = _step_case(d, B)
    pi, P = torch.as_tensor(pi_h, device=dev), torch.as_tensor(P_h, device=dev)
    pn, r = _ops().step_given_P(pi, P, reward_kind=kind or 0, want_reward=kind is not None)
    assert np.array_equal(pn.cpu().numpy(), ref_pn)
    if kind is not None:
        assert _rel(r.cpu().numpy(), ref_r[kind], 1e-30) < 1e-6
    for align in ALIGNMENTS:
        _step_guarded(dev, pi, P, kind, align, 'd=%d B=%d align=%s' % (d, B, align), pn, r)


# ---------------------------------------------------------------------------------------------------
# B. mfg_step_given_P, burst stores
# ---------------------------------------------------------------------------------------------------
def _step_kb(B, d, cus):
    """(KB, B4) of launch_step_given_P (csrc/mfg_step.hip) for d = 21 / 15 with 16-byte-aligned buffers: KB = 0 is the per-tile
    kernel; B4 trajectories go to the main launch, B - B4 to the ragged one."""
    G = 64 // d
    unit = G if G % 4 == 0 else (2 * G if G % 2 == 0 else 4 * G)
    B4 = B - B % unit
    ntiles = (B4 + G - 1) // G
    nw_target = cus * 2 * WAVES
    kb = 0
    for cand in (32, 16, 8):
        ns = (ntiles + cand - 1) // cand
        rr = (ns + nw_target - 1) // nw_target
        if not kb and rr >= 2 and 10 * ns >= 9 * rr * nw_target:
            kb = cand
    return kb, B4


def _smallest_batch_for_kb(d, kb, cus):
    """The smallest B that selects KB = kb with B mod lcm(G, 4) != 0 (the ragged kernel runs) and a ragged last super tile (the
    per-tile fall-back inside the batched kernel runs)."""
    G = 64 // d
    unit = G if G % 4 == 0 else (2 * G if G % 2 == 0 else 4 * G)
    nw_target = cus * 2 * WAVES
    ns_min = (9 * 2 * nw_target + 9) // 10               # rr = 2, 10 ns >= 9 rr nw_target
    ntiles_min = (ns_min - 1) * kb + 1                   # the fewest tiles that make ns_min super tiles
    B4 = (ntiles_min * G + unit - 1) // unit * unit
    for _ in range(4 * kb):
        if _step_kb(B4, d, cus)[0] == kb and B4 % (kb * G) != 0:
            break
        B4 += unit
    B = B4 + (5 if unit > 5 else 1)
    assert _step_kb(B, d, cus) == (kb, B4) and B % unit != 0 and B4 % (kb * G) != 0
    return B


def _rows_kt(B, cus):
    """The super-tile size of k_step_rows (d = 128 / 256, aligned buffers): 8 or 1."""
    nw_target = cus * 2 * WAVES                          # MFG_ROWS_BPC = 2
    ns8 = (B + 7) // 8
    rr8 = (ns8 + nw_target - 1) // nw_target
    return 8 if (ns8 >= nw_target and 10 * ns8 >= 9 * rr8 * nw_target) else 1


def _burst_batch(case):
    cus = _cus()
    if case[0] in (21, 15):
        return _smallest_batch_for_kb(case[0], case[1], cus)
    B = 8 * cus * 2 * WAVES - (5 if case[0] == 128 else 1)
    assert _rows_kt(B, cus) == 8 and B % 8 != 0
    return B


@pytest.mark.parametrize('case', [(21, 8), (21, 16), (21, 32), (15, 8), (128, 0), (256, 0)],
                         ids=['d21-KB8', 'd21-KB16', 'd21-KB32', 'd15-KB8', 'd128-KT8', 'd256-KT8'])
def test_step_given_P_burst_stores(dev, case):
    """One case per store form of k_step_wave_batched (KB = 8 / 16 / 32) and of k_step_rows<.., 8>, at the smallest batch the
    launch rule (restated above, from the CU count) gives that form, with B mod 12 != 0 and a ragged last super tile: bursts,
    the per-tile fall-back and the ragged kernel all store in one call.  Then the same call with `reward` 4 bytes off a
    16-byte boundary, which must fall back (out16) and agree bit for bit.  The oracle sees the last 300 (20) trajectories."""
    d = case[0]
    B = _burst_batch(case)
    pi = _simplex(dev, (B, d), B)
    P = _simplex(dev, (B, d, d), B + 1)
    pn, r = _ops().step_given_P(pi, P, reward_kind=0)
    n = 300 if d <= 64 else 20
    Pn, pin = P[B - n:].cpu().numpy().astype(np.float64), pi[B - n:].cpu().numpy().astype(np.float64)
    assert np.array_equal(pn[B - n:].cpu().numpy(), _O().transition(Pn, pin).astype(np.float32))
    assert _rel(r[B - n:].cpu().numpy(), _O().calc_reward(Pn, pin), 1e-30) < 1e-6
    for align in ((0, 0, 0, 0), (0, 4, 0, 0)):
        _step_guarded(dev, pi, P, 0, align, 'd=%d B=%d align=%s' % (d, B, align), pn, r)


# ---------------------------------------------------------------------------------------------------
# C. mfg_sample_dirichlet and mfg_rollout
# ---------------------------------------------------------------------------------------------------
CORE_SHAPES = [(21, 1), (21, 13), (15, 5), (7, 37), (5, 257), (64, 5), (65, 3), (127, 2), (128, 5), (130, 3), (256, 2), (320, 2),
               (448, 3), (512, 1)]
CORE_CASES = [(d, B, m) for d, B in CORE_SHAPES for m in ((1, 2) if d in (21, 15) else (0,))]
CORE_IDS = ['d%d-B%d-map%d' % c for c in CORE_CASES]


class _mapping:
    """mfg_set_core_mapping(mode) for a block; the previous mode comes back in any case."""

    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        self.prev = _L().lib().mfg_set_core_mapping(self.mode)

    def __exit__(self, *exc):
        _L().lib().mfg_set_core_mapping(self.prev)


@pytest.mark.parametrize('precision', ['mixed', 'f64'])
@pytest.mark.parametrize('d,B,mode', CORE_CASES, ids=CORE_IDS)
def test_sample_dirichlet(dev, d, B, mode, precision):
    ops = _ops()
    pi, th = _simplex(dev, (B, d), 7 * d + B), _theta(dev)
    with _mapping(mode):
        want = ops.sample_dirichlet(pi, th, SHIFT, SCALE, seed=99, step=5, traj_offset=1000, precision=precision)
        bufs = {'P': _out(dev, (B, d, d)), 'pi': _in(pi), 'theta': _in(th)}
        ops.sample_dirichlet(bufs['pi'].t, bufs['theta'].t, SHIFT, SCALE, seed=99, step=5, traj_offset=1000, out=bufs['P'].t,
                             precision=precision)
        _verify(bufs, {'P': want, 'pi': pi, 'theta': th}, 'sample d=%d B=%d' % (d, B))


ROLLOUT_FLAGS = [('env', False, False), ('td', True, False), ('td+P', True, True), ('P', False, True)]


def _rollout_bufs(dev, B, d, T, td, write_P, ext, pi_traj=True):
    F = _ops().num_features(d)
    b = {'pi_traj': _out(dev, (B, T + 1, d)) if pi_traj else None, 'pi_last': _out(dev, (B, d)),
         'reward': None if ext else _out(dev, (B, T))}
    if td:
        b['delta'], b['g'] = _out(dev, (B, T), F64), _out(dev, (B, T), F64)
        if not ext:
            b['G'] = _out(dev, (F + 3,), F64)
            b['ws'] = _ws(dev, int(_L().lib().mfg_workspace_bytes(B * T, d)))
    if write_P:
        b['P'] = _out(dev, (B, T, d, d))
    return b


def _rollout_case(dev, d, B, T, td, write_P, precision, kind, ctx):
    ops = _ops()
    pi0, th = _simplex(dev, (B, d), 31 + d + B), _theta(dev)
    w = _randn64(dev, (ops.num_features(d),), d).abs_() if td else None
    kw = dict(w=w, gamma=GAMMA, reward_kind=kind, seed=99, first_step=5, traj_offset=1000, td=td, write_P=write_P,
              precision=precision)
    plain = ops.rollout(pi0, T, th, SHIFT, SCALE, **kw)
    ext = kind == _L().REWARD_EXTERNAL
    b = _rollout_bufs(dev, B, d, T, td, write_P, ext)
    ins = {'pi0': _in(pi0), 'theta': _in(th), 'w': _in(w) if td else None}
    kw['w'] = ins['w'].t if td else None
    ops.rollout(ins['pi0'].t, T, ins['theta'].t, SHIFT, SCALE, out={k: v.t for k, v in b.items() if k not in ('G', 'ws') and v is not None},
                G=b['G'].t if 'G' in b else None, ws=b['ws'].t if 'ws' in b else None, **kw)
    want = {k: plain[k] for k in b if k != 'ws' and b[k] is not None}
    want.update(pi0=pi0, theta=th)
    if td:
        want['w'] = w
    _verify(dict(b, **ins), want, ctx)
    return plain


@pytest.mark.parametrize('precision', ['mixed', 'f64'])
@pytest.mark.parametrize('d,B,mode', CORE_CASES, ids=CORE_IDS)
def test_rollout(dev, d, B, mode, precision):
    """T = 1 and 3 under the four flag sets: up to six outputs per launch from the packed mapping (3 / 4 / 64 // d trajectories
    per wave), the one-trajectory-per-wave mapping (mode 2) and the R = 2 .. 8 wave-per-trajectory instantiations; B is a ragged
    last tile of each.  T = 1 with a workspace is the sums-fused step form (core_sums_rows): the workspace has exactly
    mfg_workspace_bytes(B T, d) bytes.  Once per case the env-only call runs with pi_traj = NULL."""
    L = _L()
    with _mapping(mode):
        for T in (1, 3):
            for name, td, write_P in ROLLOUT_FLAGS:
                ctx = 'rollout d=%d B=%d T=%d %s' % (d, B, T, name)
                plain = _rollout_case(dev, d, B, T, td, write_P, precision, L.REWARD_MFG_AC2, ctx)
        # env only, pi_traj = NULL (T = 3): pi_last and reward are the only outputs
        T = 3
        pi0, th = _simplex(dev, (B, d), 31 + d + B), _theta(dev)
        b = _rollout_bufs(dev, B, d, T, False, False, False, pi_traj=False)
        b.update(pi0=_in(pi0), theta=_in(th))
        flags = L.ROLLOUT_F64 if precision == 'f64' else 0
        _call('mfg_rollout', b['pi0'].ptr(), B, d, T, b['theta'].ptr(), SHIFT, SCALE, None, GAMMA, L.REWARD_MFG_AC2, 99, 5, 1000,
              flags, None, b['pi_last'].ptr(), b['reward'].ptr(), None, None, None, None, 0, None, 0)
        env = _ops().rollout(pi0, T, th, SHIFT, SCALE, gamma=GAMMA, seed=99, first_step=5, traj_offset=1000, td=False,
                             precision=precision)
        _verify(b, {'pi_last': env['pi_last'], 'reward': env['reward'], 'pi0': pi0, 'theta': th},
                'rollout d=%d B=%d T=3 env, pi_traj NULL' % (d, B))
        assert _same(plain['pi_last'], env['pi_last'])      # (the last flag set above, WRITE_P only, T = 3: the same states)


@pytest.mark.parametrize('precision', ['mixed', 'f64'])
@pytest.mark.parametrize('d,B', [(21, 13), (130, 3)])
def test_rollout_external_reward(dev, d, B, precision):
    """MFG_REWARD_EXTERNAL (the IRL step): no reward, no G, no workspace; delta and g are still written."""
    for T in (1, 3):
        for write_P in (False, True):
            _rollout_case(dev, d, B, T, True, write_P, precision, _L().REWARD_EXTERNAL,
                          'rollout external d=%d B=%d T=%d P=%d' % (d, B, T, write_P))


# ---------------------------------------------------------------------------------------------------
# D. mfg_train_rollout with MFG_TRAIN_APPLY, mfg_train_rollout_deferred
# ---------------------------------------------------------------------------------------------------
TRAIN_SHAPES = [(21, 13, 3), (15, 5, 2), (47, 9, 2), (128, 5, 2)]
LR_C, LR_A = 0.1, 0.001
NUM_START = 40


def _train_inputs(dev, d, B):
    mat = _simplex(dev, (NUM_START, d), 900 + d)
    g = torch.Generator(device=dev)
    g.manual_seed(d + B)
    idx = torch.randint(NUM_START, (B,), device=dev, generator=g, dtype=I32)
    w = _randn64(dev, (_ops().num_features(d),), d).abs_()
    return mat, idx, w


def _train_bufs(B, d, T, dev, guarded):
    shapes = {'pi_traj': ((B, T + 1, d), F32), 'pi_last': ((B, d), F32), 'reward': ((B, T), F32), 'delta': ((B, T), F64),
              'g': ((B, T), F64)}
    if guarded:
        return {k: _out(dev, s, dt) for k, (s, dt) in shapes.items()}
    return {k: torch.full(s, NAN, dtype=dt, device=dev) for k, (s, dt) in shapes.items()}


@pytest.mark.parametrize('with_idx', [True, False], ids=['idx', 'drawn'])
@pytest.mark.parametrize('d,B,T', TRAIN_SHAPES)
def test_train_rollout_apply(dev, d, B, T, with_idx):
    """theta and reward_acc are ONE double each: their neighbours on either side are the point.  w (F), G (F + 3) and the
    workspace (exactly mfg_workspace_bytes(B T, d), zeroed once) are written by the launch that finishes the sums."""
    ops = _ops()
    F = ops.num_features(d)
    mat, idx, w0 = _train_inputs(dev, d, B)
    th0, acc0 = _theta(dev), torch.tensor([-3.25], dtype=F64, device=dev)
    nws = int(_L().lib().mfg_workspace_bytes(B * T, d))
    kw = dict(lr_critic=LR_C, lr_actor=LR_A, apply=True, seed=7, first_step=3, traj_offset=100)
    # the plain call
    th, w, acc = th0.clone(), w0.clone(), acc0.clone()
    G = torch.zeros(F + 3, dtype=F64, device=dev)
    plain = ops.train_rollout(mat, idx if with_idx else None, T, th, SHIFT, SCALE, w, GAMMA, G, ops.workspace(B * T, d, dev),
                              _train_bufs(B, d, T, dev, False), reward_acc=acc, **kw)
    # guarded
    b = _train_bufs(B, d, T, dev, True)
    par = {'theta': _in(th0), 'w': _in(w0), 'reward_acc': _in(acc0), 'G': _out(dev, (F + 3,), F64), 'ws': _ws(dev, nws),
           'mat_pi0': _in(mat), 'idx': _in(idx) if with_idx else None}
    ops.train_rollout(par['mat_pi0'].t, par['idx'].t if with_idx else None, T, par['theta'].t, SHIFT, SCALE, par['w'].t, GAMMA,
                      par['G'].t, par['ws'].t, {k: v.t for k, v in b.items()}, reward_acc=par['reward_acc'].t, **kw)
    want = dict(plain, theta=th, w=w, reward_acc=acc, G=G, mat_pi0=mat)
    if with_idx:
        want['idx'] = idx
    _verify(dict(b, **par), want, 'train_rollout d=%d B=%d T=%d' % (d, B, T))
    assert not torch.equal(th, th0) and not torch.equal(acc, acc0)      # (the update did run)


@pytest.mark.parametrize('with_idx', [True, False], ids=['idx', 'drawn'])
@pytest.mark.parametrize('d,B,T', TRAIN_SHAPES)
def test_train_rollout_deferred(dev, d, B, T, with_idx):
    """The pending update lands in (theta_out, w_out) -- one double and F doubles -- and in *reward_acc_pending; theta, w and
    G_pending are inputs."""
    ops = _ops()
    F = ops.num_features(d)
    mat, idx, w0 = _train_inputs(dev, d, B)
    th0, acc0 = _theta(dev), torch.tensor([-3.25], dtype=F64, device=dev)
    Gp = _randn64(dev, (F + 3,), 11 * d)
    Gp[F + 2] = 7.0
    nws = int(_L().lib().mfg_workspace_bytes(B * T, d))
    kw = dict(seed=7, first_step=3, traj_offset=100)
    acc, th_out, w_out = acc0.clone(), torch.full((1,), NAN, dtype=F64, device=dev), torch.full((F,), NAN, dtype=F64, device=dev)
    G = torch.zeros(F + 3, dtype=F64, device=dev)
    plain = ops.train_rollout_deferred(mat, idx if with_idx else None, T, th0, w0, (Gp, LR_C, LR_A, acc), th_out, w_out, SHIFT,
                                       SCALE, GAMMA, G, ops.workspace(B * T, d, dev), _train_bufs(B, d, T, dev, False), **kw)
    b = _train_bufs(B, d, T, dev, True)
    par = {'theta': _in(th0), 'w': _in(w0), 'G_pending': _in(Gp), 'reward_acc': _in(acc0), 'theta_out': _out(dev, (1,), F64),
           'w_out': _out(dev, (F,), F64), 'G': _out(dev, (F + 3,), F64), 'ws': _ws(dev, nws), 'mat_pi0': _in(mat),
           'idx': _in(idx) if with_idx else None}
    ops.train_rollout_deferred(par['mat_pi0'].t, par['idx'].t if with_idx else None, T, par['theta'].t, par['w'].t,
                               (par['G_pending'].t, LR_C, LR_A, par['reward_acc'].t), par['theta_out'].t, par['w_out'].t, SHIFT,
                               SCALE, GAMMA, par['G'].t, par['ws'].t, {k: v.t for k, v in b.items()}, **kw)
    want = dict(plain, theta=th0, w=w0, G_pending=Gp, reward_acc=acc, theta_out=th_out, w_out=w_out, G=G, mat_pi0=mat)
    if with_idx:
        want['idx'] = idx
    _verify(dict(b, **par), want, 'train_rollout_deferred d=%d B=%d T=%d' % (d, B, T))
    assert not torch.equal(th_out, th0) and not torch.equal(acc, acc0)


# ---------------------------------------------------------------------------------------------------
# E. batch sums
# ---------------------------------------------------------------------------------------------------
SUM_D = [15, 21, 28, 29, 40, 64, 80, 128, 144, 512]


def _sum_sizes(d):
    """N = 1 and one chunk + 1 where the test suite restates the chunk (oracle/grad_index_ref.py: 64 samples for d <= 28); else
    N in {1, 37, 1025}."""
    from oracle import grad_index_ref as R
    if d <= R.GRAD_SMALL_MAX_D:
        return [1, R.GS_CH + 1]
    return [1, 37, 1025]


def _sum_inputs(dev, d, N):
    pi = _simplex(dev, (N, d), 3 * d + N)
    delta, g = _randn64(dev, (N,), d + N), _randn64(dev, (N,), d + N + 1)
    reward = _randn64(dev, (N,), d + N + 2).float()
    F = _ops().num_features(d)
    return pi, delta, g, reward, _randn64(dev, (F,), d).abs_(), _randn64(dev, (F + 3,), d + 5)


@pytest.mark.parametrize('accumulate', [0, 1])
@pytest.mark.parametrize('d', SUM_D)
def test_td_pg_accumulate(dev, d, accumulate):
    ops = _ops()
    F = ops.num_features(d)
    for precision in ('mixed', 'f64'):
        for N in _sum_sizes(d):
            pi, _, _, reward, w, G0 = _sum_inputs(dev, d, N)
            pin, P, th = _simplex(dev, (N, d), 5 * d + N), _simplex(dev, (N, d, d), 7 * d + N), _theta(dev)
            G = G0.clone()
            delta, g, _ = ops.td_pg_accumulate(pi, pin, P, reward, w, th, SHIFT, GAMMA, G=G, accumulate=bool(accumulate),
                                               precision=precision)
            b = {'delta': _out(dev, (N,), F64), 'g': _out(dev, (N,), F64),
                 'G': _in(G0) if accumulate else _out(dev, (F + 3,), F64),
                 'ws': _ws(dev, int(_L().lib().mfg_workspace_bytes(N, d))), 'pi': _in(pi), 'pi_next': _in(pin), 'P': _in(P),
                 'reward': _in(reward), 'w': _in(w), 'theta': _in(th)}
            ops.td_pg_accumulate(b['pi'].t, b['pi_next'].t, b['P'].t, b['reward'].t, b['w'].t, b['theta'].t, SHIFT, GAMMA,
                                 G=b['G'].t, accumulate=bool(accumulate), ws=b['ws'].t, precision=precision,
                                 out=(b['delta'].t, b['g'].t))
            _verify(b, dict(delta=delta, g=g, G=G, pi=pi, pi_next=pin, P=P, reward=reward, w=w, theta=th),
                    'td_pg_accumulate d=%d N=%d %s' % (d, N, precision))


@pytest.mark.parametrize('accumulate', [0, 1])
@pytest.mark.parametrize('d', SUM_D)
def test_grad_accumulate(dev, d, accumulate):
    """accumulate = 1 also runs add_reward = 1: delta is then updated in place (and is a written buffer)."""
    ops = _ops()
    F = ops.num_features(d)
    for N in _sum_sizes(d):
        pi, delta0, g, reward, _, G0 = _sum_inputs(dev, d, N)
        G, delta = G0.clone(), delta0.clone()
        ops.grad_accumulate(pi, delta, g, reward, G, ops.workspace(N, d, dev), add_reward=bool(accumulate),
                            accumulate=bool(accumulate))
        b = {'delta': _in(delta0), 'G': _in(G0) if accumulate else _out(dev, (F + 3,), F64),
             'ws': _ws(dev, int(_L().lib().mfg_workspace_bytes(N, d))), 'pi': _in(pi), 'g': _in(g), 'reward': _in(reward)}
        ops.grad_accumulate(b['pi'].t, b['delta'].t, b['g'].t, b['reward'].t, b['G'].t, b['ws'].t, add_reward=bool(accumulate),
                            accumulate=bool(accumulate))
        _verify(b, dict(delta=delta, G=G, pi=pi, g=g, reward=reward), 'grad_accumulate d=%d N=%d' % (d, N))


@pytest.mark.parametrize('add_reward', [0, 1])
@pytest.mark.parametrize('d', SUM_D)
def test_grad_apply(dev, d, add_reward):
    """The update rides in the kernel that finishes the sums: w, theta and reward_acc (one double each for the last two) are
    written next to G."""
    ops = _ops()
    F = ops.num_features(d)
    for N in _sum_sizes(d):
        pi, delta0, g, reward, w0, _ = _sum_inputs(dev, d, N)
        th0, acc0 = _theta(dev), torch.tensor([-3.25], dtype=F64, device=dev)
        G, delta, w, th, acc = torch.zeros(F + 3, dtype=F64, device=dev), delta0.clone(), w0.clone(), th0.clone(), acc0.clone()
        ops.grad_apply(pi, delta, g, reward, G, ops.workspace(N, d, dev), LR_C, LR_A, w, th, reward_acc=acc,
                       add_reward=bool(add_reward))
        b = {'delta': _in(delta0), 'G': _out(dev, (F + 3,), F64), 'w': _in(w0), 'theta': _in(th0), 'reward_acc': _in(acc0),
             'ws': _ws(dev, int(_L().lib().mfg_workspace_bytes(N, d))), 'pi': _in(pi), 'g': _in(g), 'reward': _in(reward)}
        ops.grad_apply(b['pi'].t, b['delta'].t, b['g'].t, b['reward'].t, b['G'].t, b['ws'].t, LR_C, LR_A, b['w'].t, b['theta'].t,
                       reward_acc=b['reward_acc'].t, add_reward=bool(add_reward))
        _verify(b, dict(delta=delta, G=G, w=w, theta=th, reward_acc=acc, pi=pi, g=g, reward=reward),
                'grad_apply d=%d N=%d' % (d, N))
        assert not torch.equal(th, th0)


# ---------------------------------------------------------------------------------------------------
# F. launch-once kernels
# ---------------------------------------------------------------------------------------------------
def _f_value(dev, d, B):
    pi, w = _simplex(dev, (B, d), d + B), _randn64(dev, (_ops().num_features(d),), d)
    b = {'value': _out(dev, (B,), F64), 'pi': _in(pi), 'w': _in(w)}
    _call('mfg_value', b['pi'].ptr(), b['w'].ptr(), B, d, b['value'].ptr())
    return b, dict(value=_ops().value(pi, w), pi=pi, w=w)


def _f_features(dev, d, B):
    pi = _simplex(dev, (B, d), d + B)
    b = {'phi': _out(dev, (B, _ops().num_features(d)), F64), 'pi': _in(pi)}
    _call('mfg_features', b['pi'].ptr(), B, d, b['phi'].ptr())
    return b, dict(phi=_ops().features(pi), pi=pi)


def _f_alpha(dev, d, B):
    pi, th = _simplex(dev, (B, d), d + B), _theta(dev)
    b = {'alpha': _out(dev, (B, d, d), F64), 'alpha_deriv': _out(dev, (B, d, d), F64), 'pi': _in(pi), 'theta': _in(th)}
    _call('mfg_alpha', b['pi'].ptr(), B, d, b['theta'].ptr(), SHIFT, b['alpha'].ptr(), b['alpha_deriv'].ptr())
    a, ad = _ops().alpha(pi, th, SHIFT)
    return b, dict(alpha=a, alpha_deriv=ad, pi=pi, theta=th)


def _f_score(dev, d, B):
    pi, P, th = _simplex(dev, (B, d), d + B), _simplex(dev, (B, d, d), d + B + 1), _theta(dev)
    L = _L()
    b = {'g_mixed': _out(dev, (B,), F64), 'g_f64': _out(dev, (B,), F64), 'pi': _in(pi), 'P': _in(P), 'theta': _in(th)}
    for prec in ('mixed', 'f64'):
        _call('mfg_score', b['pi'].ptr(), b['P'].ptr(), B, d, b['theta'].ptr(), SHIFT, L.PRECISIONS[prec], b['g_' + prec].ptr())
    return b, dict(g_mixed=_ops().score(pi, P, th, SHIFT, 'mixed'), g_f64=_ops().score(pi, P, th, SHIFT, 'f64'), pi=pi, P=P,
                   theta=th)


def _f_policy_logpdf(dev, d, B):
    K = 3
    pi, P = _simplex(dev, (B, d), d + B), _simplex(dev, (B, d, d), d + B + 1)
    th = torch.tensor([2.0, 6.5, 8.64], dtype=F64, device=dev)
    b = {'logpdf': _out(dev, (B, K), F64), 'pi': _in(pi), 'P': _in(P), 'thetas': _in(th)}
    _call('mfg_policy_logpdf', b['pi'].ptr(), b['P'].ptr(), B, d, b['thetas'].ptr(), K, 0.05, 1.0, 1.0 + 1e-6, 0.0,
          b['logpdf'].ptr())
    return b, dict(logpdf=_ops().policy_logpdf(pi, P, th, 0.05, 1.0, 1.0 + 1e-6, 0.0), pi=pi, P=P, thetas=th)


def _f_gather_start(dev, d, B):
    mat = _simplex(dev, (NUM_START, d), d)
    g = torch.Generator(device=dev)
    g.manual_seed(d + B)
    idx = torch.randint(NUM_START, (B,), device=dev, generator=g, dtype=I32)
    b = {'pi0': _out(dev, (B, d)), 'mat_pi0': _in(mat), 'idx': _in(idx)}
    _call('mfg_gather_start', b['mat_pi0'].ptr(), NUM_START, b['idx'].ptr(), B, d, b['pi0'].ptr())
    return b, dict(pi0=_ops().gather_start(mat, idx), mat_pi0=mat, idx=idx)


def _f_draw_start(dev, d, B):
    mat = _simplex(dev, (NUM_START, d), d)
    b = {'idx': _out(dev, (B,), I32, fill=-7), 'pi0': _out(dev, (B, d)), 'idx_only': _out(dev, (B,), I32, fill=-7),
         'pi0_only': _out(dev, (B, d)), 'mat_pi0': _in(mat)}
    _call('mfg_draw_start', b['mat_pi0'].ptr(), NUM_START, B, d, 2024, 30, 5, b['idx'].ptr(), b['pi0'].ptr())
    _call('mfg_draw_start', b['mat_pi0'].ptr(), NUM_START, B, d, 2024, 30, 5, b['idx_only'].ptr(), None)
    _call('mfg_draw_start', b['mat_pi0'].ptr(), NUM_START, B, d, 2024, 30, 5, None, b['pi0_only'].ptr())
    idx, pi0 = _ops().draw_start(mat, B, 2024, 30, 5, want_idx=True)
    assert int(idx.min()) >= 0
    return b, dict(idx=idx, pi0=pi0, idx_only=idx, pi0_only=pi0, mat_pi0=mat)


def _f_dirichlet_from_gamma(dev, d, B):
    g = torch.Generator(device=dev)
    g.manual_seed(d + B)
    y = (torch.rand((B, d, d), device=dev, generator=g) * 3.0).contiguous()
    y[0, 0] = 0.0                                              # an all-zero row: uniform
    b = {'P': _out(dev, (B, d, d)), 'y': _in(y)}
    _call('mfg_dirichlet_from_gamma', b['y'].ptr(), B, d, b['P'].ptr())
    return b, dict(P=_ops().dirichlet_from_gamma(y), y=y)


def _f_jsd(dev, d, B):
    p, q = _simplex(dev, (B, d), d + B), _simplex(dev, (B, d), d + B + 1)
    b = {'jsd': _out(dev, (B,), F64), 'p': _in(p), 'q': _in(q)}
    _call('mfg_jsd', b['p'].ptr(), b['q'].ptr(), B, d, b['jsd'].ptr())
    return b, dict(jsd=_ops().jsd(p, q), p=p, q=q)


def _f_backward_value(dev, d, B):
    T = 2
    P = _simplex(dev, (B, T, d, d), d + B)
    b = {'V': _out(dev, (B, T + 1, d), F64), 'l1': _out(dev, (B, T), F64), 'jsd': _out(dev, (B, T), F64), 'P': _in(P)}
    _call('mfg_backward_value', b['P'].ptr(), B, T, d, b['V'].ptr(), b['l1'].ptr(), b['jsd'].ptr())
    V, l1, js = _ops().backward_value(P)
    return b, dict(V=V, l1=l1, jsd=js, P=P)


LAUNCH_ONCE = {'value': _f_value, 'features': _f_features, 'alpha': _f_alpha, 'score': _f_score, 'policy_logpdf': _f_policy_logpdf,
               'gather_start': _f_gather_start, 'draw_start': _f_draw_start, 'dirichlet_from_gamma': _f_dirichlet_from_gamma,
               'jsd': _f_jsd, 'backward_value': _f_backward_value}


@pytest.mark.parametrize('B', [1, 5, 257])
@pytest.mark.parametrize('d', [1, 21, 64, 65, 512])
@pytest.mark.parametrize('kernel', sorted(LAUNCH_ONCE))
def test_launch_once(dev, kernel, d, B):
    bufs, want = LAUNCH_ONCE[kernel](dev, d, B)
    _verify(bufs, want, 'mfg_%s d=%d B=%d' % (kernel, d, B))


@pytest.mark.parametrize('with_reward_acc', [False, True], ids=['no_reward_acc', 'reward_acc'])
@pytest.mark.parametrize('d', [1, 21, 64, 65, 512])
def test_apply_update(dev, d, with_reward_acc):
    """mfg_apply_update has no batch: one thread per weight.  G is an input; theta and reward_acc are one double each."""
    ops = _ops()
    F = ops.num_features(d)
    G, w0, th0 = _randn64(dev, (F + 3,), d), _randn64(dev, (F,), d + 1), _theta(dev)
    G[F + 2] = 7.0
    acc0 = torch.tensor([-3.25], dtype=F64, device=dev)
    w, th, acc = w0.clone(), th0.clone(), acc0.clone()
    ops.apply_update(G, d, LR_C, LR_A, w, th, acc if with_reward_acc else None)
    b = {'G': _in(G), 'w': _in(w0), 'theta': _in(th0), 'reward_acc': _in(acc0)}
    ops.apply_update(b['G'].t, d, LR_C, LR_A, b['w'].t, b['theta'].t, b['reward_acc'].t if with_reward_acc else None)
    _verify(b, dict(G=G, w=w, theta=th, reward_acc=acc if with_reward_acc else acc0), 'mfg_apply_update d=%d' % d)
    assert not torch.equal(th, th0)


def test_a_device_write_into_a_band_is_seen(dev):
    """The helper on the device (tests/test_guard_bands_host.py shows the rest on the CPU): plain torch indexing one element past
    a guarded output, inside its back band."""
    g = _out(dev, (5,), F32)
    g.t.fill_(0.0)
    g.check('untouched')
    g.raw[g.end:g.end + 4] = 0
    with pytest.raises(AssertionError, match=r'back band changed, bytes \+0 \.\. \+3 '):
        g.check('out')


# ---------------------------------------------------------------------------------------------------
# G. calls with an advertised workspace
# ---------------------------------------------------------------------------------------------------
class _Alloc:
    """The buffers of one call, plain (fresh exact-size tensors) or guarded.  The two modes pre-fill an output DIFFERENTLY (plain:
    12345, guarded: NaN / -7), so an element neither call wrote fails the bit-for-bit comparison too; `keep` is a fill both
    modes share, for outputs of which the call leaves a part alone on purpose."""

    def __init__(self, dev, guarded):
        self.dev, self.guarded, self.bufs, self.t = dev, guarded, {}, {}

    def _put(self, name, g):
        self.bufs[name] = g
        self.t[name] = g.t
        return g.t

    def inp(self, name, data):
        """An input, or an in/out buffer that starts from `data`."""
        if self.guarded:
            return self._put(name, _in(data))
        self.t[name] = data.clone()
        return self.t[name]

    def out(self, name, shape, dtype=F32, keep=None):
        fill = keep if keep is not None else ((NAN if dtype.is_floating_point else -7) if self.guarded else 12345)
        if self.guarded:
            return self._put(name, _out(self.dev, shape, dtype, fill=fill))
        self.t[name] = torch.full(shape, fill, dtype=dtype, device=self.dev)
        return self.t[name]

    def ws(self, name, nbytes, zero=False, dtype=U8, shape=None):
        """Exactly the advertised bytes (guarded: with the bands right behind them); its contents are not compared."""
        if self.guarded:
            g = _ws(self.dev, nbytes, dtype, zero)
            self.bufs[name] = g
            t = g.t
        else:
            t = torch.zeros(nbytes // torch.empty(0, dtype=dtype).element_size(), dtype=dtype, device=self.dev)
        return t if shape is None else t.view(shape)


def _pair(dev, fn, ctx, nan_ok=()):
    """fn(alloc) issues the call on buffers from `alloc`: once plain, once guarded; then the three assertions (an output named
    in nan_ok may hold NaN by its contract: it is compared bit for bit only)."""
    plain, g = _Alloc(dev, False), _Alloc(dev, True)
    fn(plain)
    fn(g)
    torch.cuda.synchronize()
    check_all(*[('%s %s' % (ctx, name), b) for name, b in g.bufs.items()])
    assert set(plain.t) == set(g.t)
    for name, ref in plain.t.items():
        got = g.t[name]
        if got.dtype.is_floating_point and name not in nan_ok:
            assert not bool(torch.isnan(got).any()), '%s %s: an element still holds its NaN fill' % (ctx, name)
        assert _same(got, ref), '%s %s: differs from the plain call' % (ctx, name)
    return plain.t


def _policies(a, K):
    """thetas, shifts, alpha_scales (fp64 [K]) and seeds (int64 [K]) of K policies; two of them share a seed."""
    dev = a.dev
    seeds = torch.arange(K, dtype=I64, device=dev) * 7919 + (1 << 33)
    if K > 1:
        seeds[1] = seeds[0]
    return (a.inp('thetas', torch.linspace(6.5, 9.5, K, dtype=F64, device=dev)),
            a.inp('shifts', torch.linspace(0.1, 0.3, K, dtype=F64, device=dev)),
            a.inp('alpha_scales', torch.linspace(9000.0, 13000.0, K, dtype=F64, device=dev)), a.inp('seeds', seeds))


def _prec(precision):
    return _L().PRECISIONS[precision]


@pytest.mark.parametrize('want_traj', [False, True], ids=['traj_in_ws', 'traj'])
@pytest.mark.parametrize('d,precision,K,R', [(21, 'mixed', 3, 3), (15, 'f64', 1, 1)])
def test_evaluate_pop(dev, d, precision, K, R, want_traj):
    N, Lr = 5, 6
    emp = _simplex(dev, (N, Lr, d), 10 + d)
    nbytes = int(_L().lib().mfg_evaluate_pop_workspace_bytes(N, Lr, d, K, R, int(want_traj)))

    def fn(a):
        e32, e64 = a.inp('emp32', emp), a.inp('emp64', emp.double())
        th, sh, al, sd = _policies(a, K)
        metrics = a.out('metrics', (K, 8), F64)
        traj = a.out('traj', (K, N * R, Lr, d)) if want_traj else None
        ws = a.ws('ws', nbytes)
        _call('mfg_evaluate_pop', e32.data_ptr(), e64.data_ptr(), N, Lr, d, K, th.data_ptr(), sh.data_ptr(), al.data_ptr(),
              sd.data_ptr(), 37, R, _prec(precision), metrics.data_ptr(), None if traj is None else traj.data_ptr(),
              ws.data_ptr(), nbytes)

    _pair(dev, fn, 'evaluate_pop d=%d' % d)


@pytest.mark.parametrize('want_traj', [False, True], ids=['traj_in_ws', 'traj'])
@pytest.mark.parametrize('R', [3, 65])
def test_forecast_pop(dev, R, want_traj):
    """R = 3 and 65: the sort of the order statistics pads the members to 4 and 128."""
    d, K, N, H = 21, 2, 2, 4
    emp = _simplex(dev, (N, H, d), 100 + R)
    ranks = (0, R - 1, R // 2)
    nbytes = int(_L().lib().mfg_forecast_pop_workspace_bytes(N, H, d, K, R, int(want_traj)))

    def fn(a):
        s32, e32, e64 = a.inp('start32', emp[:, 0].contiguous()), a.inp('emp32', emp), a.inp('emp64', emp.double())
        th, sh, al, sd = _policies(a, K)
        mean, std = a.out('mean', (K, N, H, d), F64), a.out('std', (K, N, H, d), F64)
        quant, curves = a.out('quant', (K, N, H, len(ranks), d)), a.out('curves', (K, H, 4), F64)
        traj = a.out('traj', (K, N * R, H, d)) if want_traj else None
        ws = a.ws('ws', nbytes)
        _call('mfg_forecast_pop', s32.data_ptr(), N, H, d, K, th.data_ptr(), sh.data_ptr(), al.data_ptr(), sd.data_ptr(), 37, R,
              _prec('mixed'), (C.c_int32 * len(ranks))(*ranks), len(ranks), e32.data_ptr(), e64.data_ptr(), mean.data_ptr(),
              std.data_ptr(), quant.data_ptr(), curves.data_ptr(), None if traj is None else traj.data_ptr(), ws.data_ptr(),
              nbytes)

    _pair(dev, fn, 'forecast_pop R=%d' % R)


@pytest.mark.parametrize('energy', [False, True], ids=['no_energy', 'energy'])
@pytest.mark.parametrize('R', [3, 65, 130])
def test_forecast_score(dev, R, energy):
    """R = 130 is past two tiles of MFG_FORECAST_SCORE_TILE = 64 members.  Without `energy` the summary's second column is NaN
    by contract."""
    d, K, N, H = 15, 2, 2, 3
    traj0, emp = _simplex(dev, (K, N * R, H, d), 200 + R), _simplex(dev, (N, H, d), 300 + R)
    nbytes = int(_L().lib().mfg_forecast_score_workspace_bytes(N, H, d, K, R))

    def fn(a):
        traj, e32, e64 = a.inp('traj', traj0), a.inp('emp32', emp), a.inp('emp64', emp.double())
        crps, less, equal = a.out('crps', (K, N, H, d), F64), a.out('less', (K, N, H, d), I32), a.out('equal', (K, N, H, d), I32)
        en = a.out('energy', (K, N, H), F64) if energy else None
        summary = a.out('summary', (K, H, 2), F64)
        ws = a.ws('ws', nbytes)
        _call('mfg_forecast_score', traj.data_ptr(), N, H, d, K, R, e32.data_ptr(), e64.data_ptr(), crps.data_ptr(),
              less.data_ptr(), equal.data_ptr(), None if en is None else en.data_ptr(), summary.data_ptr(), ws.data_ptr(), nbytes)

    out = _pair(dev, fn, 'forecast_score R=%d' % R, nan_ok=() if energy else ('summary',))
    assert not bool(torch.isnan(out['summary'][..., 0]).any())
    assert int(out['less'].min()) >= 0 and int(out['equal'].min()) >= 0


@pytest.mark.parametrize('given', [True, False], ids=['steps_V', 'metrics_only'])
def test_consistency_given(dev, given):
    """With `steps` the advertised workspace is 0 bytes; without, the per-hour values live in it."""
    K, M, T, d = 2, 3, 2, 7
    P0 = _simplex(dev, (K, M, T, d, d), 400)
    nbytes = int(_L().lib().mfg_consistency_given_workspace_bytes(K, M, T, int(given)))
    assert (nbytes == 0) == given

    def fn(a):
        P = a.inp('P', P0)
        metrics = a.out('metrics', (K, 4), F64)
        steps = a.out('steps', (K, M, T, 2), F64) if given else None
        V = a.out('V', (K, M, T + 1, d), F64) if given else None
        ws = a.ws('ws', nbytes)
        _call('mfg_consistency_given', P.data_ptr(), K, M, T, d, metrics.data_ptr(), None if steps is None else steps.data_ptr(),
              None if V is None else V.data_ptr(), ws.data_ptr() if nbytes else None, nbytes)

    _pair(dev, fn, 'consistency_given')


@pytest.mark.parametrize('given', [True, False], ids=['all_outputs', 'metrics_only'])
@pytest.mark.parametrize('d,precision', [(15, 'mixed'), (21, 'f64')])
def test_consistency_pop(dev, d, precision, given):
    K, N, H, R = 2, 3, 3, 2
    NR, T = N * R, H - 1
    start = _simplex(dev, (N, d), 500 + d)
    nbytes = int(_L().lib().mfg_consistency_pop_workspace_bytes(N, H, d, K, R, int(given), int(given), int(given)))

    def fn(a):
        s32 = a.inp('start32', start)
        th, sh, al, sd = _policies(a, K)
        metrics = a.out('metrics', (K, 4), F64)
        opt = [None] * 4
        if given:
            opt = [a.out('steps', (K, NR, T, 2), F64), a.out('V', (K, NR, H, d), F64), a.out('actions', (K, NR, T, d, d)),
                   a.out('traj', (K, NR, H, d))]
        ws = a.ws('ws', nbytes)
        _call('mfg_consistency_pop', s32.data_ptr(), N, H, d, K, th.data_ptr(), sh.data_ptr(), al.data_ptr(), sd.data_ptr(), 37, R,
              _prec(precision), metrics.data_ptr(), *[None if t is None else t.data_ptr() for t in opt], ws.data_ptr(), nbytes)

    _pair(dev, fn, 'consistency_pop d=%d' % d)


@pytest.mark.parametrize('K,N,d', [(2, 37, 21), (1, 1, 15), (3, 300, 64)])
def test_action_mean_pop(dev, K, N, d):
    act = _simplex(dev, (K, N, d, d), 600 + d)
    nbytes = int(_L().lib().mfg_action_mean_pop_workspace_bytes(K, N, d))

    def fn(a):
        action, mean, ws = a.inp('action', act), a.out('mean', (K, d, d), F64), a.ws('ws', nbytes)
        _call('mfg_action_mean_pop', action.data_ptr(), N * d * d, K, N, d, mean.data_ptr(), ws.data_ptr(), nbytes)

    _pair(dev, fn, 'action_mean_pop K=%d N=%d d=%d' % (K, N, d))


@pytest.mark.parametrize('N', [1, 257])
@pytest.mark.parametrize('G', [0, 1, 200])
@pytest.mark.parametrize('bins', [1, 1024])
def test_row_distribution(dev, bins, G, N):
    """Rows `stride` = N + 3 apart: the gap holds the band's pattern.  One value has no variance (ddof 1) and no KDE: moments and
    density may hold NaN by contract."""
    R, stride = 3, N + 3
    vals = _randn64(dev, (R, stride), 700 + N).float()
    nbytes = int(_L().lib().mfg_row_distribution_workspace_bytes(R, N, bins, G))

    def fn(a):
        v = a.inp('values', vals)
        moments, counts = a.out('moments', (R, 6), F64), a.out('counts', (R, bins), I64)
        edges, status = a.out('edges', (R, bins + 1), F64), a.out('status', (R,), I32)
        density = a.out('density', (R, G), F64) if G else None
        ws = a.ws('ws', nbytes)
        _call('mfg_row_distribution', v.data_ptr(), R, N, stride, bins, 0, 0.0, 0.0, G, -3.0, 3.0, moments.data_ptr(),
              counts.data_ptr(), edges.data_ptr(), None if density is None else density.data_ptr(), status.data_ptr(),
              ws.data_ptr() if nbytes else None, nbytes)

    out = _pair(dev, fn, 'row_distribution bins=%d G=%d N=%d' % (bins, G, N), nan_ok=('moments', 'density') if N == 1 else ())
    assert int(out['counts'].sum()) == R * N and int(out['status'].min()) >= 0


@pytest.mark.parametrize('per_learner', [False, True], ids=['shared_store', 'store_per_learner'])
def test_traj_log_z_pop(dev, per_learner):
    """The scratch has exactly 4 n_rows bytes; the row list skips rows, so the other log_z rows must keep their fill (7)."""
    K, cap, T, d, n_pol = 2, 6, 3, 15, 2
    lead = (K,) if per_learner else ()
    st0, ac0 = _simplex(dev, lead + (cap, T, d), 800), _simplex(dev, lead + (cap, T, d, d), 801)
    rows = [4, 0, 2]

    def fn(a):
        state, action = a.inp('state', st0), a.inp('action', ac0)
        th = a.inp('thetas', torch.tensor([[7.9, 8.5], [8.8, 8.1]], dtype=F64, device=dev))
        sh = a.inp('shifts', torch.tensor([0.05, -0.02], dtype=F64, device=dev))
        log_z = a.out('log_z', (K, cap), F64, keep=7.0)
        _ops().traj_log_z_pop(state, action, rows, th, sh, float(np.log(9.0)), out=log_z,
                              scratch=a.ws('scratch', 4 * len(rows), dtype=I32))

    out = _pair(dev, fn, 'traj_log_z_pop')
    rest = sorted(set(range(cap)) - set(rows))
    assert bool((out['log_z'][:, rest] == 7.0).all()) and not bool((out['log_z'][:, rows] == 7.0).any())


def _forward_cases():
    """One shape per family of oracle/reward_forward_cases.py (tests/test_reward_forward_cases.py), and one per kernel."""
    from oracle import reward_forward_cases as FC
    picked = {}
    for fam in FC.FAMILIES:
        c = FC.by_family(fam)[0]
        picked[c.name] = c
    for c in FC.CASES:
        if FC.kernel_of(c) not in {FC.kernel_of(p) for p in picked.values()}:
            picked[c.name] = c
    return list(picked.values())


@pytest.mark.parametrize('case', _forward_cases(), ids=[c.name for c in _forward_cases()])
def test_reward_net_forward(dev, case):
    from oracle import reward_forward_cases as FC
    net, state, action = FC.build(case, dev)
    s0, a0 = torch.as_tensor(state, device=dev), torch.as_tensor(action, device=dev)
    B, d = s0.shape
    dropout = 'dropout' in case.reg
    seed, off = FC.dropout_key(case)
    prm = [net.conv1.weight, net.conv1.bias, net.conv2.weight, net.conv2.bias, net.fc3.weight, net.fc3.bias, net.fc4.weight,
           net.fc4.bias, net.out.weight, net.out.bias]
    want = _ops().reward_net_forward(net, s0, a0, dropout=dropout, seed=seed, sample_offset=off)
    b = {'reward': _out(dev, (B,)), 'state': _in(s0), 'action': _in(a0)}
    b.update({'param%d' % i: _in(p.detach()) for i, p in enumerate(prm)})
    _call('mfg_reward_net_forward', b['state'].ptr(), b['action'].ptr(), B, d, net.conv1.kernel_size[0], net.conv2.out_channels,
          net.conv2.kernel_size[0], net.fc3.out_features, net.fc4.out_features, *[b['param%d' % i].ptr() for i in range(10)],
          float(net.keep_prob) if dropout else 1.0, seed, off, b['reward'].ptr())
    want_all = {'reward': want, 'state': s0, 'action': a0}
    want_all.update({'param%d' % i: p.detach() for i, p in enumerate(prm)})
    _verify(b, want_all, 'reward_net_forward %s (%s)' % (case.name, FC.kernel_of(case)))


@pytest.mark.parametrize('d', [21, 15])
def test_reward_net_forward_pop(dev, d):
    """Learners 2 and 0 of K = 3 listed: row 1 of the rewards keeps its fill; the scratch has exactly 16 n bytes."""
    from oracle.reward_train_cases import _net
    ops = _ops()
    K, N = 3, 37
    net = _net(d, 'dropout_l1l2', 8, 4, dev)
    st = ops.reward_net_struct(net)
    s0, a0 = _simplex(dev, (N, d), 900 + d), _simplex(dev, (N, d, d), 901 + d)

    def fn(a):
        ops.reward_net_forward_pop(st, False, K, a.inp('state', s0), a.inp('action', a0), [2, 0], [77, 1 << 40],
                                   out=a.out('reward', (K, N), keep=7.0), scratch=a.ws('scratch', 16 * 2))

    out = _pair(dev, fn, 'reward_net_forward_pop d=%d' % d)
    assert bool((out['reward'][1] == 7.0).all()) and not bool((out['reward'][[0, 2]] == 7.0).any())


@pytest.mark.parametrize('d,n3,n4,batch', [(21, 16, 4, (5, 5, 15)), (15, 8, 32, (3, 9, 4))])
def test_reward_net_train_steps_pop(dev, d, n3, n4, batch):
    """Parameters, Adam moments and stats guarded; learner 1 of K = 3 has no entry and keeps all of its rows.  The workspace is
    n_active slices of mfg_reward_net_train_workspace_bytes rounded up to 256, plan_dev exactly the plan's bytes."""
    ops, lib = _ops(), _L().lib()
    nd, ng, T = batch
    K, U, active = 3, 2, [2, 0]
    dims = (d, 5, 2, 3, n3, n4)
    NP = int(lib.mfg_reward_net_num_params(*dims))
    ld = (NP + 63) // 64 * 64
    g = torch.Generator(device=dev)
    g.manual_seed(d)
    p0 = (torch.rand(K, ld, device=dev, generator=g) - 0.5) * 0.4
    m0, v0 = torch.rand(K, ld, device=dev, generator=g) * 1e-3, torch.rand(K, ld, device=dev, generator=g) * 1e-6
    rows = 11
    demo = (_simplex(dev, (rows, T, d), d + 1), _simplex(dev, (rows, T, d, d), d + 2))
    gen = (_simplex(dev, (K, rows, T, d), d + 3), _simplex(dev, (K, rows, T, d, d), d + 4))
    slice_bytes = (int(lib.mfg_reward_net_train_workspace_bytes(*dims, (nd + ng) * T)) + 255) // 256 * 256

    def fn(a):
        plan = ops.rn_train_plan(U * len(active))
        for u in range(U):
            for s, k in enumerate(active):
                e = plan[u * len(active) + s]
                e['learner'], e['key'], e['lr'], e['adam_step'] = k, 1000 * u + k + (1 << 35), 2e-3, u + 1
                e['demo_rows'][:nd] = [(3 * j + u) % rows for j in range(nd)]
                e['gen_rows'][:ng] = [(rows - 1 - j - u) % rows for j in range(ng)]
        ops.reward_net_train_steps_pop(a.inp('params', p0), a.inp('adam_m', m0), a.inp('adam_v', v0), ld, K, dims,
                                       (a.inp('demo_state', demo[0]), a.inp('demo_action', demo[1])),
                                       (a.inp('gen_state', gen[0]), a.inp('gen_action', gen[1])), plan, U, len(active), nd, ng, T,
                                       5, 0.4, True, a.out('stats', (K, 4), keep=7.0), a.ws('ws', len(active) * slice_bytes),
                                       a.ws('plan_dev', plan.nbytes))

    out = _pair(dev, fn, 'reward_net_train_steps_pop d=%d' % d)
    assert torch.equal(out['params'][1], p0[1]) and torch.equal(out['adam_m'][1], m0[1]) and bool((out['stats'][1] == 7.0).all())
    assert not torch.equal(out['params'][0, :NP], p0[0, :NP]) and not torch.equal(out['params'][2, :NP], p0[2, :NP])


@pytest.mark.parametrize('d', [21, 15])
@pytest.mark.parametrize('entry', ['train_episodes_pop', 'train_episodes_pop_resident', 'train_rollouts_pop'])
def test_population_training(dev, entry, d):
    """K = 3 learners of B = 13 trajectories, T = 2, two episodes: theta [K], w [K, F], G [K, F + 3], reward_acc [K, E] and every
    per-learner output guarded; the workspace is K slices of ops.pop_workspace_slice(B, d, T), zeroed once."""
    ops = _ops()
    K, B, T, E = 3, 13, 2, 2
    F = ops.num_features(d)
    sb = ops.pop_workspace_slice(B, d, T)
    if entry == 'train_episodes_pop_resident':
        assert _L().lib().mfg_pop_resident_supported(d, B, 0) == 1
    mat = _simplex(dev, (NUM_START, d), 950 + d)
    w0 = _randn64(dev, (K, F), d).abs_() * 0.1

    def fn(a):
        th, sh, al, sd = _policies(a, K)
        w, G, acc = a.inp('w', w0), a.out('G', (K, F + 3), F64), a.inp('reward_acc', torch.zeros(K, E, dtype=F64, device=dev))
        lrc = a.inp('lr_critic', torch.linspace(0.05, 0.15, K, dtype=F64, device=dev))
        lra = a.inp('lr_actor', torch.linspace(5e-4, 2e-3, K, dtype=F64, device=dev))
        ws = a.ws('ws', K * sb, zero=True, dtype=F64, shape=(K, sb // 8))
        m = a.inp('mat_pi0', mat)
        if entry == 'train_rollouts_pop':
            bufs = dict(pi_traj=a.out('pi_traj', (K, B, T + 1, d)), pi_last=a.out('pi_last', (K, B, d)),
                        reward=a.out('reward', (K, B, T)), delta=a.out('delta', (K, B, T), F64), g=a.out('g', (K, B, T), F64))
            ops.train_rollouts_pop(m, T, E, 0, 0, th, sh, al, w, 1.0, G, ws, bufs, lrc, lra, sd, reward_acc=acc)
        else:
            pi = a.out('pi', (K, B, d))
            # (pi_scratch is scratch by contract, like the workspace: its bands are checked, its contents are not compared)
            bufs = dict(scratch=a.ws('scratch', K * B * d * 4, dtype=F32, shape=(K, B, d)), reward=a.out('reward', (K, B)), delta=a.out('delta', (K, B), F64),
                        g=a.out('g', (K, B), F64))
            getattr(ops, entry)(m, pi, T, E, 0, 0, th, sh, al, w, 1.0, lrc, lra, sd, G, ws, bufs, reward_acc=acc)

    out = _pair(dev, fn, '%s d=%d' % (entry, d))
    assert not torch.equal(out['w'], w0) and bool((out['reward_acc'] != 0).all())
