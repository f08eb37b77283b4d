"""-m gpu: every entry point that reads or writes an action slab, on an operand past 2^31 elements and 8 GiB.

The rest of the suite stays below 2^29 floats.  Here one allocation of large_buffers.SLAB_FLOATS = 2^31 + 2^25 floats (8.72 GB) is
viewed per case as the [B, d, d] (or [B, T, d, d]) operand of the entry point, so that the 2 GiB, 4 GiB and 8 GiB byte offsets
and the 2^31-th element lie inside it, with many tiles and super tiles wholly past the last of them.  Every element of every
output gets two kinds of evidence:

  * the whole output, bit for bit (torch.equal), against calls of the SAME entry point on large_buffers.chunks -- ranges of
    less than 2^28 floats with rebased pointers and traj_offset / sample offset advanced by the range's start, i.e. calls
    inside the address range the other modules cover.  Outputs are pre-filled with NaN (floats) or -7 (ints): an element
    nobody wrote fails the comparison.  The batch sums G re-associate by construction and are held to the tolerance of
    test_gpu_fullsize.py::test_fullsize_split_invariance (1e-9 relative over clamp_min(1e-6));
  * the items of large_buffers.boundary_windows (first, last, and round float offsets 2^29, 2^30, 2^31) against the fp64 / NumPy
    reference of the operation, with the assertions of that operation's small-shape test, cited where they are used.

CASES lists every case; tests/test_large_buffers_host.py checks the table and the index arithmetic without a GPU.  Each test
prints (-s) its B, its bytes, the window positions, the worst error against its bound per window, and its wall time.

Memory: the slab, plus at most 18 GiB per test (group D: a second slab, or an fp64 output of 17.2 GB), freed before the test
returns.
"""
import ctypes as C
import time

import numpy as np
import pytest

torch = pytest.importorskip('torch')

import large_buffers as LB

pytestmark = pytest.mark.gpu

THETA, SHIFT, SCALE = 8.86349, 0.16, 12000.0          # the `policy` regime of oracle.score_ref.regime_case
GAMMA = 0.9
NAN = float('nan')


def _case(id, group, entry, d, per_item, tile, **extra):
    c = dict(id=id, group=group, entry=entry, d=d, per_item=per_item, tile=tile, W=LB.window_items(per_item), halves=False)
    c.update(extra)
    return c


# per_item: floats of one item of the large operand; tile: the items the kernel takes together (the batch is ragged against it);
# W: items per window; halves: the batch is split into two equal groups (K = 2), the crossing of 2^31 inside the second
CASES = [
    # ---- A. given actions [B, d, d]
    _case('step-d21', 'A', 'mfg_step_given_P', 21, 441, 12),                 # k_step_wave_batched + the ragged tail launch
    _case('step-d15', 'A', 'mfg_step_given_P', 15, 225, 4),
    _case('step-d40', 'A', 'mfg_step_given_P', 40, 1600, 4),                 # k_step_small
    _case('step-d100', 'A', 'mfg_step_given_P', 100, 10000, 4),              # k_step_large
    _case('step-d128', 'A', 'mfg_step_given_P', 128, 16384, 8),              # k_step_rows
    _case('step-d256', 'A', 'mfg_step_given_P', 256, 65536, 8),
    _case('step-d21-unaligned', 'A', 'mfg_step_given_P', 21, 441, 12, offset=1),   # k_step_small_unaligned
    _case('score-d21-f64', 'A', 'mfg_score+mfg_td_pg_accumulate', 21, 441, 12, precision='f64'),
    _case('score-d21-mixed', 'A', 'mfg_score+mfg_td_pg_accumulate', 21, 441, 12, precision='mixed'),
    _case('score-d128-mixed', 'A', 'mfg_score+mfg_td_pg_accumulate', 128, 16384, 4, precision='mixed'),
    _case('logpdf-d21-K2', 'A', 'mfg_policy_logpdf', 21, 441, 4, K=2),
    _case('consistency-d21-T15', 'A', 'mfg_consistency_given', 21, 15 * 441, 4, T=15),
    # ---- B. sampled actions written out
    _case('sample-d21-mixed', 'B', 'mfg_sample_dirichlet', 21, 441, 12, precision='mixed'),
    _case('sample-d21-f64', 'B', 'mfg_sample_dirichlet', 21, 441, 12, precision='f64'),
    _case('sample-d128-mixed', 'B', 'mfg_sample_dirichlet', 128, 16384, 4, precision='mixed'),
    _case('rollout-d21-T15', 'B', 'mfg_rollout', 21, 15 * 441, 12, T=15),
    _case('rollout-d128-T3', 'B', 'mfg_rollout', 128, 3 * 16384, 4, T=3),
    # ---- C. consumers of stored actions
    _case('reward-net-d21', 'C', 'mfg_reward_net_forward', 21, 441, 8, dropout=False),
    _case('reward-net-d21-dropout', 'C', 'mfg_reward_net_forward', 21, 441, 8, dropout=True),
    _case('logz-d21-K1-shared', 'C', 'mfg_traj_log_z_pop', 21, 15 * 441, 1, T=15, K=1, W=8),
    _case('logz-d21-K2-per-learner', 'C', 'mfg_traj_log_z_pop', 21, 15 * 441, 1, T=15, K=2, W=8, halves=True),
    _case('agents-d21-K2', 'C', 'mfg_agents_step_pop', 21, 441, 1, K=2, halves=True),
    # ---- D. elementwise helpers (two-buffer budget)
    _case('alpha-d21', 'D', 'mfg_alpha', 21, 441, 256),
    _case('dirichlet-from-gamma-d21', 'D', 'mfg_dirichlet_from_gamma', 21, 441, 4),
    _case('features-d21', 'D', 'mfg_features', 21, 253, 256),
]


def case_batch(c):
    """Items of a case's large operand (for `halves`: of both groups together)."""
    B = LB.batch_for(c['per_item'], c['tile'])
    return 2 * (B // 2) if c['halves'] else B


def _by(entry):
    cs = [c for c in CASES if c['entry'] == entry]
    return dict(argvalues=cs, ids=[c['id'] for c in cs])


# ---------------------------------------------------------------------------------------------------- fixtures and plumbing
class Slab:
    """The one large allocation (4 floats longer than SLAB_FLOATS: the misaligned view) and what its front currently holds."""

    def __init__(self, dev):
        LB.require_free(4 * (LB.SLAB_FLOATS + 4))
        self.t = torch.empty(LB.SLAB_FLOATS + 4, dtype=torch.float32, device=dev)
        assert self.t.data_ptr() % 16 == 0
        self.tag = None

    def rows(self, d, n, offset=0):
        """The flat view [offset, offset + n) holding row-stochastic rows of d floats (filled once per (d, n, offset))."""
        v = self.t[offset:offset + n]
        if self.tag != (d, n, offset):
            LB.fill_rows_(v, d, seed=1000 + d)
            self.tag = (d, n, offset)
        return v

    def output(self, n):
        """The flat view [0, n) as an output: every float NaN."""
        self.tag = None
        v = self.t[:n]
        v.fill_(NAN)
        return v


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.fail('-m gpu tests need a GPU: the HIP path has no CPU fallback')
    from discrete_mean_field_game_amd import ops
    ops.init()
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def slab(dev):
    s = Slab(dev)
    yield s
    del s.t
    torch.cuda.empty_cache()


@pytest.fixture(autouse=True)
def _auto_mapping_and_clean_status():
    yield
    from discrete_mean_field_game_amd import _lib as L, ops
    L.lib().mfg_set_core_mapping(0)
    ops.clear_status()
    torch.cuda.empty_cache()


@pytest.fixture(autouse=True)
def _whole_test_wall_time(request, slab):
    """The case's wall time with its fill and its input states (Report.done prints the part behind them)."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    yield
    torch.cuda.synchronize()
    print('\n[large] %-26s   wall time of the whole test %.2f s' % (request.node.callspec.params['c']['id'], time.perf_counter() - t0), end='')


def _O():
    from oracle import mfg_oracle
    return mfg_oracle


def _call(name, *args):
    """One C ABI call on torch's current stream (as tests/test_gpu_launch_once_kernels.py::_call): the tests hand in the
    sentinel-filled outputs themselves."""
    from discrete_mean_field_game_amd import _lib as L
    L.check(getattr(L.lib(), name)(*args, torch.cuda.current_stream().cuda_stream), name)


def _ptr(t, lo=0):
    """Address of item lo of a contiguous tensor (None -> NULL)."""
    if t is None:
        return None
    return t.data_ptr() + lo * (t.stride(0) if t.dim() else 1) * t.element_size()


def _nan(shape, dev, dtype=torch.float32):
    return torch.full(shape, NAN, dtype=dtype, device=dev)


def _dirichlet_states(B, d, dev, seed):
    """[B, d] fp32 Dirichlet(1) rows, drawn on the device (start_states of tests/test_gpu_fullsize.py)."""
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    x = -torch.log(torch.rand(B, d, device=dev, generator=g).clamp_min(1e-12))
    return (x / x.sum(1, keepdim=True)).float().contiguous()


def _uniform_states(B, d, dev, seed):
    """[B, d] fp32 rows rand / sum (the states of test_given_P_batched_store_kernel_equals_per_tile_kernel)."""
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    pi = torch.rand(B, d, device=dev, generator=g)
    return (pi / pi.sum(1, keepdim=True)).contiguous()


def _windows(c, B, dev):
    wins = LB.boundary_windows(B, c['per_item'], c['W'])
    idx = LB.window_index(wins)
    return wins, idx, torch.as_tensor(idx, device=dev)


def _host(t, idx_t, dtype=np.float64):
    return t[idx_t].cpu().numpy().astype(dtype)


def _per_window(err, W):
    """Worst entry of `err` (first axis: the items of the five windows, in order) per window."""
    err = np.asarray(err, dtype=np.float64).reshape(len(err), -1)
    err = np.where(np.isnan(err), np.inf, err)
    return [float(err[k:k + W].max()) for k in range(0, err.shape[0], W)]


class Report:
    def __init__(self, c, B, nbytes, wins):
        self.c, self.t0 = c, time.perf_counter()
        print('\n[large] %-26s %-32s B = %d, %.3f GB, windows at %s' % (
            c['id'], c['entry'], B, nbytes / 1e9, ' '.join('%d..%d' % (w.start, w.stop - 1) for w in wins)), end='')

    def line(self, what, worst, bound):
        worst = worst if isinstance(worst, (list, tuple)) else [worst]
        print('\n[large] %-26s   %-28s worst per window %s  bound %.3g' % (
            self.c['id'], what, ' '.join('%.3g' % v for v in worst), bound), end='')

    def done(self):
        torch.cuda.synchronize()
        print('\n[large] %-26s   wall time of the calls and checks %.2f s' % (self.c['id'], time.perf_counter() - self.t0), end='')


def _same(whole, part, lo, hi, what):
    assert torch.equal(whole[lo:hi], part[:hi - lo]), '%s: items %d..%d of the whole call differ from the chunk call' % (what, lo, hi - 1)


def _split_sums_agree(Gsum, G):
    """The tolerance of test_gpu_fullsize.py::test_fullsize_split_invariance."""
    worst = float(((Gsum - G).abs() / G.abs().clamp_min(1e-6)).max())
    assert worst < 1e-9, worst
    return worst


# ---------------------------------------------------------------------------------------------------- A. mfg_step_given_P
@pytest.mark.parametrize('c', **_by('mfg_step_given_P'))
def test_step_given_P(dev, slab, c):
    O = _O()
    d, off = c['d'], c.get('offset', 0)
    dd = d * d
    B = case_batch(c)
    P = slab.rows(d, B * dd, off).view(B, d, d)
    assert P.data_ptr() % 16 == 4 * off
    pi = _uniform_states(B, d, dev, 7 + d)
    wins, idx, idx_t = _windows(c, B, dev)
    rep = Report(c, B, 4 * B * dd, wins)
    Pw, piw = _host(P, idx_t), _host(pi, idx_t)
    cks = LB.chunks(B, dd)
    nmax = max(hi - lo for lo, hi in cks)
    pn_c, r_c = _nan((nmax, d), dev), _nan((nmax,), dev)
    for kind in (0, 1):
        pn, r = _nan((B, d), dev), _nan((B,), dev)
        _call('mfg_step_given_P', pi.data_ptr(), P.data_ptr(), B, d, kind, pn.data_ptr(), r.data_ptr())
        for lo, hi in cks:
            pn_c.fill_(NAN), r_c.fill_(NAN)
            _call('mfg_step_given_P', _ptr(pi, lo), _ptr(P, lo), hi - lo, d, kind, pn_c.data_ptr(), r_c.data_ptr())
            _same(pn, pn_c, lo, hi, "pi' (kind %d)" % kind)
            _same(r, r_c, lo, hi, 'reward (kind %d)' % kind)
        # the assertions of test_given_P_batched_store_kernel_equals_per_tile_kernel (pi' bit exact, reward kind 0 to 1e-6) and,
        # for the synthetic reward, of test_fullsize_transition_linearity_and_reward_kinds (1e-6 over clamp_min(1e-6))
        ref_pn = O.transition(Pw, piw).astype(np.float32)
        got_pn, got_r = pn[idx_t].cpu().numpy(), r[idx_t].cpu().numpy()
        ref_r = O.calc_reward(Pw, piw) if kind == 0 else O.calc_reward_synthetic(Pw, piw)
        rel = np.abs(got_r - ref_r) / np.maximum(np.abs(ref_r), 1e-6)
        rep.line("kind %d pi' elements differing" % kind, _per_window((got_pn != ref_pn).sum(-1), c['W']), 0)
        rep.line('kind %d reward rel err' % kind, _per_window(rel, c['W']), 1e-6)
        assert np.array_equal(got_pn, ref_pn)
        assert np.max(np.where(np.isnan(rel), np.inf, rel)) < 1e-6
        del pn, r
    rep.done()


# ---------------------------------------------------------------------------------------------------- A. mfg_score, mfg_td_pg_accumulate
@pytest.mark.parametrize('c', **_by('mfg_score+mfg_td_pg_accumulate'))
def test_score_and_td_pg_accumulate(dev, slab, c):
    from discrete_mean_field_game_amd import _lib as L, ops
    from oracle import score_ref as S
    O = _O()
    d, precision = c['d'], c['precision']
    dd, prec = d * d, L.PRECISIONS[c['precision']]
    B = case_batch(c)
    P = slab.rows(d, B * dd).view(B, d, d)
    pi = _dirichlet_states(B, d, dev, 11 + d)
    wins, idx, idx_t = _windows(c, B, dev)
    rep = Report(c, B, 4 * B * dd, wins)
    theta = torch.tensor([THETA], dtype=torch.float64, device=dev)
    F = ops.num_features(d)
    w = torch.as_tensor(np.random.RandomState(1).rand(F), device=dev)          # (the weights of test_gpu_fullsize.py::full_rollout)
    pn, r = ops.step_given_P(pi, P)
    nws = int(L.lib().mfg_workspace_bytes(B, d))
    ws = torch.zeros(max(nws, 8) // 8, dtype=torch.float64, device=dev)
    ops.clear_status()
    g1, dl, g2 = _nan((B,), dev, torch.float64), _nan((B,), dev, torch.float64), _nan((B,), dev, torch.float64)
    G = torch.zeros(F + 3, dtype=torch.float64, device=dev)
    _call('mfg_score', pi.data_ptr(), P.data_ptr(), B, d, theta.data_ptr(), SHIFT, prec, g1.data_ptr())
    _call('mfg_td_pg_accumulate', pi.data_ptr(), pn.data_ptr(), P.data_ptr(), r.data_ptr(), w.data_ptr(), theta.data_ptr(), SHIFT,
          GAMMA, B, d, prec, dl.data_ptr(), g2.data_ptr(), G.data_ptr(), 0, ws.data_ptr(), nws)
    cks = LB.chunks(B, dd)
    nmax = max(hi - lo for lo, hi in cks)
    g1_c, dl_c, g2_c = (_nan((nmax,), dev, torch.float64) for _ in range(3))
    Gsum, G_c = torch.zeros_like(G), torch.zeros_like(G)
    for lo, hi in cks:
        g1_c.fill_(NAN), dl_c.fill_(NAN), g2_c.fill_(NAN)
        _call('mfg_score', _ptr(pi, lo), _ptr(P, lo), hi - lo, d, theta.data_ptr(), SHIFT, prec, g1_c.data_ptr())
        _call('mfg_td_pg_accumulate', _ptr(pi, lo), _ptr(pn, lo), _ptr(P, lo), _ptr(r, lo), w.data_ptr(), theta.data_ptr(), SHIFT,
              GAMMA, hi - lo, d, prec, dl_c.data_ptr(), g2_c.data_ptr(), G_c.data_ptr(), 0, ws.data_ptr(), nws)
        _same(g1, g1_c, lo, hi, 'g of mfg_score')
        _same(dl, dl_c, lo, hi, 'delta')
        _same(g2, g2_c, lo, hi, 'g of mfg_td_pg_accumulate')
        Gsum += G_c
    rep.line('G: chunk sums vs whole', _split_sums_agree(Gsum, G), 1e-9)
    assert ops.status() == 0
    # the assertions of test_gpu_score_regimes.py::test_given_P_score_with_exact_zeros: |g - g_ref| <= score_ref.bound, and delta
    Pw, piw = _host(P, idx_t), _host(pi, idx_t)
    tm = S.terms(piw, Pw, THETA, SHIFT)
    bd = S.bound(piw, Pw, THETA, SHIFT, None, precision, sampled=False, t=tm)
    for tag, g in (('mfg_score', g1), ('mfg_td_pg_accumulate', g2)):
        got = g[idx_t].cpu().numpy()
        assert np.all(np.isfinite(got))
        err = np.abs(got - tm['g'])
        rep.line('%s |g - g_ref| / bound' % tag, _per_window(err / bd, c['W']), 1.0)
        assert np.all(err <= bd), (tag, float(np.max(err / bd)))
    pnw, rw, wh = _host(pn, idx_t), _host(r, idx_t), w.cpu().numpy()
    V, Vn = O.calc_features(piw).dot(wh), O.calc_features(pnw).dot(wh)
    derr = np.abs(dl[idx_t].cpu().numpy() - (rw + GAMMA * Vn - V))
    dbound = 1e-11 * max(1.0, np.abs(V).max())
    rep.line('|delta - delta_ref|', _per_window(derr, c['W']), dbound)
    assert np.max(np.where(np.isnan(derr), np.inf, derr)) < dbound
    rep.done()


# ---------------------------------------------------------------------------------------------------- A. mfg_policy_logpdf
@pytest.mark.parametrize('c', **_by('mfg_policy_logpdf'))
def test_policy_logpdf(dev, slab, c):
    O = _O()
    d, K = c['d'], c['K']
    dd = d * d
    N = case_batch(c)
    P = slab.rows(d, N * dd).view(N, d, d)
    pi = _dirichlet_states(N, d, dev, 13)
    wins, idx, idx_t = _windows(c, N, dev)
    rep = Report(c, N, 4 * N * dd, wins)
    thetas = np.array([6.5, 8.64])[:K]
    th = torch.as_tensor(thetas, device=dev)
    Pw, piw = _host(P, idx_t, np.float32), _host(pi, idx_t, np.float32)
    cks = LB.chunks(N, dd)
    nmax = max(hi - lo for lo, hi in cks)
    out_c = _nan((nmax, K), dev, torch.float64)
    # the three (alpha_scale, alpha_floor, p_floor) settings and the bound of test_gpu_launch_once_kernels.py::test_policy_logpdf
    for scale, floor, pfloor in [(1.0, 0.0, 0.0), (1.0, 1.0 + 1e-6, 0.0), (50.0, 0.0, 1e-6)]:
        out = _nan((N, K), dev, torch.float64)
        _call('mfg_policy_logpdf', pi.data_ptr(), P.data_ptr(), N, d, th.data_ptr(), K, 0.05, scale, floor, pfloor, out.data_ptr())
        for lo, hi in cks:
            out_c.fill_(NAN)
            _call('mfg_policy_logpdf', _ptr(pi, lo), _ptr(P, lo), hi - lo, d, th.data_ptr(), K, 0.05, scale, floor, pfloor,
                  out_c.data_ptr())
            _same(out, out_c, lo, hi, 'log q (scale %g)' % scale)
        got = out[idx_t].cpu().numpy()
        want = O.policy_logpdf(piw, Pw, thetas, 0.05, scale, floor, pfloor)
        err = np.abs(got - want) / np.maximum(np.abs(want), 1.0)
        rep.line('scale %g floor %g p_floor %g' % (scale, floor, pfloor), _per_window(err, c['W']), 1e-10)
        assert not np.isnan(got).any()
        assert float(err.max()) < 1e-10
        del out
    rep.done()


# ---------------------------------------------------------------------------------------------------- A. mfg_consistency_given
@pytest.mark.parametrize('c', **_by('mfg_consistency_given'))
def test_consistency_given(dev, slab, c):
    from discrete_mean_field_game_amd import _lib as L
    O = _O()
    d, T = c['d'], c['T']
    per = c['per_item']
    M = case_batch(c)
    P = slab.rows(d, M * per).view(M, T, d, d)
    wins, idx, idx_t = _windows(c, M, dev)
    rep = Report(c, M, 4 * M * per, wins)
    nws = int(L.lib().mfg_consistency_given_workspace_bytes(1, M, T, 1))
    ws = torch.empty(max(nws, 8) // 8 + 1, dtype=torch.float64, device=dev)
    metrics = _nan((1, 4), dev, torch.float64)
    steps, V = _nan((M, T, 2), dev, torch.float64), _nan((M, T + 1, d), dev, torch.float64)
    _call('mfg_consistency_given', P.data_ptr(), 1, M, T, d, metrics.data_ptr(), steps.data_ptr(), V.data_ptr(), ws.data_ptr(), 8 * ws.numel())
    cks = LB.chunks(M, per)
    nmax = max(hi - lo for lo, hi in cks)
    steps_c, V_c = _nan((nmax, T, 2), dev, torch.float64), _nan((nmax, T + 1, d), dev, torch.float64)
    m_c = _nan((1, 4), dev, torch.float64)
    for lo, hi in cks:
        steps_c.fill_(NAN), V_c.fill_(NAN)
        _call('mfg_consistency_given', _ptr(P, lo), 1, hi - lo, T, d, m_c.data_ptr(), steps_c.data_ptr(), V_c.data_ptr(), ws.data_ptr(),
              8 * ws.numel())
        _same(steps, steps_c, lo, hi, 'steps')
        _same(V, V_c, lo, hi, 'V')
    # windows: the bounds of test_gpu_consistency_pop.py::_check_steps (test_given_actions_against_oracle): V rtol 1e-12 / atol
    # 1e-13, l1 rtol 1e-12, jsd rtol 1e-10
    Pw = _host(P, idx_t, np.float32)
    Vo, l1o, jso = O.evaluate_synthetic_diffs(Pw)
    sw, Vw = steps[idx_t].cpu().numpy(), V[idx_t].cpu().numpy()
    for name, got, ref, rtol, atol in (('l1', sw[..., 0], l1o, 1e-12, 0.0), ('jsd', sw[..., 1], jso, 1e-10, 0.0), ('V', Vw, Vo, 1e-12, 1e-13)):
        assert not np.isnan(got).any(), name
        rep.line('%s |got - ref| / (atol + rtol |ref|)' % name, _per_window(np.abs(got - ref) / (atol + rtol * np.abs(ref) + 1e-300), c['W']), 1.0)
        assert np.allclose(got, ref, rtol=rtol, atol=atol), name
    assert np.array_equal(Vw[:, T], np.zeros((len(idx), d)))
    # the reduction over all M T hours: the criteria of test_gpu_consistency_pop.py::_check_metrics
    got_m = metrics.cpu().numpy()[0]
    all_steps = steps.cpu().numpy().reshape(-1, 2)
    for q, name in ((0, 'l1'), (1, 'jsd')):
        mean, std = float(np.mean(all_steps[:, q])), float(np.std(all_steps[:, q]))
        rep.line('%s mean rel err' % name, abs(got_m[2 * q] - mean) / abs(mean), 1e-12)
        assert np.isfinite(got_m).all()
        assert abs(got_m[2 * q] - mean) <= 1e-12 * abs(mean)
        assert abs(got_m[2 * q + 1] - std) <= 1e-9 * std + 1e-13 * abs(mean)
    rep.done()


# ---------------------------------------------------------------------------------------------------- B. mfg_sample_dirichlet
@pytest.mark.parametrize('c', **_by('mfg_sample_dirichlet'))
def test_sample_dirichlet(dev, slab, c):
    from discrete_mean_field_game_amd import _lib as L, ops
    from oracle import sampler_ref as SR
    d, precision = c['d'], c['precision']
    dd, prec = d * d, L.PRECISIONS[c['precision']]
    B = case_batch(c)
    seed, step = 31 + d, 3
    off = 2 ** 32 - B // 2                                            # the global trajectory id crosses 2^32 inside the batch
    pi = _dirichlet_states(B, d, dev, 17 + d)
    wins, idx, idx_t = _windows(c, B, dev)
    rep = Report(c, B, 4 * B * dd, wins)
    theta = torch.tensor([THETA], dtype=torch.float64, device=dev)
    ops.clear_status()
    P = slab.output(B * dd).view(B, d, d)
    _call('mfg_sample_dirichlet', pi.data_ptr(), B, d, theta.data_ptr(), SHIFT, SCALE, seed, step, off, prec, P.data_ptr())
    cks = LB.chunks(B, dd)
    nmax = max(hi - lo for lo, hi in cks)
    P_c = _nan((nmax, d, d), dev)
    for lo, hi in cks:
        P_c[:hi - lo].fill_(NAN)
        _call('mfg_sample_dirichlet', _ptr(pi, lo), hi - lo, d, theta.data_ptr(), SHIFT, SCALE, seed, step, off + lo, prec, P_c.data_ptr())
        _same(P, P_c, lo, hi, 'P')
    assert ops.status() == 0
    del P_c
    # the five windows in ONE compare: its cap MAX_AMBIGUOUS_FRACTION applies to the union, at the element count it was measured at
    res = SR.compare(_host(P, idx_t), _host(pi, idx_t, np.float32), THETA, SHIFT, SCALE, seed, step, precision=precision,
                     traj_ids=(np.uint64(off) + idx.astype(np.uint64)))
    rep.line('|P - P_ref| / bound (union)', res['worst'], 1.0)
    rep.line('ambiguous elements of %d' % res['n'], res['ambiguous'], SR.MAX_AMBIGUOUS_FRACTION * res['n'])
    assert res['n'] >= LB.MIN_WINDOW_ELEMENTS
    rep.done()


# ---------------------------------------------------------------------------------------------------- B. mfg_rollout
ROLLOUT_KEYS = ('pi_traj', 'pi_last', 'reward', 'delta', 'g', 'P')


def _rollout_outputs(n, T, d, dev, P=None):
    return {'pi_traj': _nan((n, T + 1, d), dev), 'pi_last': _nan((n, d), dev), 'reward': _nan((n, T), dev),
            'delta': _nan((n, T), dev, torch.float64), 'g': _nan((n, T), dev, torch.float64),
            'P': _nan((n, T, d, d), dev) if P is None else P}


@pytest.mark.parametrize('c', **_by('mfg_rollout'))
def test_rollout_write_P(dev, slab, c):
    from discrete_mean_field_game_amd import _lib as L, ops
    from oracle import sampler_ref as SR
    O = _O()
    d, T, per = c['d'], c['T'], c['per_item']
    B = case_batch(c)
    seed = 11
    pi0 = _dirichlet_states(B, d, dev, 0)
    wins, idx, idx_t = _windows(c, B, dev)
    rep = Report(c, B, 4 * B * per, wins)
    theta = torch.tensor([THETA], dtype=torch.float64, device=dev)
    F = ops.num_features(d)
    w = torch.as_tensor(np.random.RandomState(1).rand(F), device=dev)
    nws = int(L.lib().mfg_workspace_bytes(B * T, d))
    ws = torch.zeros(max(nws, 8) // 8, dtype=torch.float64, device=dev)
    flags = L.ROLLOUT_WRITE_P | L.ROLLOUT_TD
    ops.clear_status()

    def run(o, G, lo, n):
        _call('mfg_rollout', _ptr(pi0, lo), n, d, T, theta.data_ptr(), SHIFT, SCALE, w.data_ptr(), GAMMA, L.REWARD_MFG_AC2, seed, 0, lo,
              flags, o['pi_traj'].data_ptr(), o['pi_last'].data_ptr(), o['reward'].data_ptr(), o['delta'].data_ptr(), o['g'].data_ptr(),
              o['P'].data_ptr(), G.data_ptr(), 0, ws.data_ptr(), nws)

    whole = _rollout_outputs(B, T, d, dev, P=slab.output(B * per).view(B, T, d, d))
    G = torch.zeros(F + 3, dtype=torch.float64, device=dev)
    run(whole, G, 0, B)
    cks = LB.chunks(B, per)
    nmax = max(hi - lo for lo, hi in cks)
    part = _rollout_outputs(nmax, T, d, dev)
    Gsum, G_c = torch.zeros_like(G), torch.zeros_like(G)
    for lo, hi in cks:
        for k in ROLLOUT_KEYS:
            part[k].fill_(NAN)
        run(part, G_c, lo, hi - lo)
        for k in ROLLOUT_KEYS:
            _same(whole[k], part[k], lo, hi, k)
        Gsum += G_c
    rep.line('G: chunk sums vs whole', _split_sums_agree(Gsum, G), 1e-9)
    assert ops.status() == 0
    del part
    # the assertions of test_gpu_fullsize.py::test_fullsize_subsample_against_oracle on the window trajectories
    Pw = _host(whole['P'], idx_t)
    trw = whole['pi_traj'][idx_t].cpu().numpy()
    traj, r, dl, gg, _, _ = O.batched_rollout_given_P(_host(pi0, idx_t, np.float32), Pw, w.cpu().numpy(), THETA, SHIFT, gamma=GAMMA)
    W = c['W']
    e_t = np.abs(trw - traj)
    e_r = np.abs(_host(whole['reward'], idx_t) - r) / np.maximum(np.abs(r), 1e-3)
    e_d = np.abs(whole['delta'][idx_t].cpu().numpy() - dl) / np.maximum(np.abs(dl), 1e-2)
    e_g = np.abs(whole['g'][idx_t].cpu().numpy() - gg) / np.maximum(np.abs(gg), 1.0)
    for name, e, bound in (('pi_traj abs err', e_t, 1e-7), ('reward rel err', e_r, 1e-5), ('delta rel err', e_d, 1e-5), ('g rel err', e_g, 1e-5)):
        rep.line(name, _per_window(e, W), bound)
    np.testing.assert_allclose(trw, traj, rtol=0, atol=1e-7)
    assert np.max(e_r) < 1e-5 and np.max(e_d) < 1e-5 and np.max(e_g) < 1e-5
    res = SR.compare_rollout(Pw, trw, THETA, SHIFT, SCALE, seed, 0, idx.astype(np.uint64))
    rep.line('|P - P_ref| / bound (union)', res['worst'], 1.0)
    rep.line('ambiguous elements of %d' % res['n'], res['ambiguous'], SR.MAX_AMBIGUOUS_FRACTION * res['n'])
    assert res['n'] >= LB.MIN_WINDOW_ELEMENTS
    rep.done()


# ---------------------------------------------------------------------------------------------------- C. mfg_reward_net_forward
@pytest.mark.parametrize('c', **_by('mfg_reward_net_forward'))
def test_reward_net_forward(dev, slab, c):
    from discrete_mean_field_game_amd import ops
    from discrete_mean_field_game_amd.networks import RewardNet
    from oracle import reward_forward_cases as FC
    from oracle import reward_net_oracle as RO
    d, dd = c['d'], c['d'] * c['d']
    N = case_batch(c)
    torch.manual_seed(0)
    net = RewardNet(d=d).to(dev)                                       # the class default: reg = 'dropout_l1l2', n_fc3 = 8, n_fc4 = 4
    with torch.no_grad():                                               # non-trivial biases (zero by default)
        for p in net.parameters():
            if p.dim() == 1:
                p.uniform_(-0.2, 0.2)
    assert ops.reward_net_supported(net)
    n3, n4 = net.fc3.out_features, net.fc4.out_features
    keep = float(net.keep_prob) if c['dropout'] else 1.0
    seed, off = ((0x9E3779B97F4A7C15, (1 << 33) + 12345) if c['dropout'] else (0, 0))
    action = slab.rows(d, N * dd).view(N, d, d)
    state = _dirichlet_states(N, d, dev, 19)
    wins, idx, idx_t = _windows(c, N, dev)
    rep = Report(c, N, 4 * N * dd, wins)
    prm = [t.data_ptr() for t in (net.conv1.weight, net.conv1.bias, net.conv2.weight, net.conv2.bias, net.fc3.weight, net.fc3.bias,
                                  net.fc4.weight, net.fc4.bias, net.out.weight, net.out.bias)]

    def run(lo, n, out):
        _call('mfg_reward_net_forward', _ptr(state, lo), _ptr(action, lo), n, d, net.conv1.kernel_size[0], net.conv2.out_channels,
              net.conv2.kernel_size[0], n3, n4, *prm, keep, seed, off + lo, out.data_ptr())

    out = _nan((N,), dev)
    run(0, N, out)
    cks = LB.chunks(N, dd)
    out_c = _nan((max(hi - lo for lo, hi in cks),), dev)
    for lo, hi in cks:
        out_c.fill_(NAN)
        run(lo, hi - lo, out_c)
        _same(out, out_c, lo, hi, 'reward')
    # criterion a of tests/test_gpu_reward_net_forward_paths.py (oracle.reward_forward_cases.oracle): within TOL_REL max(|r_ref|, m),
    # m = |h4| . |out_w| + |out_b|, and no more than TOL_ABS (gain 1)
    p64 = RO.params_from_torch(net)
    masks = None
    if c['dropout']:
        ms = [RO.dropout_masks(net.keep_prob, seed, off + w.start, len(w), n3, n4) for w in wins]
        masks = (np.concatenate([m[0] for m in ms]), np.concatenate([m[1] for m in ms]))
    ref, cache = RO.forward_cache(p64, _host(state, idx_t), _host(action, idx_t), masks)
    m = np.abs(cache['h4']).dot(np.abs(p64['out_w'])) + np.abs(p64['out_b'])
    tol = np.minimum(FC.TOL_REL * np.maximum(np.abs(ref), m)[:, 0], FC.TOL_ABS[bool(c['dropout'])])
    got = out[idx_t].cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all() and np.abs(got).max() <= 1.0
    rep.line('|r - r_ref| / tolerance', _per_window(np.abs(got - ref[:, 0]) / tol, c['W']), 1.0)
    assert FC.ratio(got - ref[:, 0], tol) <= 1.0
    rep.done()


# ---------------------------------------------------------------------------------------------------- C. mfg_traj_log_z_pop
@pytest.mark.parametrize('c', **_by('mfg_traj_log_z_pop'))
def test_traj_log_z_pop(dev, slab, c):
    O = _O()
    d, T, K, per, W = c['d'], c['T'], c['K'], c['per_item'], c['W']
    total = case_batch(c)
    cap = total // K                                                    # K = 2: learner 1's stride carries the crossing of 2^31
    assert total * per > 2 ** 31
    n_pol, nss = 3, 7
    action = slab.rows(d, total * per).view(K * cap, T, d, d)
    state = _dirichlet_states(total * T, d, dev, 23).view(K * cap, T, d)
    wins = LB.boundary_windows(total, per, W)
    rep = Report(c, total, 4 * total * per, wins)
    rows = sorted({int(r) % cap for r in LB.window_index(wins)})        # ONLY the window rows: a tiny launch
    assert len(rows) == (5 * W if K == 1 else len(rows)) and len(rows) <= 5 * W
    rs = np.random.RandomState(29 + K)
    thetas, shifts = 7.9 + 1.1 * rs.rand(K, n_pol), np.array([0.0, 0.1])[:K]
    th, sh = torch.as_tensor(thetas, device=dev), torch.as_tensor(shifts, device=dev)
    rw = (C.c_int32 * len(rows))(*rows)
    scratch = torch.empty(len(rows), dtype=torch.int32, device=dev)
    out = torch.full((K, cap), 123.0, dtype=torch.float64, device=dev)
    _call('mfg_traj_log_z_pop', state.data_ptr(), action.data_ptr(), cap, rw, len(rows), T, d, th.data_ptr(), n_pol, sh.data_ptr(), K,
          int(K > 1), 1.0, 1.0 + 1e-6, 0.0, float(np.log(nss)), out.data_ptr(), scratch.data_ptr(), 4 * len(rows))
    rows_t = torch.as_tensor(rows, device=dev)
    listed = torch.zeros(cap, dtype=torch.bool, device=dev)
    listed[rows_t] = True
    assert bool((out[:, ~listed] == 123.0).all())                       # rows not listed keep the sentinel
    # the same rows from a compact copy of the store (addresses far below 2^29 floats): the same bits
    n = len(rows)
    st_s = state.view(K, cap, T, d)[:, rows_t].contiguous()
    ac_s = action.view(K, cap, T, d, d)[:, rows_t].contiguous()
    small = torch.full((K, n), 123.0, dtype=torch.float64, device=dev)
    rw_s = (C.c_int32 * n)(*range(n))
    _call('mfg_traj_log_z_pop', st_s.data_ptr(), ac_s.data_ptr(), n, rw_s, n, T, d, th.data_ptr(), n_pol, sh.data_ptr(), K, int(K > 1),
          1.0, 1.0 + 1e-6, 0.0, float(np.log(nss)), small.data_ptr(), scratch.data_ptr(), 4 * n)
    assert torch.equal(out[:, rows_t], small)
    # reference and tolerance of tests/test_gpu_importance_weights.py::test_log_weights_match_the_oracle (rtol 1e-9, atol 1e-6)
    got = out[:, rows_t].cpu().numpy()
    for k in range(K):
        want = O.calc_z(st_s[k].cpu().numpy(), ac_s[k].cpu().numpy(), thetas[k], shifts[k], nss)
        err = np.abs(got[k] - want) / (1e-6 + 1e-9 * np.abs(want))
        rep.line('learner %d |ln z - ref| / (atol + rtol |ref|)' % k, float(np.max(np.where(np.isnan(err), np.inf, err))), 1.0)
        np.testing.assert_allclose(got[k], want, rtol=1e-9, atol=1e-6)
    rep.done()


# ---------------------------------------------------------------------------------------------------- C. mfg_agents_step_pop
@pytest.mark.parametrize('c', **_by('mfg_agents_step_pop'))
def test_agents_step_pop(dev, slab, c):
    import agents_ref as ref
    d, K, dd, W = c['d'], c['K'], c['d'] * c['d'], c['W']
    agents, step = 50, 41
    total = case_batch(c)
    B = total // K
    assert B * dd < 2 ** 31 < total * dd                                # the crossing lies inside group 1
    P = slab.rows(d, total * dd).view(K, B, d, d)
    # counts: agents // d everywhere and one more in agents % d topics, from a topic that differs per member
    g = torch.Generator(device=dev)
    g.manual_seed(37)
    first = torch.randint(0, d, (K, B, 1), device=dev, generator=g)
    topic = torch.arange(d, device=dev).view(1, 1, d)
    counts = (agents // d + (((topic - first) % d) < agents % d)).to(torch.int32).contiguous()
    assert bool((counts.sum(-1) == agents).all())
    seeds = [(7 << 32) | 12345, 99]                                     # (the seeds of test_step_equals_the_restatement)
    sd = torch.as_tensor(np.asarray(seeds, dtype=np.uint64).view(np.int64), device=dev)
    wins = LB.boundary_windows(total, dd, W)
    idx = LB.window_index(wins)
    rep = Report(c, total, 4 * total * dd, wins)
    cn = torch.full((K, B, d), -7, dtype=torch.int32, device=dev)
    pn = _nan((K, B, d), dev)
    _call('mfg_agents_step_pop', counts.data_ptr(), P.data_ptr(), B, d, K, agents, sd.data_ptr(), step, 0, cn.data_ptr(), pn.data_ptr(), None)
    cks = LB.chunks(B, dd)
    nmax = max(hi - lo for lo, hi in cks)
    cn_c, pn_c = torch.empty(nmax, d, dtype=torch.int32, device=dev), _nan((nmax, d), dev)
    for k in range(K):
        for lo, hi in cks:
            cn_c.fill_(-7), pn_c.fill_(NAN)
            _call('mfg_agents_step_pop', _ptr(counts[k], lo), _ptr(P[k], lo), hi - lo, d, 1, agents, _ptr(sd, k), step, lo, cn_c.data_ptr(),
                  pn_c.data_ptr(), None)
            _same(cn[k], cn_c, lo, hi, 'counts_next of group %d' % k)
            _same(pn[k], pn_c, lo, hi, 'pi_next of group %d' % k)
    # windows against tests/agents_ref.py, exact, as tests/test_gpu_agents.py::test_step_equals_the_restatement (_same_as_ref)
    idx_t = torch.as_tensor(idx, device=dev)
    cw = counts.view(K * B, d)[idx_t].cpu().numpy()
    Pw = P.view(K * B, d, d)[idx_t].cpu().numpy()
    got_c, got_p = cn.view(K * B, d)[idx_t].cpu().numpy(), pn.view(K * B, d)[idx_t].cpu().numpy()
    bad = []
    for q, m in enumerate(idx):
        k, b = divmod(int(m), B)
        want = ref.step(cw[q], Pw[q], agents, seeds[k], step, b)
        bad.append(int(not (np.array_equal(got_c[q], want[0]) and np.array_equal(got_p[q].view(np.int32), want[2].view(np.int32)))))
    rep.line('members differing from the restatement', _per_window(bad, W), 0)
    assert not any(bad)
    assert np.array_equal(got_c.sum(-1), cw.sum(-1))                    # every agent lands somewhere
    rep.done()


# ---------------------------------------------------------------------------------------------------- D. elementwise helpers
def _fp64_windows(c, B, dev):
    """Windows of an fp64 output: round ELEMENTS 2^29, 2^30, 2^31 (per_item) and round the 2 / 4 / 8 GiB BYTE offsets (2 per_item
    floats per item), first and last."""
    a = LB.boundary_windows(B, c['per_item'], c['W'])
    b = LB.boundary_windows(B, 2 * c['per_item'], c['W'])
    wins = sorted({(w.start, w.stop) for w in a + b})
    wins = [range(lo, hi) for lo, hi in wins]
    idx = LB.window_index(wins)
    return wins, idx, torch.as_tensor(idx, device=dev)


@pytest.mark.parametrize('c', **_by('mfg_alpha'))
def test_alpha(dev, slab, c):
    O = _O()
    d, dd = c['d'], c['d'] * c['d']
    B = case_batch(c)
    assert B * dd > 2 ** 31
    LB.require_free(8 * B * dd + 2 ** 31)
    pi = _dirichlet_states(B, d, dev, 41)
    wins, idx, idx_t = _fp64_windows(c, B, dev)
    rep = Report(c, B, 8 * B * dd, wins)
    theta = torch.tensor([THETA], dtype=torch.float64, device=dev)
    out = torch.empty(B, d, d, dtype=torch.float64, device=dev)        # 17.2 GB: alpha, then alpha' (one output at a time)
    cks = LB.chunks(B, 2 * dd)
    out_c = _nan((max(hi - lo for lo, hi in cks), d, d), dev, torch.float64)
    piw = _host(pi, idx_t, np.float32)
    p64 = piw.astype(np.float64)
    z = THETA * (p64[:, None, :] - p64[:, :, None] - SHIFT)
    for which in ('alpha', "alpha'"):
        first = which == 'alpha'
        out.fill_(NAN)
        _call('mfg_alpha', pi.data_ptr(), B, d, theta.data_ptr(), SHIFT, out.data_ptr() if first else None, None if first else out.data_ptr())
        for lo, hi in cks:
            out_c.fill_(NAN)
            _call('mfg_alpha', _ptr(pi, lo), hi - lo, d, theta.data_ptr(), SHIFT, out_c.data_ptr() if first else None,
                  None if first else out_c.data_ptr())
            _same(out, out_c, lo, hi, which)
        got = out[idx_t].cpu().numpy()
        # the bounds of test_gpu_launch_once_kernels.py::_alpha_check: alpha 1e-9 relative against log1p(exp(z)), alpha' 1e-14 absolute
        if first:
            ref = np.log1p(np.exp(z))
            err, bound = np.abs(got - ref) / np.maximum(np.abs(ref), 1e-300), 1e-9
        else:
            err, bound = np.abs(got - O.calc_alpha_deriv(piw, THETA, SHIFT)), 1e-14
        rep.line(which, _per_window(err, c['W']), bound)
        assert float(np.max(np.where(np.isnan(err), np.inf, err))) < bound
    del out, out_c
    torch.cuda.empty_cache()
    rep.done()


@pytest.mark.parametrize('c', **_by('mfg_dirichlet_from_gamma'))
def test_dirichlet_from_gamma(dev, slab, c):
    O = _O()
    d, dd, W = c['d'], c['d'] * c['d'], c['W']
    B = case_batch(c)
    LB.require_free(4 * B * dd + 2 ** 31)
    wins, idx, idx_t = _windows(c, B, dev)
    rep = Report(c, B, 4 * B * dd, wins)
    y = slab.rows(d, B * dd).view(B, d, d)                             # any positive floats serve as gamma variates
    slab.tag = None
    for w in wins:                                                      # as test_dirichlet_from_gamma: an all-zero row, rows with zeros
        y[w.start, 0] = 0.0
        y[w.start, d - 1] = 0.0
        y[w.start + 1, 1, ::3] = 0.0
        y[w.start + 1, 1, d - 1] = 0.0
    out = _nan((B, d, d), dev)                                         # the second slab
    _call('mfg_dirichlet_from_gamma', y.data_ptr(), B, d, out.data_ptr())
    cks = LB.chunks(B, dd)
    out_c = _nan((max(hi - lo for lo, hi in cks), d, d), dev)
    for lo, hi in cks:
        out_c.fill_(NAN)
        _call('mfg_dirichlet_from_gamma', _ptr(y, lo), hi - lo, d, out_c.data_ptr())
        _same(out, out_c, lo, hi, 'P')
    # the criteria of test_gpu_launch_once_kernels.py::test_dirichlet_from_gamma: one fp32 ulp, every entry > 0, row sums within d 2^-24
    rows = y[idx_t].cpu().numpy().reshape(-1, d)
    got = out[idx_t].cpu().numpy().reshape(-1, d)
    ref = O.dirichlet_from_gamma(rows).astype(np.float32)
    assert not np.isnan(got).any()
    ulps = np.abs(got.astype(np.float64) - ref.astype(np.float64)) / np.spacing(np.abs(ref)).astype(np.float64)
    sums = np.abs(got.astype(np.float64).sum(-1) - 1.0)
    rep.line('ulps', _per_window(ulps.reshape(len(idx), -1), W), 1.0)
    rep.line('row sums', _per_window(sums.reshape(len(idx), -1), W), d * 2.0 ** -24)
    assert np.all(ulps <= 1.0) and np.all(got > 0) and np.all(sums <= d * 2.0 ** -24)
    for k in range(0, len(idx), W):
        assert np.array_equal(got[k * d], np.full(d, np.float32(1.0 / d))) and np.array_equal(got[k * d + d - 1], np.full(d, np.float32(1.0 / d)))
    del out, out_c
    torch.cuda.empty_cache()
    rep.done()


@pytest.mark.parametrize('c', **_by('mfg_features'))
def test_features(dev, slab, c):
    O = _O()
    d = c['d']
    F = O.num_features(d)
    assert F == c['per_item']
    B = case_batch(c)
    assert B * F > 2 ** 31
    LB.require_free(8 * B * F + 2 ** 31)
    pi = _dirichlet_states(B, d, dev, 43)
    wins, idx, idx_t = _fp64_windows(c, B, dev)
    rep = Report(c, B, 8 * B * F, wins)
    phi = _nan((B, F), dev, torch.float64)                             # 17.2 GB
    _call('mfg_features', pi.data_ptr(), B, d, phi.data_ptr())
    cks = LB.chunks(B, 2 * F)
    phi_c = _nan((max(hi - lo for lo, hi in cks), F), dev, torch.float64)
    for lo, hi in cks:
        phi_c.fill_(NAN)
        _call('mfg_features', _ptr(pi, lo), hi - lo, d, phi_c.data_ptr())
        _same(phi, phi_c, lo, hi, 'phi')
    # test_gpu_launch_once_kernels.py::test_features: products of two fp32 numbers are exact in fp64 -- array_equal
    got = phi[idx_t].cpu().numpy()
    ref = O.calc_features(_host(pi, idx_t, np.float32))
    rep.line('elements differing', _per_window((got != ref).sum(-1), c['W']), 0)
    assert np.array_equal(got, ref)
    del phi, phi_c
    torch.cuda.empty_cache()
    rep.done()
