"""CPU: the restatement of mfg_moves_loglik_pop (tests/moves_loglik_ref.py) against 50-digit arithmetic and against the
central difference of its own value; the argument rules of ops.moves_loglik_pop, of the library's entry point and of
likelihood that need no GPU; the update rule of likelihood.fit on a stub."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

import moves_loglik_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

A_VALUES = (1e-8, 0.3, 1.0, 30.0, 1e3, 1.8e5)
M_VALUES = (1, 8, 9, 64, 65, 1000)


# ---------------------------------------------------------------------------------------------------- the restatement
def test_T_and_D_against_50_digits():
    """36 cells.  fsum adds the rounded terms exactly, so the error is that of the terms: m ulps of the largest at most."""
    mp = pytest.importorskip('mpmath')
    mp.mp.dps = 50
    for a in A_VALUES:
        for m in M_VALUES:
            T, S = R.T(a, m)
            want_T = mp.loggamma(mp.mpf(a) + m) - mp.loggamma(mp.mpf(a))
            want_D = mp.psi(0, mp.mpf(a) + m) - mp.psi(0, mp.mpf(a))
            assert abs(T - want_T) <= 1e-14 * S, (a, m)
            assert abs(R.D(a, m) - want_D) <= 1e-14 * want_D, (a, m)
            assert S >= abs(T)


def test_the_edges_of_T_and_D():
    for a in (0.0, 1e-300, 1.0, 1e30):
        assert R.T(a, 0) == (0.0, 0.0) and R.D(a, 0) == 0.0
    assert R.T(0.0, 3)[0] == -math.inf and R.D(0.0, 3) == math.inf
    assert R.T(2.0, 3)[0] == pytest.approx(math.log(24.0), rel=1e-15)          # 2 * 3 * 4


def _case(d=4, seed=0, agents=40):
    rs = np.random.RandomState(seed)
    pi = rs.dirichlet(np.ones(d)).astype(np.float32)
    moves = rs.multinomial(agents, np.ones(d * d) / (d * d)).reshape(d, d)
    moves[1] = 0                                                                # a row with n_i = 0
    return pi, moves


def test_a_row_is_the_polya_probability():
    """d = 2, one row occupied: the closed form by hand, lgamma and all, against 50 digits."""
    mp = pytest.importorskip('mpmath')
    mp.mp.dps = 50
    pi = np.float32([0.3, 0.7])
    moves = np.array([[3, 5], [0, 0]])
    ll, grad, S, G, flag = R.transition(pi, moves, 2.0, 0.1, 5.0)
    a = R.alphas(pi, 2.0, 0.1, 5.0)[0][0]
    a0, a1 = mp.mpf(float(a[0])), mp.mpf(float(a[1]))
    want = (mp.loggamma(9) - mp.loggamma(4) - mp.loggamma(6) + mp.loggamma(a0 + 3) - mp.loggamma(a0) + mp.loggamma(a1 + 5)
            - mp.loggamma(a1) - mp.loggamma(a0 + a1 + 8) + mp.loggamma(a0 + a1))
    assert flag == 0 and abs(ll - want) <= 1e-14 * S


def test_the_probabilities_of_a_row_sum_to_one():
    """All outcomes of 4 agents over 3 columns."""
    pi = np.float32([0.2, 0.5, 0.3])
    total = 0.0
    for m0 in range(5):
        for m1 in range(5 - m0):
            moves = np.zeros((3, 3), np.int64)
            moves[0] = (m0, m1, 4 - m0 - m1)
            total += math.exp(R.transition(pi, moves, 3.0, 0.05, 2.0)[0])
    assert abs(total - 1.0) < 1e-13


@pytest.mark.parametrize('point', [(8.86349, 0.16, 12000.0), (2.0, -0.1, 1.0), (0.0, 0.0, 1e-3)])
def test_the_gradient_is_the_central_difference_of_the_value(point):
    pi, moves = _case()
    theta, shift, alpha = point
    ll, grad, S, G, flag = R.transition(pi, moves, theta, shift, alpha)
    assert flag == 0
    f = lambda p: R.transition(pi, moves, p[0], p[1], math.exp(p[2]))[0]
    p0 = np.array([theta, shift, math.log(alpha)])
    for k in range(3):
        h = 1e-5 * max(1.0, abs(p0[k]))
        e = np.zeros(3)
        e[k] = h
        fd = (f(p0 + e) - f(p0 - e)) / (2 * h)
        # the truncation error of the difference is O(h^2 f'''); its rounding error eps S / h
        assert abs(fd - grad[k]) <= 1e-6 * G[k] + 1e-15 * S / h, (k, fd, grad[k])


def test_the_failures_of_a_transition():
    pi, moves = _case()
    bad = moves.copy()
    bad[2, 1] = -1
    assert R.transition(pi, bad, 1.0, 0.0, 1.0)[4] == R.BAD_DATA
    assert R.transition(np.float32([np.nan, 0.5, 0.2, 0.3]), moves, 1.0, 0.0, 1.0)[4] == R.BAD_DATA
    # every x below -0.3: theta = 3000 underflows every a to 0
    pi = np.float32([0.4, 0.35, 0.25])
    zero = np.zeros((3, 3), np.int64)
    zero[0, 1] = 2
    r = R.transition(pi, zero, 3000.0, 0.5, 1.0)
    assert r[0] == -math.inf and r[4] == R.ZERO_ALPHA and np.isnan(r[1]).all()
    out = R.loglik(np.float32(np.ones((1, 2, 3)) / 3), zero[None, None], np.nan, 0.0, 1.0, 3)
    assert out['status'][0] == R.BAD_POLICY and np.isnan(out['ll_day'][0])
    assert R.loglik(np.float32(np.ones((1, 2, 3)) / 3), zero[None, None], 1.0, 0.0, 0.0, 3)['status'][0] == R.BAD_POLICY


# ---------------------------------------------------------------------------------------------------- header, binding, library
@pytest.fixture(scope='module')
def lib():
    from discrete_mean_field_game_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib


def test_the_new_symbols_are_declared_bound_and_exported(lib):
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'mfg_hip.h')).read(), flags=re.S)
    for name in ('mfg_moves_loglik_pop', 'mfg_moves_loglik_workspace_bytes'):
        assert re.search(r'\b%s\s*\(' % name, text) and name in lib.SIGNATURES
        assert getattr(lib.lib(), name) is not None
    assert lib.lib().mfg_abi_version() == 18


def test_struct_layout_matches_the_header(lib, tmp_path):
    fields = [n for n, _ in lib.MovesLoglikStruct._fields_]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "mfg_hip.h"\nint main(void){printf("%zu", sizeof(mfg_moves_loglik_t));\n'
           + ''.join('printf(" %%zu", offsetof(mfg_moves_loglik_t, %s));\n' % n for n in fields) + 'return 0;}\n')
    c = tmp_path / 'layout.c'
    c.write_text(src)
    exe = str(tmp_path / 'layout')
    rocm = os.environ.get('ROCM_PATH', '/opt/rocm')
    subprocess.run(['gcc', '-std=c99', '-D__HIP_PLATFORM_AMD__', '-I' + os.path.join(rocm, 'include'),
                    '-I' + os.path.join(ROOT, 'include'), str(c), '-o', exe], check=True)
    got = [int(x) for x in subprocess.run([exe], check=True, stdout=subprocess.PIPE).stdout.split()]
    S = lib.MovesLoglikStruct
    assert got == [ctypes.sizeof(S)] + [getattr(S, n).offset for n in fields]


def _descriptor(lib, **kw):
    f = lib.MovesLoglikStruct()
    for name in ('state', 'moves', 'theta', 'shift', 'alpha_scale', 'll', 'll_day', 'grad', 'grad_day', 'status', 'workspace'):
        setattr(f, name, 256)                   # never dereferenced: every case below is refused before a launch
    f.workspace_bytes = 1 << 30
    f.N, f.H, f.d, f.width, f.sets, f.policies = 2, 3, 4, 5, 1, 3
    for name, value in kw.items():
        setattr(f, name, value)
    return f


@pytest.mark.parametrize('code,kw', [
    (-1, dict(state=None)), (-1, dict(moves=None)), (-1, dict(theta=None)), (-1, dict(ll=None)), (-1, dict(status=None)),
    (-1, dict(grad=None)), (-1, dict(grad_day=None)), (-1, dict(policies=0)), (-1, dict(policies=65536)), (-1, dict(N=0)),
    (-1, dict(H=1)), (-1, dict(d=0)), (-1, dict(d=65, width=70)), (-1, dict(d=6)), (-1, dict(sets=0)),
    (-1, dict(sets=2, state_stride=23, moves_stride=100)), (-1, dict(sets=2, state_stride=24, moves_stride=99)),
    (-1, dict(workspace=None)), (-1, dict(workspace=260)), (-4, dict(workspace_bytes=255))])
def test_the_library_refuses_before_it_launches(lib, code, kw):
    assert lib.lib().mfg_moves_loglik_pop(ctypes.byref(_descriptor(lib, **kw))) == code
    assert lib.lib().mfg_last_error()
    assert lib.lib().mfg_moves_loglik_pop(None) == -1


def test_the_workspace_query(lib):
    q = lib.lib().mfg_moves_loglik_workspace_bytes
    up = lambda n: (n + 255) // 256 * 256
    assert q(3, 1, 2, 3, 4) == up(1 * 2 * 2 * 4 * 8) + up(3 * 2 * 2 * 4)
    assert q(1000, 7, 24, 16, 21) == up(7 * 24 * 15 * 21 * 8) + up(1000 * 24 * 15 * 4)
    for bad in ((0, 1, 2, 3, 4), (65536, 1, 2, 3, 4), (3, 0, 2, 3, 4), (3, 1, 0, 3, 4), (3, 1, 2, 1, 4), (3, 1, 2, 3, 0), (3, 1, 2, 3, 65)):
        assert q(*bad) == 0


def test_ops_argument_rules():
    from discrete_mean_field_game_amd import ops
    chk = ops.check_moves_loglik_args
    assert chk((2, 3, 4), (2, 2, 5, 5), 3, 4) == (1, 2, 3, 4, 5)
    assert chk((7, 2, 3, 4), (7, 2, 2, 4, 4), 3, 4, 3) == (7, 2, 3, 4, 4)
    for args, match in [(((2, 3), (2, 2, 5, 5), 3, 4), 'expected'), (((2, 3, 4), (2, 2, 5), 3, 4), 'expected'),
                        (((2, 3, 4), (2, 2, 5, 5), 3, 3), 'last axis'), (((2, 3, 4), (2, 3, 5, 5), 3, 4), 'moves'),
                        (((2, 3, 4), (2, 2, 3, 3), 3, 4), 'width'), (((2, 1, 4), (2, 0, 5, 5), 3, 4), 'two hours'),
                        (((2, 3, 65), (2, 2, 65, 65), 3, 65), r'outside \[1, 64\]'), (((2, 3, 4), (2, 2, 5, 5), 0, 4), 'K=0'),
                        (((2, 3, 4), (2, 2, 5, 5), 65536, 4), 'at most 65535'), (((2, 3, 4), (2, 2, 5, 5), 3, 4, 2), 'set_index')]:
        with pytest.raises(ValueError, match=match):
            chk(*args)
    assert set(ops.moves_loglik_shapes(3, 2, 5)) == set(ops.MOVES_LOGLIK_OUTPUTS)


def _demos(N=2, H=3, d=3, width=4, R=None):
    from discrete_mean_field_game_amd.demos import BootstrapDemonstrations, Demonstrations
    def arrays(lead):
        z = lambda *s: np.zeros(lead + s, np.int32)
        return dict(state=np.zeros(lead + (N, H, d), np.float32), action=np.zeros(lead + (N, H - 1, d, d), np.float32),
                    counts=z(N, H, width), moves=z(N, H - 1, width, width), present=z(N, H), left=z(N, H - 1, width),
                    entered=z(N, H - 1, width), status=z(N), order=None)
    sample = Demonstrations(arrays(()), d, width)
    return sample if R is None else BootstrapDemonstrations(sample, arrays((R,)))


def test_likelihood_argument_rules():
    from discrete_mean_field_game_amd import likelihood as LK
    th, sh, al = LK.check_policy_args([1.0, 2.0], 0.1, 5.0)
    assert th.tolist() == [1.0, 2.0] and sh.tolist() == [0.1, 0.1] and al.tolist() == [5.0, 5.0]
    with pytest.raises(ValueError, match='one length'):
        LK.check_policy_args([1.0, 2.0], [0.1, 0.2, 0.3], 5.0)
    one, boot = _demos(), _demos(R=3)
    state, moves, index, days = LK.check_data_args(one, 2, days=[1])
    assert state.shape == (1, 1, 3, 3) and moves.shape == (1, 1, 2, 4, 4) and index is None and days == [1]
    state, moves, index, days = LK.check_data_args(boot, 3)
    assert state.shape == (3, 2, 3, 3) and index.tolist() == [0, 1, 2] and index.dtype == np.int32
    assert LK.check_data_args(boot, 2, set_index=[2, 0])[2].tolist() == [2, 0]
    for args, kw, match in [((one, 2), dict(set_index=[0, 0]), 'BootstrapDemonstrations only'), ((one, 2), dict(days=[2]), 'days outside'),
                            ((boot, 2), {}, 'one policy per replicate'), ((boot, 2), dict(set_index=[0, 3]), r'in \[0, 3\)'),
                            ((boot, 2), dict(set_index=[0]), 'expected 2'), ((object(), 1), {}, 'Demonstrations'),
                            ((one, 1), dict(days=[]), 'at least one day')]:
        with pytest.raises(ValueError, match=match):
            LK.check_data_args(*args, **kw)
    assert LK.free_mask(('theta',)).tolist() == [1.0, 0.0, 0.0] and LK.free_mask('shift').tolist() == [0.0, 1.0, 0.0]
    for bad in ((), ('alpha',), ('theta', 'nu')):
        with pytest.raises(ValueError, match='free'):
            LK.free_mask(bad)
    with pytest.raises(ValueError, match='steps'):
        LK.fit(one, 1.0, 0.0, 1.0, steps=0)
    with pytest.raises(ValueError, match='positive'):
        LK.fit(one, 1.0, 0.0, 0.0)
    with pytest.raises(ValueError, match='BootstrapDemonstrations'):
        LK.fit_bootstrap(one, 1.0, 0.0, 1.0)
    with pytest.raises(ValueError, match='level'):
        LK.fit_bootstrap(boot, 1.0, 0.0, 1.0, level=1.0)
    with pytest.raises(ValueError, match='one per replicate'):
        LK.fit_bootstrap(boot, [1.0, 2.0], 0.0, 1.0)


def test_the_result_classes():
    from discrete_mean_field_game_amd import likelihood as LK
    ll_day = np.array([[1.0, 2.0, 4.0], [-1.0, -2.0, -4.0]])
    res = LK.LogLik(np.zeros((2, 3, 1)), ll_day, np.ones((2, 3, 3)), np.zeros((2, 3), np.int32), [0, 2, 5])
    assert res.total().tolist() == [7.0, -7.0] and res.total([5, 0]).tolist() == [5.0, -5.0]
    assert res.grad_total([2]).tolist() == [[1.0] * 3] * 2
    with pytest.raises(ValueError, match='not all among'):
        res.total([1])
    points = [(1, 0, 1), (2, 0, 1), (3, 0, 1), (4, 0, 1)]
    status = np.zeros((4, 2), np.int32)
    status[2, 1] = 2
    assert LK.best_point(points, np.array([-5.0, -3.0, -1.0, -3.0]), status) == (1, (2, 0, 1), -3.0)       # first maximum, clean
    assert LK.best_point(points[:1], np.array([np.nan]), status[:1])[0] is None
    fit = LK.Fit(np.array([[1.0, 0.1, 10.0], [2.0, 0.2, 20.0], [4.0, 0.3, 30.0], [9.0, 0.9, 90.0]]), None, None, None, None,
                 np.array([0, 0, 0, 4]), None)
    b = LK.BootstrapFit(fit, 0.5)
    assert b.used.tolist() == [True, True, True, False] and b.mean[0] == pytest.approx(7.0 / 3.0)
    assert b.interval[:, 0].tolist() == [1.0, 4.0] and b.std[2] == pytest.approx(np.std([10.0, 20.0, 30.0]))


# ---------------------------------------------------------------------------------------------------- the update rule on a stub
def test_the_update_rule_of_fit_on_a_stub():
    """A concave quadratic on CPU tensors: ascent follows moves_loglik_ref.adam_step to the last bit but rounding (the two
    evaluate x ** 0.5 and the divisions in the same order), a start that turns bad is frozen at its last good iterate, a fixed
    parameter keeps its bits."""
    torch = pytest.importorskip('torch')
    from discrete_mean_field_game_amd import likelihood as LK
    centre = np.array([[1.0, -2.0, 0.5], [0.0, 0.0, 0.0], [3.0, 1.0, -1.0]])
    curv = np.array([1.0, 4.0, 0.25])
    p0 = np.array([[0.0, 0.0, 0.0], [1.0, 1.0, 1.0], [2.9, 1.2, -1.3]])
    steps, lr, mask = 12, 0.1, np.array([1.0, 0.0, 1.0])
    calls = []

    def evaluate(p):
        x = p.numpy()
        calls.append(x.copy())
        value = -0.5 * ((x - centre) ** 2 * curv).sum(1)
        status = np.zeros(3, np.int32)
        if len(calls) >= 6:
            status[1] = 2                                       # start 1 turns bad at its sixth evaluation (step index 5)
        return torch.as_tensor(value), torch.as_tensor(-(x - centre) * curv), torch.as_tensor(status)

    r = LK.ascent(evaluate, torch.as_tensor(p0), mask, steps, lr)
    assert len(calls) == steps + 1
    p, m, v = p0.copy(), np.zeros((3, 3)), np.zeros((3, 3))
    trace = np.zeros((steps, 3))
    for t in range(1, steps + 1):
        trace[t - 1] = -0.5 * ((p - centre) ** 2 * curv).sum(1)
        p, m, v = R.adam_step(p, -(p - centre) * curv, m, v, t, lr, mask)
        if t == 5:
            p5 = p.copy()
    got = r['trace'].numpy()
    np.testing.assert_allclose(got[:, [0, 2]], trace[:, [0, 2]], rtol=1e-13, atol=0)
    np.testing.assert_allclose(r['p'].numpy()[[0, 2]], p[[0, 2]], rtol=1e-13, atol=0)
    assert np.array_equal(r['p'].numpy()[:, 1], p0[:, 1])                                # the fixed parameter: the same bits
    # start 1: rows 0 .. 4 are values, NaN from row 5; it sits at the iterate of its fifth evaluation (p_4), the last good one
    assert np.isfinite(got[:5, 1]).all() and np.isnan(got[5:, 1]).all()
    np.testing.assert_allclose(got[:5, 1], trace[:5, 1], rtol=1e-13, atol=0)
    assert np.array_equal(r['p'].numpy()[1], calls[4][1]) and not np.array_equal(calls[4][1], p5[1])
    assert r['status'].tolist() == [0, 2, 0] and r['frozen_at'].tolist() == [-1, 5, -1]
    assert np.array_equal(calls[7][1], calls[4][1])                                      # and is evaluated there from then on
    # the best iterate: the values rise towards the centre, so it is the final one
    final = -0.5 * ((p - centre) ** 2 * curv).sum(1)
    np.testing.assert_allclose(r['final_value'].numpy()[[0, 2]], final[[0, 2]], rtol=1e-13)
    assert r['best_value'].numpy()[0] == max(got[:, 0].max(), r['final_value'].numpy()[0])
    assert r['best_value'].numpy()[1] == got[:5, 1].max()
