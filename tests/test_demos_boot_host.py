"""CPU: the definitions behind mfg_demos_bootstrap (include/mfg_hip.h) and its argument rules.  The twelve literals of the
weight table are recomputed with 60-digit decimals; the weights of the restatement (tests/demos_boot_ref.py) are Poisson(1), do
or do not depend on the day as the unit says and never on H; a replicate is the plain count of the log in which agent u
appears w times; the argument rules need no GPU."""
import ctypes as C
import decimal
import os
import re
import subprocess

import numpy as np
import pytest

import demos_boot_ref as B
import demos_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _table():
    decimal.getcontext().prec = 60
    e1 = decimal.Decimal(-1).exp()
    out, cdf, fact = [], decimal.Decimal(0), decimal.Decimal(1)
    for k in range(12):
        fact = fact * k if k else fact
        cdf += e1 / fact
        out.append(int((cdf * (1 << 32)).to_integral_value(rounding=decimal.ROUND_FLOOR)))
    return tuple(out)


def test_the_table_is_floor_of_two_to_32_times_the_poisson_cdf():
    from discrete_mean_field_game_amd import _lib
    want = _table()
    assert want == (1580030168, 3160060337, 3950075421, 4213413783, 4279248373, 4292415291, 4294609777, 4294923276, 4294962463,
                    4294966817, 4294967252, 4294967292)
    assert B.TABLE == want and _lib.DEMOS_BOOT_TABLE == want
    text = open(os.path.join(ROOT, 'include', 'mfg_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    body = re.search(r'#define MFG_DEMOS_BOOT_TABLE((?:[^\n]*\\\n)*[^\n]*)', text).group(1)
    assert tuple(int(x) for x in re.findall(r'(\d+)u', body)) == want
    tag = int(re.search(r'#define MFG_DEMOS_BOOT_TAG (0x[0-9A-Fa-f]+)u', text).group(1), 16)
    assert tag == B.TAG == _lib.DEMOS_BOOT_TAG and tag < 1 << 16
    assert max(want) < 1 << 32 and (1 << 32) - want[-1] <= 4          # the folded tail: mass < 2^-30 (in fact < 2^-32 beyond 12)


def test_the_weights_are_poisson_one():
    n = 1 << 22
    w = B.weights(4, 1, n // 4, seed=(5 << 40) + 17).reshape(-1)
    assert w.size == n and w.min() == 0 and w.max() <= 12
    p, fact = [], 1.0
    for k in range(7):
        fact = fact * k if k else 1.0
        p.append(np.exp(-1.0) / fact)
    for k in range(7):
        sigma = np.sqrt(p[k] * (1 - p[k]) / n)
        assert abs((w == k).mean() - p[k]) < 5 * sigma, k
    assert abs(w.mean() - 1.0) < 5 * np.sqrt(1.0 / n)                  # var of Poisson(1) is 1
    assert abs(w.var() - 1.0) < 5 * np.sqrt(3.0 / n)                   # var of (X - 1)^2: mu4 - 1 = 4 - 1 = 3


def test_the_unit_decides_whether_the_day_matters_and_the_hour_never_does():
    a = B.weights(5, 3, 500, seed=9, unit='agent')
    assert (a[:, 0] == a[:, 1]).all() and (a[:, 0] == a[:, 2]).all()
    assert (a == B.weights(5, 3, 500, seed=9, unit='agent', day_offset=7)).all()
    d = B.weights(5, 3, 500, seed=9, unit='agent_day')
    assert (d[:, 0] != d[:, 1]).any() and (d[:, 1] != d[:, 2]).any()
    assert (d[:, 1:] == B.weights(5, 2, 500, seed=9, unit='agent_day', day_offset=1)).all()      # day_offset + n is the key
    assert (d[0] != d[1]).any() and (d != B.weights(5, 3, 500, seed=10)).any()
    # a day key past 2^32 reaches the fourth counter word
    assert (B.weights(1, 1, 500, 9, day_offset=1 << 32) != B.weights(1, 1, 500, 9, day_offset=0)).any()
    rs = np.random.RandomState(3)
    rank = np.arange(6)
    for unit in B.UNITS:                                   # the first hours of a longer log: the same replicate
        log = rs.randint(-1, 6, (2, 5, 300)).astype(np.int32)
        long, short = B.bootstrap(log, rank, 6, 3, 3, 11, unit=unit), B.bootstrap(log[:, :3], rank, 6, 3, 3, 11, unit=unit)
        assert R.same(long['counts'][:, :, :3], short['counts']) and R.same(long['moves'][:, :, :2], short['moves'])


def test_a_replicate_is_the_count_of_the_resampled_log():
    N, H, U, Cn, d, width = 2, 4, 300, 9, 3, 5
    rs = np.random.RandomState(4)
    log = rs.randint(-1, Cn, (N, H, U)).astype(np.int32)
    rank = np.array([[2, 0, -1, 1, 4, 3, 7, 5, 6], [0, 1, 2, 3, 4, -1, 5, 6, 8]])
    seed, Rn = (3 << 33) + 5, 5
    got = B.bootstrap(log, rank, Cn, d, Rn, seed, width=width)
    w = B.weights(Rn, N, U, seed)
    for r in range(Rn):
        for n in range(N):
            want = R.from_logs(B.resampled_log(log[n], w[r, n])[None], Cn, d, width, 'given', rank[n:n + 1])
            for name in B.OUTPUTS:
                assert R.same(got[name][r, n], want[name][0]), (name, r, n)
    assert not R.same(got['counts'][0], got['counts'][1])


def test_the_argument_rules_need_no_gpu():
    from discrete_mean_field_game_amd import _lib, demos, ops
    ok = ((2, 3, 100), (2, 6), 6, 3, 4)
    assert ops.check_demos_boot_args(*ok) == (2, 3, 100, 6, 3, 3)
    assert ops.check_demos_boot_args((2, 3, 100), (1, 6), 6, 3, 1024, width=4, unit='agent') == (2, 3, 100, 6, 3, 4)
    for R_ in (0, 1025):
        with pytest.raises(ValueError):
            ops.check_demos_boot_args((2, 3, 100), (2, 6), 6, 3, R_)
    ops.check_demos_boot_args((1, 2, (2 ** 31 - 1) // 12), (1, 6), 6, 3, 1)
    with pytest.raises(ValueError):
        ops.check_demos_boot_args((1, 2, (2 ** 31 - 1) // 12 + 1), (1, 6), 6, 3, 1)
    with pytest.raises(ValueError):
        ops.check_demos_boot_args(*ok, unit='person')
    for shape in ((3, 6), (2, 5), (6,), None):
        with pytest.raises(ValueError):
            ops.check_demos_boot_args((2, 3, 100), shape, 6, 3, 4)
    with pytest.raises(ValueError):
        ops.check_demos_boot_args(*ok, day_offset=-1)
    with pytest.raises(ValueError):
        ops.check_demos_boot_args(*ok, day_offset=2 ** 48 - 1)
    ops.check_demos_boot_args(*ok, day_offset=2 ** 48 - 1, unit='agent')
    with pytest.raises(ValueError):
        ops.check_replicate_bands_args((4, 3), (4,))
    with pytest.raises(ValueError):
        ops.check_replicate_bands_args((1025, 3), ())
    with pytest.raises(ValueError):
        ops.check_replicate_bands_args((9, 3), range(9))
    assert ops.check_replicate_bands_args((4, 3, 5), (3, 0, 0)) == (4, 15, [3, 0, 0])
    with pytest.raises(ValueError):
        demos.bootstrap(np.zeros((2, 3, 10), np.int32), 1, 0, categories=2)
    with pytest.raises(ValueError):
        demos.bootstrap(np.zeros((2, 3, 10), np.int32), 1, 4, categories=2, unit='person')
    assert _lib.DEMOS_UNITS == {'agent_day': 0, 'agent': 1}


@pytest.fixture(scope='module')
def lib():
    from discrete_mean_field_game_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib


@pytest.mark.parametrize('ctype, struct', [('mfg_demos_boot_t', 'DemosBootStruct'), ('mfg_replicate_bands_t', 'ReplicateBandsStruct')])
def test_struct_layouts_match_the_header(lib, tmp_path, ctype, struct):
    S = getattr(lib, struct)
    fields = [n for n, _ in S._fields_]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "mfg_hip.h"\nint main(void){printf("%%zu", sizeof(%s));\n' % ctype
    for f in fields:
        src += 'printf(" %%zu", offsetof(%s, %s));\n' % (ctype, f)
    src += 'return 0;}\n'
    c = tmp_path / 'layout.c'
    c.write_text(src)
    exe = str(tmp_path / 'layout')
    subprocess.run(['gcc', '-std=c99', '-I', os.path.join(ROOT, 'include'), str(c), '-o', exe], check=True)
    out = [int(x) for x in subprocess.run([exe], check=True, stdout=subprocess.PIPE).stdout.decode().split()]
    assert out[0] == C.sizeof(S)
    assert out[1:] == [getattr(S, f).offset for f in fields]


def _descriptor(lib, **kw):
    f = lib.DemosBootStruct()
    f.topic = f.rank = f.status = f.workspace = 256               # never dereferenced: every case below is refused first
    f.N, f.H, f.U, f.C, f.d, f.width, f.R, f.rank_rows = 2, 3, 100, 6, 3, 3, 4, 2
    f.workspace_bytes = lib.lib().mfg_demos_bootstrap_workspace_bytes(4, 2, 3, 6, 3)
    for k, v in kw.items():
        setattr(f, k, v)
    return f


@pytest.mark.parametrize('code, kw', [(-1, dict(R=0)), (-1, dict(R=1025)), (-1, dict(U=(2 ** 31 - 1) // 12 + 1)), (-1, dict(rank=None)),
                                      (-1, dict(rank_rows=3)), (-1, dict(unit=2)), (-1, dict(workspace_bytes=8)),
                                      (-1, dict(day_offset=-1)), (-1, dict(day_offset=2 ** 48 - 1)), (-1, dict(status=None)),
                                      (-1, dict(H=1)), (-1, dict(d=4)), (-1, dict(width=7, d=3)), (-1, dict(empty_row=2)),
                                      (-1, dict(groups=-1)), (-1, dict(workspace=None)), (-1, dict(C=4097)),
                                      (-3, dict(width=65, d=3, C=100))])
def test_the_entry_point_refuses_before_it_launches(lib, code, kw):
    h = lib.lib()
    assert h.mfg_demos_bootstrap(C.byref(_descriptor(lib, **kw))) == code, kw        # MFG_EINVAL -1, MFG_EUNSUPPORTED -3
    assert h.mfg_demos_bootstrap(None) == -1


def test_the_workspace_query(lib):
    h = lib.lib()
    up = lambda b: (b + 255) // 256 * 256
    for R_, N, H, Cn, w in ((4, 2, 3, 6, 3), (1024, 1, 2, 1, 1), (17, 24, 16, 47, 20), (3, 2, 7, 4096, 64)):
        assert h.mfg_demos_bootstrap_workspace_bytes(R_, N, H, Cn, w) == up(N * 4) + up(R_ * N * H * w * 4) + up(R_ * N * (H - 1) * w * w * 4)
    for bad in ((0, 2, 3, 6, 3), (1025, 2, 3, 6, 3), (4, 0, 3, 6, 3), (4, 2, 1, 6, 3), (4, 2, 3, 4097, 3), (4, 2, 3, 6, 7), (4, 2, 3, 100, 65)):
        assert h.mfg_demos_bootstrap_workspace_bytes(*bad) == 0
    f = _descriptor(lib, workspace_bytes=8)
    assert h.mfg_demos_bootstrap(C.byref(f)) == -1 and b'need' in h.mfg_last_error()
    b = lib.ReplicateBandsStruct()
    assert h.mfg_replicate_bands(None) == -1 and h.mfg_replicate_bands(C.byref(b)) == -1
    b.x, b.R, b.cells, b.Q = 256, 4, 10, 1
    assert h.mfg_replicate_bands(C.byref(b)) == -1                  # Q > 0 without quant
    b.quant = 256
    b.ranks[0] = 4
    assert h.mfg_replicate_bands(C.byref(b)) == -1                  # a rank outside [0, R)
    b.ranks[0], b.Q = 0, 9
    assert h.mfg_replicate_bands(C.byref(b)) == -1


def test_the_bands_of_the_restatement():
    x = np.array([[1, 5, np.nan], [3, 5, 1], [2, 5, 2]], np.float32)
    mean, std, quant = B.bands(x, (2, 0, 0, 1))
    assert mean[0] == 2 and mean[1] == 5 and np.isnan(mean[2]) and std[1] == 0 and np.isnan(std[2])
    assert std[0] == np.sqrt(np.float64(2) / 3)
    assert R.same(quant[:, :2], np.array([[3, 5], [1, 5], [1, 5], [2, 5]], np.float32)) and np.isnan(quant[:, 2]).all()
