"""CPU: demonstrations from agent logs without a GPU -- the restatement itself (tests/demos_ref.py) on hand-built examples, the
closed-population invariant and the recovery of known transition matrices on simulated logs, the descriptor struct against the
C compiler, the new symbols, the workspace size, the refusals of the library and of the Python layers, and the round trip of
Demonstrations.write through the reference's readers."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import demos_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


@pytest.fixture(scope='module')
def lib():
    from discrete_mean_field_game_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib


def ratio(a, b):
    return F32(np.float64(a) / np.float64(b))


# ---------------------------------------------------------------------------------------------------- the restatement
def test_the_tie_rule_is_pythons_stable_sort():
    keys = [3, 5, 3, 0, 5, 0]
    rank = R.rank_by(keys)
    assert np.argsort(rank).tolist() == [1, 4, 0, 2, 3, 5]              # rank -> raw id: equal keys in ascending id, zeros too
    assert rank.tolist() == [2, 0, 3, 4, 1, 5]


def test_a_hand_built_day():
    # 6 agents, 3 hours, 4 categories; hour 0 counts: cat 0: 1, cat 1: 3, cat 2: 2, cat 3: 0 -> order 1, 2, 0, 3
    topic = np.array([[[1, 1, 1, 2, 2, 0],
                       [1, 2, 1, 2, -1, 0],
                       [1, 1, 3, 2, 2, 0]]], np.int32)
    out = R.from_logs(topic, C=4, d=2, width=3)
    assert out['order'].tolist() == [[1, 2, 0, 3]] and out['status'].tolist() == [0]
    assert out['counts'].tolist() == [[[3, 2, 1], [2, 2, 1], [2, 2, 1]]]
    assert out['present'].tolist() == [[6, 5, 5]]
    # hour 0 -> 1 in ranks: 0>0, 0>1, 0>0, 1>1, 1>absent, 2>2; hour 1 -> 2: 0>0, 1>0, 0>absent (category 3: rank 3 >= width), 1>1,
    # absent>1, 2>2
    assert out['moves'][0, 0].tolist() == [[2, 1, 0], [0, 1, 0], [0, 0, 1]]
    assert out['moves'][0, 1].tolist() == [[1, 0, 0], [1, 1, 0], [0, 0, 1]]
    assert out['left'].tolist() == [[[0, 1, 0], [1, 0, 0]]] and out['entered'].tolist() == [[[0, 0, 0], [0, 1, 0]]]
    # width > d: the state is normalised over the recorded width and sliced
    assert R.same(out['state'][0, 0], np.array([ratio(3, 6), ratio(2, 6)], F32)) and out['state'][0, 0].sum() < 1
    assert R.same(out['action'][0, 0], np.array([[ratio(2, 3), ratio(1, 3)], [ratio(0, 1), ratio(1, 1)]], F32))
    assert R.same(out['action'][0, 1], np.array([[ratio(1, 1), ratio(0, 1)], [ratio(1, 2), ratio(1, 2)]], F32))


def test_both_kinds_of_empty_row_and_an_absent_hour():
    # rank 0: two agents that both leave the recorded set at hour 1 (counts > 0, row_total = 0); rank 2: nobody, ever
    given = np.array([[0, 1, 2]])
    topic = np.array([[[0, 0, 1], [-1, -1, 1], [-1, -1, -1]]], np.int32)
    for empty_row, row2 in (('uniform', [ratio(1, 3)] * 3), ('identity', [0, 0, 1])):
        out = R.from_logs(topic, 3, 3, order='given', order_given=given, empty_row=empty_row)
        a = out['action'][0, 0]
        assert a[0].tolist() == [1, 0, 0]                               # its agents all left: identity under either setting
        assert a[1].tolist() == [0, 1, 0] and R.same(a[2], np.array(row2, F32))
        assert out['present'].tolist() == [[3, 1, 0]] and np.isnan(out['state'][0, 2]).all() and out['status'].tolist() == [R.EMPTY_HOUR]
        assert out['left'][0].tolist() == [[2, 0, 0], [0, 1, 0]] and not out['entered'].any()
    assert R.same(F32(np.float64(1) / np.float64(3)), F32(1.0 / 3.0))


def test_bad_values_and_a_given_table():
    topic = np.array([[[0, 1, 2, 7], [0, 1, 2, 2]], [[0, 1, 2, 2], [2, 1, 0, 0]]], np.int32)
    out = R.from_logs(topic, 3, 2, order='given', order_given=np.array([1, -1, 0]))
    assert out['status'].tolist() == [R.BAD_VALUE, 0] and out['order'].tolist() == [[2, 0, -1]] * 2
    assert out['counts'].tolist() == [[[1, 1], [2, 1]], [[2, 1], [1, 2]]]
    out = R.from_logs(topic[1:], 3, 2, order='given', order_given=np.array([[1, 5, 0]]))
    assert out['status'].tolist() == [R.BAD_VALUE] and out['order'].tolist() == [[2, 0, -1]]
    a, b = R.from_logs(topic, 3, 3, order='total'), R.from_logs(topic, 3, 3, order='first_hour')
    assert a['order'].tolist() == [[2, 0, 1]] * 2 and b['order'].tolist() == [[0, 1, 2], [2, 0, 1]]


def test_a_failed_member_in_the_second_mode():
    counts = np.array([[[2, 1], [-1, -1]], [[1, 2], [3, 0]]])
    moves = np.array([[[[-1, -1], [-1, -1]]], [[[1, 0], [2, 0]]]])
    out = R.finish(counts, moves, 2)
    assert out['status'].tolist() == [R.FAILED, 0] and np.isnan(out['state'][0]).all() and np.isnan(out['action'][0]).all()
    assert out['present'].tolist() == [[-1, -1], [3, 3]] and (out['left'][0] == -1).all() and (out['entered'][0] == -1).all()
    assert not out['left'][1].any() and not out['entered'][1].any() and out['action'][1, 0].tolist() == [[1, 0], [1, 0]]


@pytest.fixture(scope='module')
def simulated():
    """Seeds 0..4: U = 200 000, d = 5, H = 9, P rows from Dirichlet(2), pi0 from Dirichlet(5); (P, restatement of the log)."""
    out = []
    for seed in range(5):
        rs = np.random.RandomState(seed)
        P, pi0 = rs.dirichlet(2 * np.ones(5), (8, 5)), rs.dirichlet(5 * np.ones(5))
        topic = R.simulate_logs(P, pi0, 200_000, 9, seed)[None]
        out.append((P, R.from_logs(topic, 5, 5, order='given', order_given=np.arange(5))))
    return out


def test_a_closed_population_neither_loses_nor_gains(simulated):
    for _, out in simulated:
        assert not out['left'].any() and not out['entered'].any() and (out['present'] == 200_000).all() and not out['status'].any()
        assert R.same(out['state'][0, 1:], F32(np.float64(out['moves'][0].sum(-2)) / np.float64(200_000)))


def test_the_transition_matrices_are_recovered(simulated):
    """max |P^ - P| / sqrt(P (1 - P) / row_total) <= 5 over all 200 cells of each seed (measured: 3.35 at most, smallest row
    7 619 agents)."""
    for P, out in simulated:
        row_total = np.float64(out['moves'].sum(-1))[0]
        z = np.abs(np.float64(out['moves'][0]) / row_total[..., None] - P) / np.sqrt(P * (1 - P) / row_total[..., None])
        print('max z %.2f, smallest row %d' % (z.max(), row_total.min()))
        assert z.shape == (8, 5, 5) and z.max() <= 5


# ---------------------------------------------------------------------------------------------------- the C boundary
def test_struct_layout_matches_the_header(lib, tmp_path):
    st, ctype = lib.DemosStruct, 'mfg_demos_t'
    fields = [n for n, _ in st._fields_]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "mfg_hip.h"\nint main(void){printf("%%zu", sizeof(%s));\n' % ctype
    for f in fields:
        src += 'printf(" %%zu", offsetof(%s, %s));\n' % (ctype, f)
    src += 'return 0;}\n'
    c = tmp_path / 'layout.c'
    c.write_text(src)
    exe = str(tmp_path / 'layout')
    subprocess.run(['gcc', '-std=c99', '-I', os.path.join(ROOT, 'include'), str(c), '-o', exe], check=True)
    out = [int(x) for x in subprocess.run([exe], check=True, stdout=subprocess.PIPE).stdout.decode().split()]
    assert out[0] == C.sizeof(st)
    assert out[1:] == [getattr(st, f).offset for f in fields]
    text = open(os.path.join(ROOT, 'include', 'mfg_hip.h')).read()
    body = re.search(r'typedef struct \w+ \{([^}]*)\} %s;' % ctype, text).group(1)
    assert len(re.findall(r'[\w\]]\s*[,;]', body)) == len(fields)


def test_the_new_symbols_are_declared_bound_and_exported(lib):
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'mfg_hip.h')).read(), flags=re.S)
    h = lib.lib()
    for name in ('mfg_demos_from_logs', 'mfg_demos_workspace_bytes'):
        assert re.search(r'\b%s\s*\(' % name, text) and name in lib.SIGNATURES and getattr(h, name) is not None
    assert not re.search(r'mfg_demos_from_logs\s*\([^)]*mfg_stream_t', text)
    for macro, value in (('MAX_C', lib.DEMOS_MAX_C), ('CHUNK', lib.DEMOS_CHUNK), ('BAD_VALUE', lib.DEMOS_BAD_VALUE),
                         ('EMPTY_HOUR', lib.DEMOS_EMPTY_HOUR), ('FAILED', lib.DEMOS_FAILED)):
        assert int(re.search(r'#define MFG_DEMOS_%s (\d+)' % macro, text).group(1)) == value
    for table, prefix in ((lib.DEMOS_ORDERS, 'ORDER'), (lib.DEMOS_EMPTY_ROWS, 'EMPTY'), (lib.DEMOS_LDS_UPDATES, 'LDS')):
        for word, value in table.items():
            assert int(re.search(r'#define MFG_DEMOS_%s_%s (\d+)' % (prefix, word.upper()), text).group(1)) == value
    assert (R.BAD_VALUE, R.EMPTY_HOUR, R.FAILED) == (lib.DEMOS_BAD_VALUE, lib.DEMOS_EMPTY_HOUR, lib.DEMOS_FAILED)
    assert h.mfg_abi_version() == 18


def test_workspace_size(lib):
    h = lib.lib()
    up = lambda b: (b + 255) // 256 * 256
    want = lambda N, H, Cc, w: up(N * Cc * 8) + up(N * Cc * 4) + up(N * H * w * 4) + up(N * (H - 1) * w * w * 4)
    for shape in ((1, 2, 1, 1), (24, 16, 47, 20), (3, 5, 4096, 64), (70_000, 2, 5, 3)):
        assert h.mfg_demos_workspace_bytes(*shape) == want(*shape)
    for shape in ((0, 2, 5, 3), (1, 1, 5, 3), (1, 2, 0, 1), (1, 2, 4097, 3), (1, 2, 5, 0), (1, 2, 5, 6), (1, 2, 100, 65)):
        assert h.mfg_demos_workspace_bytes(*shape) == 0


def _desc(lib, ws_bytes=None, log=True, **kw):
    """A descriptor whose device pointers are dummies: every refusal below happens before anything is launched or read."""
    f = lib.DemosStruct()
    for name in ('topic', 'state', 'action', 'counts', 'moves', 'order', 'present', 'left', 'entered', 'status', 'workspace'):
        setattr(f, name, 4096)
    if not log:
        f.topic = None
    f.U, f.N, f.H, f.C, f.d, f.width = 100, 2, 3, 5, 3, 3
    for name, value in kw.items():
        setattr(f, name, value)
    need = lib.lib().mfg_demos_workspace_bytes(f.N, f.H, f.C, f.width)
    f.workspace_bytes = need if ws_bytes is None else ws_bytes
    return f


@pytest.mark.parametrize('why,code,kw', [
    ('N = 0', -1, dict(N=0)), ('H = 1', -1, dict(H=1)), ('U = 0', -1, dict(U=0)), ('U = 2^31', -1, dict(U=2 ** 31)),
    ('C = 0', -1, dict(C=0)), ('C = 4097', -1, dict(C=4097)), ('d = 0', -1, dict(d=0)), ('d > width', -1, dict(d=4)),
    ('width > C', -1, dict(width=6, d=3)), ('order 3', -1, dict(order_mode=3)), ('order -1', -1, dict(order_mode=-1)),
    ('empty_row 2', -1, dict(empty_row=2)), ('lds_update 2', -1, dict(lds_update=2)), ('groups -1', -1, dict(groups=-1)), ('given without a table', -1, dict(order_mode=2)),
    ('given with 3 rows of 2 days', -1, dict(order_mode=2, order_given=4096, order_given_rows=3)),
    ('null order', -1, dict(order=None)), ('null status', -1, dict(status=None)), ('null workspace', -1, dict(workspace=None)),
    ('workspace misaligned', -1, dict(workspace=4100)), ('width = 65', -3, dict(C=100, width=65)),
    ('second mode: null counts', -1, dict(log=False, counts=None)), ('second mode: null moves', -1, dict(log=False, moves=None)),
    ('second mode: d > width', -1, dict(log=False, d=4)), ('second mode: H = 1', -1, dict(log=False, H=1)),
    ('second mode: width = 65', -3, dict(log=False, width=65))])
def test_the_library_refuses_before_it_launches(lib, why, code, kw):
    kw = dict(kw)
    f = _desc(lib, log=kw.pop('log', True), **kw)
    assert lib.lib().mfg_demos_from_logs(C.byref(f)) == code, why        # MFG_EINVAL -1, MFG_EUNSUPPORTED -3


def test_the_library_names_the_bytes_of_a_short_workspace(lib):
    h = lib.lib()
    assert h.mfg_demos_from_logs(None) == -1
    need = h.mfg_demos_workspace_bytes(2, 3, 5, 3)
    f = _desc(lib, ws_bytes=need - 1)
    assert h.mfg_demos_from_logs(C.byref(f)) == -1 and (b'need %d bytes' % need) in h.mfg_last_error()


# ---------------------------------------------------------------------------------------------------- the Python layers
def test_ops_argument_rules_and_shapes():
    from discrete_mean_field_game_amd import ops
    assert ops.check_demos_args((2, 3, 100), 5, 3) == (2, 3, 100, 5, 3, 3)
    assert ops.check_demos_args((2, 3, 100), 47, 15, 20, 'given', (1, 47), 'identity') == (2, 3, 100, 47, 15, 20)
    for shape, args in (((2, 3), (5, 3)), ((0, 3, 100), (5, 3)), ((2, 1, 100), (5, 3)), ((2, 3, 0), (5, 3)), ((2, 3, 2 ** 31), (5, 3)),
                        ((2, 3, 100), (0, 1)), ((2, 3, 100), (4097, 3)), ((2, 3, 100), (5, 0)), ((2, 3, 100), (5, 4, 3)),
                        ((2, 3, 100), (5, 3, 6)), ((2, 3, 100), (100, 3, 65)), ((2, 3, 100), (5, 3, None, 'popular')),
                        ((2, 3, 100), (5, 3, None, 'given')), ((2, 3, 100), (5, 3, None, 'given', (3, 5))),
                        ((2, 3, 100), (5, 3, None, 'total', (2, 5))), ((2, 3, 100), (5, 3, None, 'total', None, 'zero')),
                        ((2, 3, 100), (5, 3, None, 'total', None, 'uniform', 'fast'))):
        with pytest.raises(ValueError):
            ops.check_demos_args(shape, *args)
    torch = pytest.importorskip('torch')
    shapes = ops.demos_shapes(2, 3, 47, 15, 20)
    assert {n: s for n, (s, _) in shapes.items()} == {
        'state': (2, 3, 15), 'action': (2, 2, 15, 15), 'counts': (2, 3, 20), 'moves': (2, 2, 20, 20), 'order': (2, 47),
        'present': (2, 3), 'left': (2, 2, 20), 'entered': (2, 2, 20), 'status': (2,)}
    assert all((t == torch.float32) == (n in R.FLOAT_OUTPUTS) for n, (_, t) in shapes.items()) and set(shapes) == set(ops.DEMOS_OUTPUTS)
    assert ops.check_demos_moves_args((6, 2, 21), (6, 1, 21, 21)) == (6, 2, 21, 21)
    for c, m, d in (((6, 2), (6, 1, 21, 21), None), ((6, 1, 21), (6, 0, 21, 21), None), ((6, 2, 21), (6, 2, 21, 21), None),
                    ((6, 2, 21), (6, 1, 21, 21), 22), ((6, 2, 65), (6, 1, 65, 65), None)):
        with pytest.raises(ValueError):
            ops.check_demos_moves_args(c, m, d)


def test_demos_argument_rules():
    from discrete_mean_field_game_amd import demos as D
    import discrete_mean_field_game_amd as pkg
    assert pkg.demos is D and 'demos' in pkg.__all__
    assert D.check_from_logs_args((2, 3, 100), 3, 5) == (2, 3, 100, 5, 3, 3)
    assert D.check_from_logs_args((2, 100, 3), 3, 5, layout='nuh') == (2, 3, 100, 5, 3, 3)
    for shape, kw in (((2, 3, 100), dict(layout='hun')), ((3, 100), {}), ((2, 100, 1), dict(layout='nuh')), ((2, 3, 100), dict(width=6)),
                      ((2, 3, 100), dict(order='popular')), ((2, 3, 100), dict(empty_row='zero'))):
        with pytest.raises(ValueError):
            D.check_from_logs_args(shape, 3, 5, **kw)
    out = R.from_logs(np.array([[[0, 1, 1], [1, 1, 0]]], np.int32), 2, 2)
    dm = D.Demonstrations(out, 2, 2)
    assert (dm.N, dm.H) == (1, 2) and dm.closed().tolist() == [True]
    with pytest.raises(ValueError):
        D.Demonstrations(out, 2, 3)
    with pytest.raises(ValueError):
        dm.pi0([1])


# ---------------------------------------------------------------------------------------------------- the reference's files
def through_text(a):
    return np.array([float('%.3e' % x) for x in np.asarray(a).ravel()]).reshape(np.shape(a))


def test_written_files_read_back_through_the_references_readers(tmp_path):
    from discrete_mean_field_game_amd import demos as D
    from discrete_mean_field_game_amd.ac_irl import AC_IRL
    from discrete_mean_field_game_amd.mfg_ac2 import actor_critic
    d, width, Cn, H, N, U = 3, 5, 7, 16, 3, 400
    rs = np.random.RandomState(3)
    topic = rs.choice(Cn + 1, size=(N, H, U), p=[.3, .2, .15, .1, .1, .05, .05, .05]).astype(np.int32) - 1    # -1: absent
    topic[1, 4][topic[1, 4] == topic[1, 0, 0]] = -1                    # an hour with an emptied category: an empty row
    out = R.from_logs(topic, Cn, d, width)
    dm = D.Demonstrations(out, d, width)
    state_dir, action_dir = str(tmp_path / 'states'), str(tmp_path / 'actions')
    dm.write(state_dir, action_dir, start_day=1)
    assert sorted(os.listdir(state_dir)) == ['trend_distribution_day%d.csv' % n for n in (1, 2, 3)]
    lines = open(os.path.join(action_dir, 'action_day2.txt')).read().split('\n')
    assert len(lines) == 15 * width + 14 + 1 and lines[width] == '' and len(lines[0].split(' ')) == width and lines[-1] == ''
    assert len(open(os.path.join(state_dir, 'trend_distribution_day1.csv')).readline().split(' ')) == width
    reader = AC_IRL.__new__(AC_IRL)
    reader.d = d
    trajs = reader.read_demonstrations(state_dir, action_dir, dim_action=width, start_day=1)
    want = dm.demonstrations()
    assert len(trajs) == N and all(len(t) == 15 for t in trajs) and len(want[0]) == H - 1
    for got_day, want_day in zip(trajs, want):
        for (gs, ga), (ws, wa) in zip(got_day, want_day):
            assert np.array_equal(gs, through_text(ws)) and np.array_equal(ga, through_text(wa))
    ac = actor_critic.__new__(actor_critic)
    ac.d, ac.device = d, 'cpu'
    ac.init_pi0(state_dir)
    assert np.array_equal(ac.mat_pi0, through_text(dm.pi0())) and dm.emp().shape == (N, H, d) and dm.emp().dtype == np.float64
    full_state, full_action = dm.full_rows()
    assert R.same(full_state[..., :d], out['state']) and R.same(full_action[..., :d, :d], out['action'])
