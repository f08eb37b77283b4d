"""CPU checks of the mixed IRL population (the calls that take a geometry table, AC_IRLPopulation(mixed_nets=True), gridsearch): declared in
the header, bound in _lib.SIGNATURES, exported by the library; the geometry struct's layout; the per-learner row layout; the
argument checks; the grid order and the CSV lines of gridsearch on a stubbed population."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NETS = ('mfg_train_episodes_irl_pop', 'mfg_train_rollouts_irl_pop', 'mfg_reward_net_forward_pop', 'mfg_reward_net_train_steps_pop')
M4 = (('dropout', 4, 4), ('l1l2', 8, 6), ('dropout_l1l2', 16, 32), ('none', 6, 8))


@pytest.fixture(scope='module')
def lib():
    from discrete_mean_field_game_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib


def _header():
    return re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'mfg_hip.h')).read(), flags=re.S)


def test_declared_bound_and_exported(lib):
    text = _header()
    for name in NETS:
        assert re.search(r'\b%s\s*\(' % name, text), name
        assert name in lib.SIGNATURES
        assert getattr(lib.lib(), name) is not None


def test_argument_counts_match_header(lib):
    text = _header()
    for name in NETS:
        decl = re.search(r'\b%s\s*\(([^;]*)\);' % name, text, flags=re.S).group(1)
        args = decl.split(',')
        assert len(args) == len(lib.SIGNATURES[name][1]), name
        assert sum('mfg_rn_geom_t' in a for a in args) == 2, name      # the host copy and the device copy


def test_abi_version_unchanged(lib):
    assert lib.lib().mfg_abi_version() == 18


def test_geom_struct_layout_matches_the_header(lib, tmp_path):
    """mfg_rn_geom_t crosses the boundary by pointer (host table) and is read by the kernels (device table): the ctypes mirror
    must have the C compiler's size and field offsets, and the size the kernels' 16-byte scalar load assumes."""
    fields = [n for n, _ in lib.RnGeomStruct._fields_]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "mfg_hip.h"\nint main(void){printf("%zu", sizeof(mfg_rn_geom_t));\n'
    for f in fields:
        src += 'printf(" %%zu", offsetof(mfg_rn_geom_t, %s));\n' % f
    src += 'return 0;}\n'
    c = tmp_path / 'layout.c'
    c.write_text(src)
    exe = str(tmp_path / 'layout')
    subprocess.run(['gcc', '-std=c99', '-I', os.path.join(ROOT, 'include'), str(c), '-o', exe], check=True)
    out = [int(x) for x in subprocess.run([exe], check=True, stdout=subprocess.PIPE).stdout.decode().split()]
    assert out[0] == C.sizeof(lib.RnGeomStruct) == 16
    assert out[1:] == [getattr(lib.RnGeomStruct, f).offset for f in fields]


def test_geom_table_holds_the_entries(lib):
    pytest.importorskip('torch')
    from discrete_mean_field_game_amd import ops
    host, dev = ops.rn_geom_table([(4, 4, 0.4, False), (16, 32, 1.0, True)])
    assert dev is None and host.dtype.itemsize == 16 and host.shape == (2,)
    raw = (lib.RnGeomStruct * 2).from_buffer_copy(host.tobytes())
    assert (raw[0].n3, raw[0].n4, raw[0].l1l2) == (4, 4, 0) and raw[0].keep_prob == np.float32(0.4)
    assert (raw[1].n3, raw[1].n4, raw[1].keep_prob, raw[1].l1l2) == (16, 32, 1.0, 1)


@pytest.mark.parametrize('d', [15, 21])
def test_row_offsets_are_the_single_layout(lib, d):
    """Learner k's tensors sit at mfg_reward_net_param_offsets of ITS geometry in its row; fc3_w is 8-byte aligned in every
    row of a buffer whose rows are PARAM_ALIGN floats apart."""
    pytest.importorskip('torch')
    from discrete_mean_field_game_amd import irl_population as ip
    from discrete_mean_field_game_amd.networks import RewardNet
    rows = []
    for reg, n3, n4 in M4:
        offs = (C.c_int64 * 11)()
        assert lib.lib().mfg_reward_net_param_offsets(d, 5, 2, 3, n3, n4, offs) == 0
        got = ip.net_row_offsets(d, n3, n4)
        assert got == [int(o) for o in offs]
        net = RewardNet(d=d, reg=reg, n_fc3=n3, n_fc4=n4)
        sizes = [net.get_parameter(pname).numel() for _, pname in ip.NET_TENSORS]
        assert [got[i + 1] - got[i] for i in range(10)] == sizes
        assert got[10] == lib.lib().mfg_reward_net_num_params(d, 5, 2, 3, n3, n4) == sum(sizes)
        assert got[:5] == [0, 25, 26, 44, 46]          # the first five offsets do not depend on n3 / n4
        rows.append(got)
    stride = (max(r[10] for r in rows) + ip.PARAM_ALIGN - 1) // ip.PARAM_ALIGN * ip.PARAM_ALIGN
    assert stride >= rows[2][10] and max(r[10] for r in rows) == rows[2][10]
    for k, r in enumerate(rows):
        assert ((k * stride + r[4]) * 4) % 8 == 0


def _net(**kw):
    from discrete_mean_field_game_amd.networks import RewardNet
    return RewardNet(**kw)


def test_net_geometries_and_limits():
    pytest.importorskip('torch')
    from discrete_mean_field_game_amd import ops
    nets = [_net(d=21, reg=reg, n_fc3=n3, n_fc4=n4) for reg, n3, n4 in M4]
    d, geoms = ops.irl_pop_net_geometries(nets)
    assert d == 21
    assert geoms == [(4, 4, 0.4, False), (8, 6, 1.0, True), (16, 32, 0.4, True), (6, 8, 1.0, False)]
    assert ops.irl_pop_net_geometries([_net(d=15, n_fc3=1, n_fc4=1)]) == (15, [(1, 1, 0.4, True)])
    for bad in (dict(n_fc3=17), dict(n_fc4=33), dict(k1=3), dict(k2=5), dict(f2=1), dict(f1=2), dict(keep_prob=0.0),
                dict(keep_prob=1.5)):
        with pytest.raises(ValueError):
            ops.irl_pop_net_geometries([_net(d=21), _net(d=21, **bad)])
    with pytest.raises(ValueError):
        ops.irl_pop_net_geometries([_net(d=21), _net(d=15)])
    with pytest.raises(ValueError):
        ops.irl_pop_net_geometries([_net(d=16)])
    with pytest.raises(ValueError):
        ops.irl_pop_net_geometries([])
    # the shared-geometry helper still refuses a mixed list
    with pytest.raises(ValueError):
        ops.irl_pop_net_geometry(nets)


def test_check_args_mixed():
    pytest.importorskip('torch')
    from discrete_mean_field_game_amd.irl_population import check_args, check_args_mixed
    nets = [_net(d=15, reg=reg, n_fc3=n3, n_fc4=n4) for reg, n3, n4 in M4]
    got, geoms = check_args_mixed(4, 15, 32, 'step', 'mixed', nets)
    assert len(got) == 4 and [g[:2] for g in geoms] == [(4, 4), (8, 6), (16, 32), (6, 8)]
    with pytest.raises(ValueError):
        check_args(4, 15, 32, 'step', 'mixed', nets)               # without the flag a mixed list is refused
    for kw in (dict(reward_nets=nets[0]), dict(reward_nets=nets[:3]), dict(reward_nets=nets[:3] + [_net(d=15, n_fc3=17)]),
               dict(reward_nets=nets[:3] + [_net(d=15, n_fc4=33)]), dict(reward_nets=nets[:3] + [_net(d=15, k1=3)]),
               dict(reward_nets=nets[:3] + [_net(d=21)]), dict(d=21), dict(batch=1), dict(update_every='episode'),
               dict(precision='f32'), dict(reward_nets=nets[:3] + [object()])):
        args = dict(K=4, d=15, batch=32, update_every='step', precision='mixed', reward_nets=nets)
        args.update(kw)
        with pytest.raises(ValueError):
            check_args_mixed(**args)


def test_mixed_population_needs_a_gpu_but_checks_first():
    torch = pytest.importorskip('torch')
    from discrete_mean_field_game_amd.irl_population import AC_IRLPopulation
    nets = [_net(d=15, reg=reg, n_fc3=n3, n_fc4=n4) for reg, n3, n4 in M4]
    with pytest.raises(ValueError):
        AC_IRLPopulation([8.0] * 4, d=15, batch=32, reward_nets=nets)                       # mixed by mistake
    with pytest.raises(ValueError):
        AC_IRLPopulation([8.0] * 4, d=15, batch=32, reward_nets=nets[0], mixed_nets=True)   # one shared network
    if not torch.cuda.is_available():
        from discrete_mean_field_game_amd._lib import MfgError
        with pytest.raises(MfgError):
            AC_IRLPopulation([8.0] * 4, d=15, batch=32, reward_nets=nets, mixed_nets=True,
                             pi0=np.full((2, 15), 1.0 / 15))


class _StubPopulation:
    """What gridsearch needs of AC_IRLPopulation, without a GPU; records how it was built."""
    last = None

    def __init__(self, thetas, shifts, alpha_scales, d, **kw):
        self.thetas0, self.shifts, self.alpha_scales, self.d, self.kw = list(thetas), shifts, alpha_scales, d, kw
        self.calls = []
        _StubPopulation.last = self

    def outerloop(self, **kw):
        self.calls.append(('outerloop', kw))
        return np.array([t + 0.125 * p for p, t in enumerate(self.thetas0)])

    def test_reward_network(self):
        self.calls.append(('test_reward_network', {}))
        K = len(self.thetas0)
        out = np.empty((K, 3))
        out[:, 0] = [0.5 + 0.001 * p for p in range(K)]
        out[:, 1] = np.nan if self.kw.get('demonstrations_test') is None else [-0.25 - 0.01 * p for p in range(K)]
        out[:, 2] = [1e-7 * (p + 1) for p in range(K)]
        return out


def test_gridsearch_order_and_csv_on_a_stub(monkeypatch, tmp_path):
    torch = pytest.importorskip('torch')
    from discrete_mean_field_game_amd import irl_population as ip
    from discrete_mean_field_game_amd.networks import RewardNet
    monkeypatch.setattr(ip, 'AC_IRLPopulation', _StubPopulation)
    # the reference's 27 points: reg outermost, n_fc4 innermost
    pts = ip.gridsearch_points(('dropout', 'l1l2', 'dropout_l1l2'), range(4, 10, 2), range(4, 10, 2))
    assert len(pts) == 27 and pts[0] == ('dropout', 4, 4) and pts[1] == ('dropout', 4, 6) and pts[3] == ('dropout', 6, 4)
    assert pts[9] == ('l1l2', 4, 4) and pts[26] == ('dropout_l1l2', 8, 8)
    out = tmp_path / 'results' / 'grid.csv'
    torch.manual_seed(123)
    state = torch.random.get_rng_state()
    rows = ip.gridsearch(('dropout', 'l1l2'), (4, 6), (4,), demonstrations=['demo'], demonstrations_test=['test'], d=15, batch=32,
                         seed=40, net_seed=7, outfile=str(out), outerloop_kwargs=dict(num_iterations=1, final_training=False))
    assert torch.equal(torch.random.get_rng_state(), state)          # the caller's generator is left alone
    stub = _StubPopulation.last
    assert stub.thetas0 == [6.5] * 4 and stub.shifts == 0 and stub.alpha_scales == 1e4 and stub.d == 15
    kw = stub.kw
    assert kw['mixed_nets'] is True and kw['seeds'] == [40, 41, 42, 43] and kw['host_seeds'] == [40, 41, 42, 43]
    assert kw['batch'] == 32 and kw['demonstrations'] == ['demo'] and kw['demonstrations_test'] == ['test']
    assert kw['update_every'] == 'step' and kw['precision'] == 'mixed'
    points = [('dropout', 4, 4), ('dropout', 6, 4), ('l1l2', 4, 4), ('l1l2', 6, 4)]
    for p, (net, (reg, n3, n4)) in enumerate(zip(kw['reward_nets'], points)):
        assert (net.reg, net.fc3.out_features, net.fc4.out_features, net.d) == (reg, n3, n4, 15)
        with torch.random.fork_rng(devices=[]):
            torch.manual_seed(7 + p)
            ref = RewardNet(15, reg, n_fc3=n3, n_fc4=n4)
        for a, b in zip(net.parameters(), ref.parameters()):
            assert torch.equal(a, b)
    assert stub.calls == [('outerloop', dict(num_iterations=1, final_training=False)), ('test_reward_network', {})]
    lines = out.read_text().splitlines(keepends=True)
    assert lines[0] == 'reg,n_fc3,n_fc4,reward_demo_avg_train,reward_demo_avg_test,reward_gen_avg,theta\n'
    assert lines[1] == 'dropout,4,4,0.500000,-0.250000,0.000000,6.500000\n'
    assert lines[4] == 'l1l2,6,4,0.503000,-0.280000,0.000000,6.875000\n'
    assert len(lines) == 5
    assert [r[:3] for r in rows] == points and rows[3][3:] == (0.503, -0.28, 4e-7, 6.875)
    for p, row in enumerate(rows):
        assert lines[1 + p] == '%s,%d,%d,%f,%f,%f,%f\n' % row
    # a second sweep appends below, without a second header; no test set: nan, as '%f' prints it
    rows2, pop2 = ip.gridsearch(('none',), (8,), (4,), demonstrations=['demo'], batch=8, outfile=str(out), return_population=True)
    assert pop2 is _StubPopulation.last and pop2.calls[0] == ('outerloop', {})
    lines = out.read_text().splitlines(keepends=True)
    assert len(lines) == 6 and lines[5] == 'none,8,4,0.500000,nan,0.000000,6.500000\n'
    assert np.isnan(rows2[0][4])
    # no file on request, and an empty grid is refused
    before = sorted(os.listdir(str(tmp_path / 'results')))
    ip.gridsearch(('none',), (8,), (4,), demonstrations=['demo'], batch=8, outfile=None)
    assert sorted(os.listdir(str(tmp_path / 'results'))) == before
    with pytest.raises(ValueError):
        ip.gridsearch((), (8,), (4,), demonstrations=['demo'], batch=8, outfile=None)


# ------------------------------------------------------------------ the optional table of the four population calls
EINVAL, EUNSUPPORTED = -1, -3
REMOVED = tuple(base + suffix for base, suffixes in (('mfg_train_episodes_irl_pop', ('_calls', '_nets')),
                                                     ('mfg_train_rollouts_irl_pop', ('_calls', '_nets')),
                                                     ('mfg_reward_net_forward_pop', ('_nets',)),
                                                     ('mfg_reward_net_train_steps_pop', ('_nets',))) for suffix in suffixes)


def test_suffixed_entry_points_are_gone(lib):
    text = open(os.path.join(ROOT, 'include', 'mfg_hip.h')).read()
    for name in REMOVED:
        assert name not in text, name
        assert name not in lib.SIGNATURES, name
        assert not hasattr(lib.lib(), name), name
    assert lib.lib().mfg_abi_version() == 18


def _table_calls(lib, d=15, K=4):
    """The four calls as functions of (geom_host, geom_dev, per_learner_net, stride) over dummy pointers: a refusal of the
    table comes before anything dereferences them or reaches the GPU."""
    h = lib.lib()
    p = C.c_void_p(16)
    net = lib.RewardNetStruct()
    net.k1, net.f2, net.k2, net.n3, net.n4, net.keep_prob = 5, 2, 3, 16, 32, 1.0
    for f in ('conv1_w', 'conv1_b', 'conv2_w', 'conv2_b', 'fc3_w', 'fc3_b', 'fc4_w', 'fc4_b', 'out_w', 'out_b'):
        setattr(net, f, 16)
    lr = np.array([0, 2], dtype=np.int32)
    ky = np.array([1, 2], dtype=np.uint64)
    plan = np.zeros(1, dtype=np.dtype(lib.RnTrainPlan))
    keep = (net, lr, ky, plan)

    def episodes(gh, gd, per, stride):
        return h.mfg_train_episodes_irl_pop(p, 4, p, p, 32, K, d, 3, 1, 1, 0, p, p, p, p, 1.0, p, 0, 0, 1, p, p, C.byref(net), per,
                                            stride, gh, gd, p, p, p, p, p, p, p, None, p, 1 << 20, None)

    def rollouts(gh, gd, per, stride):
        return h.mfg_train_rollouts_irl_pop(p, 4, 32, K, d, 3, 1, 1, 0, p, p, p, p, 1.0, p, 0, 0, 0, p, p, C.byref(net), per, stride,
                                            gh, gd, p, p, p, None, p, p, p, p, p, None, p, 1 << 20, None)

    def forward(gh, gd, per, stride):
        return h.mfg_reward_net_forward_pop(p, p, 8 * d, 8 * d * d, 8, d, C.byref(net), per, stride, gh, gd, K, lr.ctypes.data,
                                            ky.ctypes.data, 2, 0, p, p, 128, None)

    def steps(gh, gd, per, stride):      # (no per_learner_net here: the rows are always per learner)
        return h.mfg_reward_net_train_steps_pop(p, p, p, stride, K, d, 5, 2, 3, 16, 32, gh, gd, p, p, 6, p, p, 6, plan.ctypes.data,
                                                p, 0, 1, 1, 5, 5, 15, 5, 1.0, 0, 0.9, 0.999, 1e-8, p, p, 128, None)
    return (episodes, rollouts, forward, steps), keep


def test_one_copy_of_the_table_is_refused(lib):
    pytest.importorskip('torch')
    from discrete_mean_field_game_amd import ops
    d, K = 15, 4
    host, _ = ops.rn_geom_table([(n3, n4, 1.0 if 'dropout' not in reg else 0.4, 'l1l2' in reg) for reg, n3, n4 in M4])
    stride = (int(lib.lib().mfg_reward_net_num_params(d, 5, 2, 3, 16, 32)) + 63) // 64 * 64
    calls, _keep = _table_calls(lib, d, K)
    for call in calls:
        assert call(host.ctypes.data, None, 1, stride) == EINVAL, call.__name__
        assert b'both copies' in lib.lib().mfg_last_error(), call.__name__
        assert call(None, C.c_void_p(16), 1, stride) == EINVAL, call.__name__
        assert b'both copies' in lib.lib().mfg_last_error(), call.__name__


def test_table_refusals_through_the_unified_calls(lib):
    """What the calls with a table refused under their own names they refuse with the same codes now: per_learner_net = 0, a
    stride below the largest NP_k, an entry with n3 = 17, keep_prob = 0 -- from the host copy alone, before the device copy
    (a dummy pointer here) is handed to a kernel."""
    pytest.importorskip('torch')
    from discrete_mean_field_game_amd import ops
    d, K = 15, 4
    geoms = [(n3, n4, 1.0 if 'dropout' not in reg else 0.4, 'l1l2' in reg) for reg, n3, n4 in M4]
    good, _ = ops.rn_geom_table(geoms)
    np_max = int(lib.lib().mfg_reward_net_num_params(d, 5, 2, 3, 16, 32))
    stride = (np_max + 63) // 64 * 64
    dev = C.c_void_p(16)

    def table(k, **kw):
        host = good.copy()
        for f, val in kw.items():
            host[k][f] = val
        return host
    calls, _keep = _table_calls(lib, d, K)
    for call in calls:
        if call.__name__ != 'steps':
            assert call(good.ctypes.data, dev, 0, stride) == EINVAL, call.__name__
            assert b'per_learner_net = 1' in lib.lib().mfg_last_error()
        assert call(good.ctypes.data, dev, 1, np_max - 1) == EINVAL, call.__name__
        assert b'below the largest parameter count' in lib.lib().mfg_last_error()
        bad = table(1, n3=17)
        assert call(bad.ctypes.data, dev, 1, stride) == EUNSUPPORTED, call.__name__
        bad = table(2, keep_prob=0.0)
        assert call(bad.ctypes.data, dev, 1, stride) == EINVAL, call.__name__
        assert b'keep_prob' in lib.lib().mfg_last_error()
