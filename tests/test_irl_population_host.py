"""CPU checks of the IRL population (mfg_train_episodes_irl_pop / mfg_train_rollouts_irl_pop, AC_IRLPopulation): declared in
the header, bound in _lib.SIGNATURES, exported by the library; the class's argument checks and the ops wrappers refuse what the
kernels do not serve before any call."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IRL_POP = ('mfg_train_episodes_irl_pop', 'mfg_train_rollouts_irl_pop')


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
    for name in IRL_POP:
        assert re.search(r'\b%s\s*\(' % name, text), name
        assert name in lib.SIGNATURES
        assert getattr(lib.lib(), name) is not None


def test_argument_counts_match_header(lib):
    text = _header()
    for name in IRL_POP:
        decl = re.search(r'\b%s\s*\(([^;]*)\);' % name, text, flags=re.S).group(1)
        assert len(decl.split(',')) == len(lib.SIGNATURES[name][1]), name


def test_abi_version_unchanged(lib):
    assert lib.lib().mfg_abi_version() == 18


def _net(**kw):
    from discrete_mean_field_game_amd.networks import RewardNet
    return RewardNet(**kw)


def _args(**kw):
    args = dict(K=3, d=21, batch=256, update_every='step', precision='mixed', reward_nets=None)
    args.update(kw)
    if args['reward_nets'] is None:
        args['reward_nets'] = _net(d=args['d'])
    return args


def test_check_args_accepts_shared_and_per_learner_nets():
    pytest.importorskip('torch')
    from discrete_mean_field_game_amd.irl_population import check_args
    assert len(check_args(**_args())) == 1
    assert len(check_args(**_args(reward_nets=[_net(d=21, n_fc3=16) for _ in range(3)]))) == 3
    assert len(check_args(**_args(d=15, update_every='rollout', precision='f64', reward_nets=_net(d=15)))) == 1


@pytest.mark.parametrize('case', ['K0', 'geometry', 'dropout', 'keep', 'd', 'fc3', 'count', 'net_d', 'batch', 'mode',
                                  'precision', 'k2'])
def test_check_args_refuses(case):
    pytest.importorskip('torch')
    from discrete_mean_field_game_amd.irl_population import check_args
    kw = {'K0': dict(K=0),
          'geometry': dict(reward_nets=[_net(d=21, n_fc3=8), _net(d=21, n_fc3=4), _net(d=21, n_fc3=8)]),
          'dropout': dict(reward_nets=[_net(d=21), _net(d=21, reg='l1l2'), _net(d=21)]),
          'keep': dict(reward_nets=[_net(d=21), _net(d=21, keep_prob=1.0), _net(d=21)]),
          'd': dict(d=16, reward_nets=_net(d=16)),
          'fc3': dict(reward_nets=_net(d=21, n_fc3=17)),
          'count': dict(reward_nets=[_net(d=21), _net(d=21)]),
          'net_d': dict(reward_nets=_net(d=15)),
          'batch': dict(batch=1),
          'mode': dict(update_every='episode'),
          'precision': dict(precision='half'),
          'k2': dict(reward_nets=_net(d=21, k2=5))}[case]
    with pytest.raises(ValueError):
        check_args(**_args(**kw))


def test_ops_wrappers_refuse_host_tensors_and_wrong_lengths(lib):
    torch = pytest.importorskip('torch')
    from discrete_mean_field_game_amd import ops
    K, B, d, T = 2, 32, 21, 15
    F = 21 * 22 // 2 + 22
    st = lib.RewardNetStruct()
    st.n3 = 8
    host = dict(dtype=torch.float32)
    # host tensors: refused before the library is called
    with pytest.raises(ValueError):
        ops.train_episodes_irl_pop(torch.zeros(4, d, **host), torch.zeros(K, B, d, **host), T, 1, 1, 0,
                                   torch.zeros(K, dtype=torch.float64), None, None, torch.zeros(K, F, dtype=torch.float64), 1.0,
                                   None, None, None, st, 0, None, 0, torch.zeros(K, F + 3, dtype=torch.float64), None,
                                   {'P': torch.zeros(K, B, d, d, **host)})
    with pytest.raises(ValueError):
        ops.train_rollouts_irl_pop(torch.zeros(4, d, **host), T, 1, 1, 0, torch.zeros(K, dtype=torch.float64), None, None,
                                   torch.zeros(K, F, dtype=torch.float64), 1.0, None, None, None, st, 0, None, 0,
                                   torch.zeros(K, F + 3, dtype=torch.float64), None,
                                   {'pi_traj': torch.zeros(K, B, T + 1, d, **host), 'P': torch.zeros(K, B, T, d, d, **host)})
    # per-learner arrays of the wrong length / on the host
    with pytest.raises(ValueError):
        ops._chk_pop(K, 'rn_seeds', torch.zeros(K + 1, dtype=torch.int64), torch.int64)
    with pytest.raises(ValueError):
        ops._chk_pop(K, 'shifts', torch.zeros(K, dtype=torch.float64), torch.float64)


@pytest.mark.parametrize('case', ['d', 'fc3', 'k1', 'n4'])
def test_net_geometry_refusals(case):
    pytest.importorskip('torch')
    from discrete_mean_field_game_amd import ops
    net = {'d': _net(d=16), 'fc3': _net(d=15, n_fc3=20), 'k1': _net(d=21, k1=3), 'n4': _net(d=21, n_fc4=33)}[case]
    with pytest.raises(ValueError):
        ops.irl_pop_net_geometry([net])
    assert ops.irl_pop_net_geometry([_net(d=15, n_fc3=16)])[:3] == (15, 16, 4)


def test_workspace_slice_covers_both_flows(lib):
    pytest.importorskip('torch')
    from discrete_mean_field_game_amd import ops
    for B in (10, 64, 1000, 4096):
        for d in (15, 21):
            sb = ops.irl_pop_workspace_slice(B, d, 15)
            FO = d * (d + 1) // 2 + d + 1 + 3
            rows = min((B + 15) // 16, 256)
            assert sb % 256 == 0
            assert sb >= 64 + rows * (FO + 1) * 8                         # the step flow's rows + column F
            assert sb >= int(lib.lib().mfg_workspace_bytes(B * 15, d))     # the rollout flow's gradient rows


def test_irl_population_exported_lazily():
    pytest.importorskip('torch')
    import subprocess
    import sys
    code = 'from discrete_mean_field_game_amd import AC_IRLPopulation as A; print(A.__name__)'
    out = subprocess.run([sys.executable, '-c', code], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == 'AC_IRLPopulation', out.stderr[-2000:]
    import discrete_mean_field_game_amd as pkg
    assert 'AC_IRLPopulation' in pkg.__all__

