"""CPU checks of the population entry points (mfg_train_episodes_pop / mfg_train_rollouts_pop): declared in the header, bound
in _lib.SIGNATURES, exported by the library; the Python wrappers refuse badly shaped per-learner arrays before any call."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POP = ('mfg_train_episodes_pop', 'mfg_train_rollouts_pop')


@pytest.fixture(scope='module')
def lib():
    from discrete_mean_field_game_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib


def test_declared_bound_and_exported(lib):
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'mfg_hip.h')).read(), flags=re.S)
    for name in POP:
        assert re.search(r'\b%s\s*\(' % name, text), name
        assert name in lib.SIGNATURES
        assert getattr(lib.lib(), name) is not None


def test_argument_counts_match_header(lib):
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'mfg_hip.h')).read(), flags=re.S)
    for name in POP:
        decl = re.search(r'\b%s\s*\(([^;]*)\);' % name, text, flags=re.S).group(1)
        assert len(decl.split(',')) == len(lib.SIGNATURES[name][1]), name


def test_abi_version_unchanged(lib):
    assert lib.lib().mfg_abi_version() == 18


def test_wrappers_refuse_host_or_misshaped_arrays():
    torch = pytest.importorskip('torch')
    from discrete_mean_field_game_amd import ops
    K = 3
    with pytest.raises(ValueError):
        ops._chk_pop(K, 'shifts', torch.zeros(K, dtype=torch.float64), torch.float64)  # host tensor
    with pytest.raises(ValueError):
        ops._chk_pop(K, 'seeds', [0, 1, 2], torch.int64)


def test_broadcast_scalars_and_arrays():
    np = pytest.importorskip('numpy')
    pytest.importorskip('torch')
    from discrete_mean_field_game_amd.population import broadcast
    assert np.array_equal(broadcast('shifts', 0.16, 3), [0.16, 0.16, 0.16])
    assert np.array_equal(broadcast('lr', [1, 2, 3], 3), [1.0, 2.0, 3.0])
    assert broadcast('seeds', 7, 2, np.uint64).dtype == np.uint64
    with pytest.raises(ValueError):
        broadcast('shifts', [0.1, 0.2], 3)


@pytest.mark.parametrize('kw', [dict(K=0), dict(d=65), dict(d=0), dict(batch=1), dict(update_every='episode'),
                                dict(reward='irl'), dict(precision='half'), dict(episode_steps=0)])
def test_check_args_refuses(kw):
    pytest.importorskip('torch')
    from discrete_mean_field_game_amd.population import check_args
    args = dict(K=4, d=21, batch=1024, update_every='step', reward='mfg_ac2', precision='mixed', episode_steps=15)
    check_args(**args)
    args.update(kw)
    with pytest.raises(ValueError):
        check_args(**args)


def test_population_exported_lazily():
    pytest.importorskip('torch')
    import subprocess
    import sys
    # a fresh interpreter: the first access goes through the package's lazy attribute, not an earlier submodule import
    code = 'from discrete_mean_field_game_amd import ActorCriticPopulation as A; print(A.__name__)'
    out = subprocess.run([sys.executable, '-c', code], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == 'ActorCriticPopulation', out.stderr[-2000:]
    import discrete_mean_field_game_amd as pkg
    from discrete_mean_field_game_amd.population import ActorCriticPopulation
    assert pkg.ActorCriticPopulation is ActorCriticPopulation
    assert 'ActorCriticPopulation' in pkg.__all__
