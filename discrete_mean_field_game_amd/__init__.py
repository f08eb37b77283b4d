"""MI355X-native batched mean-field-game environment + actor-critic hot path.

Host side: Python on PyTorch-ROCm (device memory, streams, torch.distributed).
Hot path: hand-written HIP kernels behind the C ABI of include/mfg_hip.h (csrc/).
"""
from . import _lib  # noqa: F401

__all__ = ['_lib', 'population', 'ActorCriticPopulation', 'irl_population', 'AC_IRLPopulation', 'demos']


def __getattr__(name):
    # the population modules (K independent learners in the launches of one) import torch: loaded on first use
    if name in ('population', 'ActorCriticPopulation'):
        import importlib
        population = importlib.import_module(__name__ + '.population')
        return population if name == 'population' else population.ActorCriticPopulation
    if name in ('irl_population', 'AC_IRLPopulation'):
        import importlib
        irl_population = importlib.import_module(__name__ + '.irl_population')
        return irl_population if name == 'irl_population' else irl_population.AC_IRLPopulation
    if name == 'demos':
        import importlib
        return importlib.import_module(__name__ + '.demos')
    raise AttributeError('module %r has no attribute %r' % (__name__, name))
__version__ = '0.1.0'
