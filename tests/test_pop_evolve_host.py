"""CPU checks of population-based training inside a population training call (mfg_ctx_set_pop_evolve): the evolve block's ctypes
mirror has the C compiler's layout, the setter is declared / bound / exported without a stream and with the ABI number
unchanged, Evolution checks its arguments on the host, train() takes the keyword, and the NumPy restatement of a step
(tests/pop_evolve_ref.py) has the properties the header promises."""
import inspect
import os
import re

import pytest

np = pytest.importorskip('numpy')

import pop_evolve_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ['lr_critic', 'lr_actor', 'order', 'active', 'rank', 'parent', 'lr_log', 'seed', 'factor_down', 'factor_up',
          'lr_critic_min', 'lr_critic_max', 'lr_actor_min', 'lr_actor_max', 'every', 'n_top', 'n_bottom', 'perturb', 'max_steps', 'K']


@pytest.fixture(scope='module')
def lib():
    from discrete_mean_field_game_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib


def test_pop_evolve_struct_layout_matches_the_header(lib, tmp_path):
    """mfg_pop_evolve_t crosses the boundary by pointer: _lib.PopEvolveStruct must have the C compiler's size and field offsets
    (a small C program prints them from include/mfg_hip.h)."""
    import ctypes as C
    import subprocess
    fields = [n for n, _ in lib.PopEvolveStruct._fields_]
    assert fields == FIELDS
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "mfg_hip.h"\nint main(void){printf("%zu", '
           'sizeof(mfg_pop_evolve_t));\n')
    for f in fields:
        src += 'printf(" %%zu", offsetof(mfg_pop_evolve_t, %s));\n' % f
    src += 'return 0;}\n'
    c = tmp_path / 'layout.c'
    c.write_text(src)
    exe = str(tmp_path / 'layout')
    subprocess.run(['gcc', '-std=c99', '-I', os.path.join(ROOT, 'include'), str(c), '-o', exe], check=True)
    out = [int(x) for x in subprocess.run([exe], check=True, stdout=subprocess.PIPE).stdout.decode().split()]
    assert out[0] == C.sizeof(lib.PopEvolveStruct)
    assert out[1:] == [getattr(lib.PopEvolveStruct, f).offset for f in fields]


def test_pop_evolve_declared_bound_and_exported(lib):
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'mfg_hip.h')).read(), flags=re.S)
    decl = re.search(r'\bmfg_ctx_set_pop_evolve\s*\(([^;]*)\);', text, flags=re.S).group(1)
    assert len(decl.split(',')) == len(lib.SIGNATURES['mfg_ctx_set_pop_evolve'][1]) == 2
    assert 'mfg_stream_t' not in decl                # host only: no stream, no row in the stream-order table
    assert lib.lib().mfg_ctx_set_pop_evolve is not None
    assert lib.lib().mfg_abi_version() == 18


def test_set_pop_evolve_refuses_a_null_context(lib):
    """Checked before anything touches a device: no context, no block."""
    import ctypes as C
    blk = lib.PopEvolveStruct(*([8] * 7), 0, 0.8, 1.25, 1e-6, 10.0, 1e-8, 1.0, 1, 1, 1, 3, 4, 5)
    assert lib.lib().mfg_ctx_set_pop_evolve(None, C.byref(blk)) == -1
    assert b'context' in lib.lib().mfg_last_error()
    assert lib.lib().mfg_ctx_set_pop_evolve(None, None) == -1


def test_evolution_checks_its_arguments_on_the_host():
    pytest.importorskip('torch')
    from discrete_mean_field_game_amd.population import Evolution
    e = Evolution()
    assert (e.every, e.factors, e.perturb, e.perturb_bits, e.seed) == (1, (0.8, 1.25), ('lr_critic', 'lr_actor'), 3, 0)
    assert (e.lr_critic_bounds, e.lr_actor_bounds) == ((1e-6, 10.0), (1e-8, 1.0))
    assert e.counts(16) == (4, 4) and e.counts(5) == (1, 1) and e.counts(2) == (1, 1)       # max(1, floor(f K))
    assert Evolution(top=2, bottom=3).counts(5) == (2, 3) and Evolution(top=0.5, bottom=1).counts(7) == (3, 1)
    assert Evolution(perturb=()).perturb_bits == 0 and Evolution(perturb='lr_actor').perturb_bits == 2
    assert Evolution(perturb=('lr_critic',)).perturb_bits == 1
    with pytest.raises(ValueError):
        e.counts(1)                                   # 1 + 1 > 1
    with pytest.raises(ValueError):
        Evolution(top=3, bottom=3).counts(5)
    for bad in (dict(every=0), dict(every=1.5), dict(top=0), dict(top=0.0), dict(top=1.0), dict(bottom=-1), dict(bottom=1.5),
                dict(top=float('nan')), dict(factors=(0.8,)), dict(factors=(0.0, 1.25)), dict(factors=(0.8, float('inf'))),
                dict(factors=(-1.0, 2.0)), dict(perturb=('lr',)), dict(perturb=('lr_actor', 'lr_actor')),
                dict(lr_critic_bounds=(0.0, 1.0)), dict(lr_critic_bounds=(2.0, 1.0)), dict(lr_actor_bounds=(1e-8, float('inf'))),
                dict(lr_actor_bounds=(1e-8,)), dict(seed=-1), dict(seed=2 ** 64), dict(seed=0.5)):
        with pytest.raises(ValueError):
            Evolution(**bad)


def test_train_takes_evolve_keyword_only():
    pytest.importorskip('torch')
    from discrete_mean_field_game_amd.irl_population import AC_IRLPopulation
    from discrete_mean_field_game_amd.population import ActorCriticPopulation, EvolutionTrace
    par = inspect.signature(ActorCriticPopulation.train).parameters
    assert par['evolve'].kind is inspect.Parameter.KEYWORD_ONLY and par['evolve'].default is None
    assert 'evolve' not in inspect.signature(AC_IRLPopulation.train).parameters
    # lineage: learner 2 took learner 0's parameters at step 1, learner 0 had taken learner 1's at step 0; learner 3 was not active
    parent = np.array([[1, 0], [1, 1], [2, 0], [-1, -1]], dtype=np.int32)
    tr = EvolutionTrace(parent * 0, parent, np.zeros((4, 2, 2)), np.zeros(4), np.zeros(4), 1)
    assert tr.lineage(2).tolist() == [1, 0, 2] and tr.lineage(1).tolist() == [1, 1, 1] and tr.lineage(3).tolist() == [3, 3, 3]


# ------------------------------------------------------------------------------------- properties of the restatement
def _random_case(rs):
    K = int(rs.randint(2, 40))
    n_top = int(rs.randint(1, K))
    n_bottom = int(rs.randint(1, K - n_top + 1))
    values = rs.choice(np.round(rs.rand(6), 3), size=K)          # few distinct values: many ties
    bad = rs.rand(K) < rs.choice([0.0, 0.2, 0.7])
    values = np.where(bad, rs.choice([np.nan, np.inf, -np.inf], size=K), values)
    active = rs.rand(K) < rs.choice([1.0, 0.8, 0.4])
    F = 3
    kw = dict(s=int(rs.randint(0, 5)), seed=int(rs.randint(0, 2 ** 62)), n_top=n_top, n_bottom=n_bottom,
              perturb=int(rs.randint(0, 4)), factors=(0.5, 3.0), lr_critic_bounds=(0.05, 0.4), lr_actor_bounds=(1e-3, 4e-3))
    return values, active, rs.randn(K), rs.randn(K, F), rs.uniform(0.05, 0.4, K), rs.uniform(1e-3, 4e-3, K), kw


def test_restatement_properties_over_random_inputs():
    rs = np.random.RandomState(7)
    seen = dict(replaced=0, few=0, nonfinite_top=0, clamped=0)
    for _ in range(400):
        values, active, theta, w, lrc, lra, kw = _random_case(rs)
        K, n_top, n_bottom = len(values), kw['n_top'], kw['n_bottom']
        out = R.step(values, active, theta, w, lrc, lra, **kw)
        order, rank, parent, A = out['order'], out['rank'], out['parent'], int(active.sum())
        # rank is a permutation of the active set; the inactive stay -1 / NaN and keep everything
        assert sorted(order) == np.flatnonzero(active).tolist() and len(order) == A
        assert sorted(rank[active].tolist()) == list(range(A)) and (rank[~active] == -1).all() and (parent[~active] == -1).all()
        assert all(rank[order[r]] == r for r in range(A)) and np.isnan(out['lr'][~active]).all()
        for name, before in (('theta', theta), ('w', w), ('lr_critic', lrc), ('lr_actor', lra)):
            assert np.array_equal(out[name][~active], before[~active])
        # ties go to the smaller index, non-finite values come last (in index order)
        fin = np.isfinite(values)
        for a, b in zip(order, order[1:]):
            if fin[a] and fin[b]:
                assert values[a] < values[b] or (values[a] == values[b] and a < b)
            else:
                assert not fin[b] and (fin[a] or a < b)
        # when a step replaces and when it only logs
        enough = A >= n_top + n_bottom
        top_finite = enough and bool(fin[order[n_top - 1]])
        assert out['replaced'] == (enough and top_finite)
        seen['few'] += not enough
        seen['nonfinite_top'] += enough and not top_finite
        if not out['replaced']:
            assert np.array_equal(parent[active], np.flatnonzero(active))
            for name, before in (('theta', theta), ('w', w), ('lr_critic', lrc), ('lr_actor', lra)):
                assert np.array_equal(out[name], before)
            continue
        seen['replaced'] += 1
        # receivers are exactly the last n_bottom ranks; donors always have rank < n_top (and a finite value)
        changed = np.flatnonzero(active & (parent != np.arange(K)))
        receivers = order[A - n_bottom:]
        assert set(changed) <= set(receivers)
        for k in np.flatnonzero(active):
            if k in receivers:
                dnr = parent[k]
                assert 0 <= rank[dnr] < n_top and fin[dnr] and dnr not in receivers
                assert out['theta'][k] == theta[dnr] and np.array_equal(out['w'][k], w[dnr])
                for new, old, (lo, hi), bit in ((out['lr_critic'], lrc, kw['lr_critic_bounds'], 1),
                                                (out['lr_actor'], lra, kw['lr_actor_bounds'], 2)):
                    assert lo <= new[k] <= hi                                   # rates stay inside their bounds
                    if kw['perturb'] & bit:
                        assert new[k] in (min(max(old[dnr] * 0.5, lo), hi), min(max(old[dnr] * 3.0, lo), hi))
                        seen['clamped'] += new[k] in (lo, hi)
                    else:
                        assert new[k] == old[dnr]
            else:
                assert parent[k] == k and out['theta'][k] == theta[k] and np.array_equal(out['w'][k], w[k])
                assert out['lr_critic'][k] == lrc[k] and out['lr_actor'][k] == lra[k]
        assert np.array_equal(out['lr'][active], np.stack([out['lr_critic'], out['lr_actor']], 1)[active])
    assert min(seen.values()) > 10, seen             # every branch above was taken


def test_restatement_draws_the_documented_words():
    """Counter (0xFFFFFFFE, s, k, 0), key (seed low, seed high); donor = order[floor(x0 n_top / 2^32)]; coins x1 >> 31, x2 >> 31."""
    from oracle.philox_ref import philox4x32_10
    seed, s = 0x123456789ABCDEF0, 3
    K, n_top, n_bottom = 9, 4, 3
    values = np.arange(K, dtype=np.float64)[::-1].copy()          # learner 8 is the best, learner 0 the worst
    out = R.step(values, np.ones(K, bool), np.arange(K) * 1.0, np.arange(K)[:, None] * np.ones((1, 2)), np.full(K, 0.1),
                 np.full(K, 0.001), s=s, seed=seed, n_top=n_top, n_bottom=n_bottom)
    assert out['order'] == list(range(K - 1, -1, -1)) and out['replaced']
    for k in (0, 1, 2):
        x = [int(v) for v in philox4x32_10(0xFFFFFFFE, s, k, 0, 0x9ABCDEF0, 0x12345678)]
        donor = K - 1 - ((x[0] * n_top) >> 32)
        assert out['parent'][k] == donor and out['theta'][k] == donor
        assert out['lr_critic'][k] == 0.1 * (1.25 if x[1] >> 31 else 0.8)
        assert out['lr_actor'][k] == 0.001 * (1.25 if x[2] >> 31 else 0.8)
    assert out['parent'][3:].tolist() == list(range(3, K))
