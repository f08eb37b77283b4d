"""CPU checks of the finite-population members (mfg_agents_step_pop, mfg_forecast_agents_pop, ops.agents_step_pop /
forecast_agents_pop, population.apportion / forecast_agents / forecast_agents_score and the class methods): the start counts, the
NumPy restatement the GPU tests compare with bit for bit (tests/agents_ref.py) -- its thresholds, its conservation, its moments
against the multinomial and its mean-field limit -- and what needs no GPU of the entries: declared, bound, exported, refused."""
import inspect
import os
import re

import numpy as np
import pytest

import agents_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED, EWORKSPACE = -1, -3, -4
NAMES = ('mfg_agents_step_pop', 'mfg_forecast_agents_pop', 'mfg_forecast_agents_pop_workspace_bytes')
SEED = 20261020


@pytest.fixture(scope='module')
def lib():
    from discrete_mean_field_game_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib


def _actions(rs, d, zeros=False):
    """An action [d, d] fp32, rows on the simplex up to fp32 rounding (with `zeros`: some exact zeros, renormalised)."""
    P = rs.dirichlet(np.ones(d), size=d)
    if zeros:
        P[rs.rand(d, d) < 0.3] = 0.0
        P[np.arange(d), rs.randint(d, size=d)] += 0.1
        P /= P.sum(axis=1, keepdims=True)
    return P.astype(np.float32)


# ------------------------------------------------------------------------------------------------------- the start counts
@pytest.mark.parametrize('agents', [1, 3, 1000, 1 << 24])
def test_apportion_rows_sum_to_agents(agents):
    pytest.importorskip('torch')
    from discrete_mean_field_game_amd.population import apportion
    rs = np.random.RandomState(agents % 1000)
    pi = rs.dirichlet(np.ones(21), size=5)
    pi[1, ::2] = 0.0                                                 # zeros
    pi[1] /= pi[1].sum()
    pi[2] = 1.0 / 21                                                 # all ties
    pi[3] = 0.0
    pi[3, [4, 9]] = 0.5                                              # two tied topics, the rest empty
    c = apportion(pi, agents)
    assert c.dtype == np.int32 and c.shape == pi.shape
    assert np.array_equal(c.sum(axis=1), np.full(5, agents)) and c.min() >= 0
    assert np.all(c[1, ::2] == 0) and np.all(c[3, [0, 1, 20]] == 0)
    assert np.abs(c - pi.astype(np.float32).astype(np.float64) * agents).max() < 1.0 + 1e-6 * agents
    # ties go to the lower index
    assert c[3, 4] == (agents + 1) // 2 and c[3, 9] == agents // 2
    base, extra = divmod(agents, 21)
    assert np.array_equal(c[2], base + (np.arange(21) < extra))
    assert np.array_equal(apportion(pi[0], agents), c[0])            # a single row


def test_apportion_is_exact_on_integral_rows():
    pytest.importorskip('torch')
    from discrete_mean_field_game_amd.population import apportion
    want = np.array([[512, 0, 256, 128, 64, 32, 16, 8, 4, 2, 1, 1], [1, 1, 2, 4, 8, 16, 32, 64, 128, 256, 0, 512]])
    pi = (want / 1024.0).astype(np.float32)                          # fp32-representable, 1024 pi integral
    assert np.array_equal(apportion(pi, 1024), want)
    assert np.array_equal(apportion(np.array([0.25, 0.75], dtype=np.float32), 1 << 24), [1 << 22, 3 << 22])
    for bad in (dict(pi=[0.5, 0.5], agents=0), dict(pi=[0.5, 0.5], agents=(1 << 24) + 1), dict(pi=[0.5, 0.5], agents=2.5),
                dict(pi=[0.0, 0.0], agents=3), dict(pi=[-0.5, 1.5], agents=3), dict(pi=[np.nan, 1.0], agents=3),
                dict(pi=np.ones((2, 2, 2)), agents=3)):
        with pytest.raises(ValueError):
            apportion(**bad)


# -------------------------------------------------------------------------------------------------- the restatement itself
def test_thresholds_edge_cases():
    P = np.array([[0.0, 0.5, 0.0, 0.5], [1e-20, 1.0, 1e-20, 1e-20], [0.0, 0.0, 0.0, 3.0], [0.25, 0.25, 0.25, 0.25]], dtype=np.float32)
    t, last = ref.thresholds(P)
    assert np.all(t[:, -1] == 1 << 32)                               # the last threshold: every agent lands somewhere
    assert np.all(np.diff(t, axis=1) >= 0)
    assert t[0].tolist() == [0, 1 << 31, 1 << 31, 1 << 32]           # zero columns: equal thresholds
    assert t[1, 0] == 0 and t[1, 1] == t[1, 2] == (1 << 32)          # 1e-20 is below 2^-32 of the row, and 1 + 1e-20 == 1 in fp64
    assert t[2].tolist() == [0, 0, 0, 1 << 32] and t[3].tolist() == [1 << 30, 1 << 31, 3 << 30, 1 << 32]
    counts = np.array([7, 5, 9, 4])
    nxt, moves, pi = ref.step(counts, P, 25, SEED, 3, 11)
    assert np.all(moves[0, [0, 2]] == 0) and moves[0].sum() == 7     # empty moves into the zero columns
    assert moves[1].tolist() == [0, 5, 0, 0] and moves[2].tolist() == [0, 0, 0, 9]
    assert np.array_equal(moves.sum(axis=1), counts) and nxt.sum() == 25
    assert np.array_equal(pi, (nxt / 25.0).astype(np.float32))
    # t = 2^32 accepts the word 0xFFFFFFFF, t = 0 accepts nothing (the comparison is in 64 bits)
    w = np.array([0, 0xFFFFFFFF], dtype=np.int64)
    assert np.all(w < t[2, 3]) and not np.any(w < t[2, 0])


def test_a_bad_row_fails_its_member_only_when_it_has_agents():
    P = _actions(np.random.RandomState(0), 5)
    for poison in (np.nan, np.inf, -np.inf):
        Q = P.copy()
        Q[2, 1] = poison
        nxt, moves, pi = ref.step([3, 4, 1, 0, 2], Q, 10, SEED, 0, 0)
        assert np.all(nxt == -1) and np.all(moves == -1) and np.isnan(pi).all()
        nxt, moves, pi = ref.step([3, 4, 0, 1, 2], Q, 10, SEED, 0, 0)
        assert nxt.sum() == 10 and np.all(moves[2] == 0)
    Q = P.copy()
    Q[0] = 0.0                                                       # a row that sums to 0
    assert np.all(ref.step([1, 0, 0, 0, 9], Q, 10, SEED, 0, 0)[0] == -1)
    assert np.all(ref.step([-1, 2, 0, 0, 9], P, 10, SEED, 0, 0)[0] == -1) and np.all(ref.step([11, 0, 0, 0, 0], P, 10, SEED, 0, 0)[0] == -1)


def test_words_follow_the_counter_layout():
    from oracle.philox_ref import philox4x32_10
    j, seed = (5 << 32) | 77, (9 << 32) | 1234
    w = ref.words(seed, 6, j, 3, 11)
    for a in (0, 1, 3, 4, 10):
        blk = philox4x32_10(0x80000000 | (3 << 22) | (a >> 2), 6, 77, 5, 1234, 9)
        assert w[a] == int(blk[a & 3])


@pytest.mark.parametrize('d,agents', [(21, 1000), (15, 257), (3, 5), (1, 4)])
def test_every_step_returns_all_agents(d, agents):
    rs = np.random.RandomState(d)
    counts = rs.multinomial(agents, rs.dirichlet(np.ones(d)))
    for s in range(4):
        P = _actions(rs, d, zeros=bool(s & 1))
        nxt, moves, _ = ref.step(counts, P, agents, SEED + d, s, 3)
        assert nxt.sum() == agents and np.array_equal(moves.sum(axis=1), counts) and moves.min() >= 0
        many = ref.step_members(counts, P, SEED + d, s, [0, 3, (1 << 40) + 3])
        assert np.array_equal(many[1], nxt) and np.all(many.sum(axis=1) == agents)      # the two forms of the restatement agree
        counts = nxt


@pytest.mark.parametrize('d,agents', [(21, 1000), (15, 257), (3, 5)])
def test_moments_are_the_multinomial_ones(d, agents):
    """M members from the same counts and action: counts'_c is a sum of independent multinomials, mean sum_i n_i P_ic and variance
    sum_i n_i P_ic (1 - P_ic).  The mean within 5 standard errors, the sample variance within [0.85, 1.15] of it."""
    M = 4096
    rs = np.random.RandomState(SEED % (1 << 31) + d)
    P = _actions(rs, d)
    n = rs.multinomial(agents, rs.dirichlet(np.ones(d)))
    got = ref.step_members(n, P, SEED, 2, np.arange(M)).astype(np.float64)
    Pn = P.astype(np.float64) / P.astype(np.float64).sum(axis=1, keepdims=True)
    mean, var = n @ Pn, n @ (Pn * (1.0 - Pn))
    z = (got.mean(axis=0) - mean) / np.sqrt(var / M)
    ratio = got.var(axis=0, ddof=1) / var
    print('d=%d A=%d: largest |z| %.2f, variance ratios %.3f .. %.3f' % (d, agents, np.abs(z).max(), ratio.min(), ratio.max()))
    assert np.abs(z).max() < 5.0
    assert ratio.min() > 0.85 and ratio.max() < 1.15


def test_mean_field_limit():
    """One step at A = 2^20: every column within 6 multinomial standard deviations of agents (P^T pi)."""
    d, agents = 21, 1 << 20
    rs = np.random.RandomState(7)
    P = _actions(rs, d)
    n = rs.multinomial(agents, rs.dirichlet(np.ones(d)))
    got = ref.step_members(n, P, SEED, 0, [0])[0].astype(np.float64)
    Pn = P.astype(np.float64) / P.astype(np.float64).sum(axis=1, keepdims=True)
    z = (got - n @ Pn) / np.sqrt(n @ (Pn * (1.0 - Pn)))
    print('largest |z| %.2f' % np.abs(z).max())
    assert got.sum() == agents and np.abs(z).max() < 6.0


# ------------------------------------------------------------------------------------------- declared, bound, built, refused
def test_declared_bound_and_exported(lib):
    raw = open(os.path.join(ROOT, 'include', 'mfg_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', raw, flags=re.S)
    for name in NAMES:
        decl = re.search(r'\b%s\s*\(([^;]*)\);' % name, text, flags=re.S).group(1)
        assert len(decl.split(',')) == len(lib.SIGNATURES[name][1]), name
        assert getattr(lib.lib(), name) is not None
    assert re.search(r'#define MFG_AGENTS_MAX \(1 << (\d+)\)', text).group(1) == '24' and lib.AGENTS_MAX == 1 << 24
    assert lib.lib().mfg_abi_version() == 18
    comment = raw[raw.index('Finite populations: a member is ONE population'):raw.index('#define MFG_AGENTS_MAX')]
    for cite in ('0x80000000 | (i << 22) | (a >> 2)', 'floor(S_ic / S_i,d-1 2^32)', 'mfg_sample_dirichlet', '2 (H - 1)', 'ONE launch'):
        assert cite in comment, cite


def test_the_unit_is_built_with_default_flags():
    mk = open(os.path.join(ROOT, 'discrete_mean_field_game_amd', 'csrc', 'Makefile')).read()
    assert 'mfg_agents' in re.search(r'^UNITS := (.*)$', mk, flags=re.M).group(1).split()
    assert 'mfg_agents.h' in re.search(r'^HDRS := (.*)$', mk, flags=re.M).group(1).split()
    for var in ('NOSLP_UNITS', 'ILP_UNITS'):
        assert 'mfg_agents' not in re.search(r'^%s :?= (.*)$' % var, mk, flags=re.M).group(1).split()
    for f in ('mfg_agents.hip', 'mfg_agents.h'):
        assert os.path.exists(os.path.join(ROOT, 'discrete_mean_field_game_amd', 'csrc', f))


def _step(lib, **kw):
    """mfg_agents_step_pop with fake device addresses: every call here must be refused (or do nothing) before any launch."""
    a = dict(counts=8, P=8, B=5, d=21, K=3, agents=1000, seed=8, step=0, traj_offset=0, counts_next=8, pi_next=8, moves=8)
    a.update(kw)
    return lib.lib().mfg_agents_step_pop(a['counts'], a['P'], a['B'], a['d'], a['K'], a['agents'], a['seed'], a['step'],
                                         a['traj_offset'], a['counts_next'], a['pi_next'], a['moves'], None)


@pytest.mark.parametrize('kw,code', [
    (dict(K=0), EINVAL), (dict(K=65536), EINVAL), (dict(B=-1), EINVAL), (dict(d=0), EINVAL), (dict(d=65), EUNSUPPORTED),
    (dict(agents=0), EINVAL), (dict(agents=(1 << 24) + 1), EINVAL), (dict(counts=None), EINVAL), (dict(P=None), EINVAL),
    (dict(seed=None), EINVAL), (dict(counts_next=None), EINVAL), (dict(B=1 << 31), EINVAL), (dict(traj_offset=1 << 48), EINVAL),
])
def test_step_entry_refuses_before_launch(lib, kw, code):
    assert _step(lib, **kw) == code
    assert lib.lib().mfg_last_error()


def test_step_entry_with_no_member_launches_nothing(lib):
    assert _step(lib, B=0) == 0 and _step(lib, B=0, pi_next=None, moves=None, agents=1 << 24) == 0


def _forecast(lib, **kw):
    a = dict(counts0=8, N=5, H=6, d=21, K=3, agents=1000, theta=8, shift=8, alpha=8, seed=8, first_step=0, repeats=4, precision=1,
             ranks=(0, 3), emp32=8, emp64=8, mean=8, std=8, quant=8, curves=8, traj=8, counts=8, actions=8, ws=8, ws_bytes=0)
    a.update(kw)
    import ctypes as C
    rk = (C.c_int32 * max(len(a['ranks']), 1))(*a['ranks'])
    return lib.lib().mfg_forecast_agents_pop(a['counts0'], a['N'], a['H'], a['d'], a['K'], a['agents'], a['theta'], a['shift'],
                                             a['alpha'], a['seed'], a['first_step'], a['repeats'], a['precision'], rk,
                                             len(a['ranks']), a['emp32'], a['emp64'], a['mean'], a['std'], a['quant'], a['curves'],
                                             a['traj'], a['counts'], a['actions'], a['ws'], a['ws_bytes'], None)


@pytest.mark.parametrize('kw,code', [
    (dict(K=0), EINVAL), (dict(K=65536), EINVAL), (dict(d=0), EINVAL), (dict(d=65), EUNSUPPORTED), (dict(H=1), EINVAL),
    (dict(N=0), EINVAL), (dict(repeats=0), EINVAL), (dict(agents=0), EINVAL), (dict(agents=(1 << 24) + 1), EINVAL),
    (dict(counts0=None), EINVAL), (dict(theta=None), EINVAL), (dict(seed=None), EINVAL), (dict(mean=None), EINVAL),
    (dict(ws=None), EINVAL), (dict(precision=2), EINVAL), (dict(first_step=0xFFFFFFFF), EINVAL), (dict(ranks=(4,)), EINVAL),
    (dict(quant=None), EINVAL), (dict(emp32=None), EINVAL), (dict(curves=None), EINVAL), (dict(repeats=1025), EUNSUPPORTED),
    (dict(), EWORKSPACE), (dict(traj=None, counts=None, actions=None), EWORKSPACE),
    (dict(emp32=None, emp64=None, curves=None, ranks=(), quant=None), EWORKSPACE),
])
def test_forecast_entry_refuses_before_launch(lib, kw, code):
    assert _forecast(lib, **kw) == code
    assert lib.lib().mfg_last_error()


def test_forecast_workspace_bytes(lib):
    h = lib.lib()
    N, H, d, K, R = 5, 6, 21, 3, 4
    full = h.mfg_forecast_agents_pop_workspace_bytes(N, H, d, K, R, 0, 0)
    members = K * N * R * H * d * 4
    assert h.mfg_forecast_agents_pop_workspace_bytes(N, H, d, K, R, 1, 0) == full - members
    assert h.mfg_forecast_agents_pop_workspace_bytes(N, H, d, K, R, 1, 1) == full - 2 * members
    assert full - 2 * members >= K * N * R * (d + d * d) * 4 + K * H * N * R * 16      # current rows, one step's actions, the curves' terms
    assert full % 8 == 0
    for empty in ((0, H, d, K, R), (N, 0, d, K, R), (N, H, 0, K, R), (N, H, d, 0, R), (N, H, d, K, 0)):
        assert h.mfg_forecast_agents_pop_workspace_bytes(*empty, 1, 1) == 0
    assert _forecast(lib, ws_bytes=full - 2 * members - 1) == EWORKSPACE
    assert str(full - 2 * members) in h.mfg_last_error().decode()


def test_ops_argument_rules(lib):
    torch = pytest.importorskip('torch')
    from discrete_mean_field_game_amd import ops
    ok = dict(counts_shape=(5, 21), agents=1000, horizon=6, repeats=4, ranks=(0, 3), precision='mixed')
    assert ops.check_forecast_agents_args(**ok) == (5, 21, 6, 4, [0, 3], 1000)
    for bad in (dict(agents=0), dict(agents=(1 << 24) + 1), dict(agents=2.5), dict(agents=True), dict(counts_shape=(5, 65)),
                dict(counts_shape=(21,)), dict(horizon=1), dict(repeats=0), dict(repeats=1025), dict(ranks=(4,)),
                dict(precision='f32'), dict(emp32_shape=(5, 6, 21)), dict(emp32_shape=(5, 6, 20), emp64_shape=(5, 6, 20))):
        with pytest.raises(ValueError):
            ops.check_forecast_agents_args(**dict(ok, **bad))
    assert ops.check_agents(np.int64(7)) == 7 and ops.check_agents(1 << 24) == 1 << 24
    with pytest.raises(ValueError):                                  # tensors off the device
        ops.agents_step_pop(torch.zeros(1, 2, 3, dtype=torch.int32), torch.zeros(1, 2, 3, 3), 5, torch.zeros(1, dtype=torch.int64))
    with pytest.raises(ValueError):
        ops.forecast_agents_pop(torch.zeros(2, 3, dtype=torch.int32), 5, None, None, None, None, 4)


def test_population_argument_rules(lib):
    pytest.importorskip('torch')
    from discrete_mean_field_game_amd import population
    emp = np.random.RandomState(0).dirichlet(np.ones(21), size=(2, 6))
    ok = dict(d=21, agents=100)
    for kw in (dict(agents=0), dict(agents=(1 << 24) + 1), dict(agents=1.5), dict(repeats=0), dict(repeats=1025), dict(d=65),
               dict(precision='f32'), dict(horizon=1), dict(horizon=7), dict(pi0=np.ones((3, 21)) / 21), dict(budget=1000)):
        with pytest.raises(ValueError):
            population.forecast_agents_score([8.0], 0.5, 1e4, emp, **dict(ok, **kw))
    for kw in (dict(agents=0), dict(agents=1.5), dict(repeats=0), dict(probs=(1.5,)), dict(precision='f32'), dict(d=65)):
        with pytest.raises(ValueError):
            population.forecast_agents([8.0], 0.5, 1e4, emp[:, 0], 6, **dict(ok, **kw))
    with pytest.raises(ValueError):
        population.forecast_agents([8.0], 0.5, 1e4, np.zeros(21), 6, **ok)           # a start row without mass
    with pytest.raises(TypeError):
        population.forecast_agents([8.0], 0.5, 1e4, emp[:, 0], 6, d=21)              # agents has no default
    assert population.forecast_agents_score_bytes(2, 6, 21, 256) >= 2 * 2 * 256 * 6 * 21 * 4   # members and counts


def test_class_methods_exist_and_take_agents():
    pytest.importorskip('torch')
    from discrete_mean_field_game_amd import ac_irl, mfg_ac2, mfg_synthetic, ops, population
    from discrete_mean_field_game_amd.irl_population import AC_IRLPopulation
    for name in ('forecast_agents', 'forecast_agents_score'):
        assert getattr(population.ActorCriticPopulation, name) is getattr(AC_IRLPopulation, name) is getattr(population._Population, name)
        assert getattr(ac_irl.AC_IRL, name) is getattr(mfg_ac2.actor_critic, name) is getattr(mfg_synthetic.actor_critic, name)
        for fn in (getattr(population, name), getattr(population._Population, name), getattr(mfg_ac2.actor_critic, name)):
            p = inspect.signature(fn).parameters['agents']
            assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is inspect.Parameter.empty
    for name in ('apportion', 'forecast_agents', 'forecast_agents_score', 'forecast_agents_policies', 'forecast_agents_score_policies'):
        assert hasattr(population, name), name
    for name in ('agents_step_pop', 'forecast_agents_pop', 'check_forecast_agents_args', 'forecast_agents_pop_workspace'):
        assert hasattr(ops, name), name
    want = inspect.signature(population.forecast).parameters
    got = inspect.signature(population.forecast_agents).parameters
    assert [p for p in got if p not in ('agents', 'want_counts')] == list(want)      # forecast's arguments, in its order
    f = population.Forecast(np.zeros((2, 1, 2, 3)), np.zeros((2, 1, 2, 3)), np.zeros((2, 1, 2, 0, 3)), (), (), None, 4,
                            counts=np.ones((2, 4, 2, 3), np.int32))
    assert f.learner(1).counts.shape == (4, 2, 3) and population.Forecast(0, 0, 0, (), (), None, 1).counts is None
