"""-m gpu: mfg_moves_loglik_pop (csrc/mfg_moves_loglik.hip) against its restatement (tests/moves_loglik_ref.py), and the
module on it (discrete_mean_field_game_amd/likelihood.py).

The bound is the project's own for mfg_policy_logpdf, 1e-10 relative (tests/test_gpu_launch_once_kernels.py), applied to the
condition sums of the restatement because ll itself may cancel: |ll - ref| <= 1e-10 S and |grad - ref| <= 1e-10 G per output
element.  Every comparison prints its worst ratio to the bound before it asserts."""
import numpy as np
import pytest

import guard_bands as GB
import moves_loglik_ref as R

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

REFERENCE_POINTS = [(8.86349, 0.16, 12000.0), (8.64, 0.0, 1e4), (9.99, 0.02, 2e4)]
POINTS = REFERENCE_POINTS + [(2.0, 0.1, 1.0), (1.0, -0.05, 1e-3), (0.0, 0.0, 3.0)]


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    return torch.device('cuda:0')


def _ops():
    from discrete_mean_field_game_amd import ops
    return ops


def _params(K):
    """K distinct policies: POINTS cycled, theta moved a little per cycle."""
    return np.array([(POINTS[k % 6][0] + 0.013 * (k // 6), POINTS[k % 6][1], POINTS[k % 6][2]) for k in range(K)])


def _data(S, N, H, d, width, seed):
    """Hand-made integers: states that sum to 1 over `width` (so below 1 over d < width); moves multinomial over width^2 cells,
    three agents to a cell on average, rows 3, 6, ... emptied and one cell of row 1 (row 0 at width 1) with 500 more."""
    rs = np.random.RandomState(seed)
    state = rs.dirichlet(np.ones(width), size=(S, N, H)).astype(np.float32)[..., :d].copy()
    cells = width * width
    moves = rs.multinomial(3 * cells, np.ones(cells) / cells, size=(S, N, H - 1)).reshape(S, N, H - 1, width, width)
    moves[..., 3::3, :] = 0
    moves[..., min(1, width - 1), 0] += 500
    return state, moves.astype(np.int32)


def _run(dev, state, moves, params, d, set_index=None, grad=True, **kw):
    t64 = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=dev)
    S = state.shape[0]
    st, mv = torch.as_tensor(state, device=dev), torch.as_tensor(moves, device=dev)
    if S == 1 and set_index is None:
        st, mv = st[0], mv[0]
    idx = None if set_index is None else torch.as_tensor(np.asarray(set_index, dtype=np.int32), device=dev)
    res = _ops().moves_loglik_pop(st, mv, t64(params[:, 0]), t64(params[:, 1]), t64(params[:, 2]), d, idx, grad, **kw)
    torch.cuda.synchronize()
    return {k: (None if v is None else v.cpu().numpy()) for k, v in res.items()}


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def _same(a, b):
    return all(np.array_equal(_bits(a[k]), _bits(b[k])) for k in a if a[k] is not None)


def _compare(what, got, state, moves, params, d, set_index=None):
    """Every policy against the restatement on its data set; prints the worst ratios; asserts the bound and the flags."""
    worst = [0.0, 0.0]
    for k, (theta, shift, alpha) in enumerate(params):
        s = 0 if set_index is None else int(set_index[k])
        ref = R.loglik(state[s], moves[s], theta, shift, alpha, d)
        clean = ref['flags'] == 0
        assert np.array_equal(got['status'][k], ref['status']), (what, k)
        with np.errstate(invalid='ignore'):                      # (-inf and NaN transitions are compared through their flags)
            err, bound = np.abs(got['ll'][k] - ref['ll'])[clean], R.BOUND * ref['S'][clean]
            gerr, gbound = np.abs(got['grad'][k] - ref['grad'])[clean], R.BOUND * ref['G'][clean]
        with np.errstate(invalid='ignore', divide='ignore'):
            worst[0] = max(worst[0], np.nan_to_num(err / bound).max(initial=0.0))
            worst[1] = max(worst[1], np.nan_to_num(gerr / gbound).max(initial=0.0))
        assert (err <= bound).all(), (what, k, 'll', float((err / bound).max()))
        assert (gerr <= gbound).all(), (what, k, 'grad', float(np.nanmax(gerr / gbound)))
        exact = clean & (ref['S'] == 0)                          # nothing counted: exactly 0
        assert (got['ll'][k][exact] == 0).all() and (got['grad'][k][exact] == 0).all()
        sums = R.day_sums(got['ll'][k], got['grad'][k], ref['flags'])
        assert np.array_equal(_bits(got['ll_day'][k]), _bits(sums['ll_day'])), (what, k)
        assert np.array_equal(_bits(got['grad_day'][k]), _bits(sums['grad_day'])), (what, k)
    print('moves_loglik %s: worst |ll - ref| / (1e-10 S) = %.3g, worst |grad - ref| / (1e-10 G) = %.3g' % (what, *worst))
    return worst


# ---------------------------------------------------------------------------------------------------- geometry
GEOMETRY = [  # (d, width, N, H, K, set_index over S data sets)
    (1, 1, 1, 2, 1, None), (1, 2, 3, 5, 3, None), (2, 2, 1, 2, 5, None), (2, 3, 3, 5, 3, [2, 0, 1]), (3, 3, 3, 5, 257, None),
    (3, 5, 1, 2, 5, [1, 2, 0, 2, 1]), (15, 15, 3, 5, 3, None), (15, 17, 1, 2, 5, None), (21, 21, 3, 5, 5, None),
    (21, 24, 1, 2, 3, [2, 0, 1]), (64, 64, 1, 2, 1, None), (64, 66, 1, 2, 3, None)]


@pytest.mark.parametrize('d,width,N,H,K,index', GEOMETRY, ids=lambda v: 'x' if isinstance(v, list) else str(v))
def test_geometry(dev, d, width, N, H, K, index):
    S = 1 if index is None else 3
    state, moves = _data(S, N, H, d, width, seed=d * 100 + K)
    params = _params(K)
    got = _run(dev, state, moves, params, d, index)
    _compare('d=%d width=%d N=%d H=%d K=%d S=%d' % (d, width, N, H, K, S), got, state, moves, params, d, index)


def test_logs_counted_on_the_device(dev):
    """The moves of ops.demos_from_logs on a small random log, handed over as they come."""
    rs = np.random.RandomState(5)
    topic = torch.as_tensor(rs.randint(-1, 6, size=(2, 4, 400)).astype(np.int32), device=dev)
    res = _ops().demos_from_logs(topic, 6, 4, width=5)
    params = _params(3)
    t64 = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev)
    out = _ops().moves_loglik_pop(res['state'], res['moves'], t64(params[:, 0]), t64(params[:, 1]), t64(params[:, 2]), 4)
    got = {k: v.cpu().numpy() for k, v in out.items()}
    _compare('from_logs', got, res['state'].cpu().numpy()[None], res['moves'].cpu().numpy()[None], params, 4)


# ---------------------------------------------------------------------------------------------------- counts
def _count_state(d=21, seed=3):
    return np.random.RandomState(seed).dirichlet(np.ones(d), size=(1, 1, 2)).astype(np.float32)


@pytest.mark.parametrize('alpha', [None, 1.0, 1e-3])
def test_every_boundary_of_the_small_m_form(dev, alpha):
    """m = 0 .. 70 in consecutive cells (rows 0 to 3 of d = 21), the other rows empty: under the reference's points a is 1e3 to
    2e5 (the series), under alpha_scale = 1 and 1e-3 it is below 16 (the recurrence), and theta = 0."""
    state = _count_state()
    moves = np.zeros((1, 1, 1, 21, 21), np.int32)
    moves.reshape(-1)[:71] = np.arange(71)
    params = np.array(REFERENCE_POINTS + [(0.0, 0.0, 12000.0)]) if alpha is None else np.array([(8.86349, 0.16, alpha), (0.0, 0.0, alpha),
                                                                                                  (2.0, -0.1, alpha)])
    got = _run(dev, state, moves, params, 21)
    _compare('m = 0..70, alpha_scale %s' % alpha, got, state, moves, params, 21)


def test_a_million_agents(dev):
    """One cell of 1 000 000 with the rest of its row empty, and one row that spreads 1 000 000 agents evenly: one policy, so
    that the restatement's finite sums over 1e6 terms run once."""
    state = np.repeat(_count_state(), 2, axis=1)
    moves = np.zeros((1, 2, 1, 21, 21), np.int32)
    moves[0, 0, 0, 10, 3] = 1000000
    moves[0, 1, 0, 12] = 1000000 // 21
    moves[0, 1, 0, 12, 0] += 1000000 - 21 * (1000000 // 21)
    assert moves[0, 1, 0, 12].sum() == 1000000
    params = np.array(REFERENCE_POINTS[:1])
    got = _run(dev, state, moves, params, 21)
    _compare('1e6 agents', got, state, moves, params, 21)


# ---------------------------------------------------------------------------------------------------- failures
def test_underflow_and_the_status_bits(dev):
    """d = 3, state (0.4, 0.35, 0.25), shift 0.5: x lies in [-0.65, -0.35], so theta = 1500 underflows a to 0 exactly where
    pi_j <= pi_i (theta x <= -750) and leaves a > 0 elsewhere, with no overflow anywhere."""
    state = np.tile(np.float32([0.4, 0.35, 0.25]), (2, 2, 3, 1))
    moves = np.zeros((2, 2, 2, 3, 3), np.int32)
    moves[:, :, :, 1, 0], moves[:, :, :, 2, 0], moves[:, :, :, 2, 1] = 4, 2, 9       # cells with a > 0 only: finite
    moves[0, 1, 1, 0, 2] = 3                                                          # set 0, day 1: a cell with a = 0
    moves[1, 0, 0, 1, 1] = -1                                                         # set 1, day 0: a failed member
    params = np.array([(1500.0, 0.5, 1.0), (1500.0, 0.5, 1.0), (2.0, 0.1, 5.0), (np.nan, 0.0, 1.0), (1.0, 0.0, 0.0),
                       (1.0, np.inf, 1.0), (1.0, 0.0, -2.0), (2.0, 0.1, 5.0), (2.0, 0.1, 5.0)])
    index = [0, 1, 1, 0, 0, 0, 0, 2, -1]
    got = _run(dev, state, moves, params, 3, index)
    assert got['status'].tolist() == [[0, 2], [1, 0], [1, 0], [4, 4], [4, 4], [4, 4], [4, 4], [8, 8], [8, 8]]
    a = R.alphas(state[0, 0, 0], 1500.0, 0.5, 1.0)[0]
    assert (a[np.triu_indices(3)] == 0).all() and (a[np.tril_indices(3, -1)] > 0).all()
    assert np.isfinite(got['ll'][0, 0]).all() and np.isfinite(got['grad'][0, 0]).all() and np.isfinite(got['ll_day'][0, 0])
    assert got['ll'][0, 1].tolist()[1] == -np.inf and np.isfinite(got['ll'][0, 1, 0]) and got['ll_day'][0, 1] == -np.inf
    assert np.isnan(got['grad'][0, 1, 1]).all() and np.isnan(got['grad_day'][0, 1]).all()
    assert np.isnan(got['ll'][1, 0, 0]) and np.isnan(got['grad'][1, 0, 0]).all() and np.isnan(got['ll_day'][1, 0])
    assert np.isfinite(got['ll'][1, 0, 1]) and np.isfinite(got['ll_day'][1, 1])
    for k in range(3, 9):
        assert all(np.isnan(got[name][k]).all() for name in ('ll', 'll_day', 'grad', 'grad_day')), k
    _compare('status', {n: v[:3] for n, v in got.items()}, state, moves, params[:3], 3, index[:3])


# ---------------------------------------------------------------------------------------------------- invariance
@pytest.fixture(scope='module')
def population(dev):
    state, moves = _data(3, 3, 5, 3, 4, seed=11)
    params = _params(257)
    index = (np.arange(257) * 7 % 3).astype(np.int32)
    return state, moves, params, index, _run(dev, state, moves, params, 3, index)


def test_a_policy_alone_and_permuted(dev, population):
    state, moves, params, index, full = population
    for k in (0, 100, 255, 256):
        alone = _run(dev, state, moves, params[k:k + 1], 3, index[k:k + 1])
        assert _same(alone, {n: v[k:k + 1] for n, v in full.items()}), k
    perm = np.random.RandomState(1).permutation(257)
    assert not np.array_equal(perm, np.arange(257))
    shuffled = _run(dev, state, moves, params[perm], 3, index[perm])
    assert _same(shuffled, {n: v[perm] for n, v in full.items()})
    halves = [_run(dev, state, moves, params[sl], 3, index[sl]) for sl in (slice(0, 130), slice(130, 257))]
    assert _same({n: np.concatenate([h[n] for h in halves]) for n in full}, full)
    no_grad = _run(dev, state, moves, params, 3, index, grad=False)
    assert no_grad['grad'] is None and no_grad['grad_day'] is None and _same(no_grad, full)


def _guarded(dev, state, moves, params, index, d, pad=1 << 16):
    ops = _ops()
    S, N, H = state.shape[:3]
    K = len(params)
    out = {n: GB.Guarded(shape, dtype, dev, pad=pad, fill=float('nan') if dtype == torch.float64 else None)
           for n, (shape, dtype) in ops.moves_loglik_shapes(K, N, H).items()}
    nbytes = ops.moves_loglik_workspace_bytes(K, S, N, H, d)
    ws = GB.Guarded(nbytes // 8, torch.int64, dev, pad=pad)          # (left 0xA5: poisoned)
    return out, ws


def test_guard_bands_poisoned_workspace_side_stream_and_graph(dev, population):
    state, moves, params, index, full = population
    ops = _ops()
    t64 = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev)
    args = (torch.as_tensor(state, device=dev), torch.as_tensor(moves, device=dev), t64(params[:, 0]), t64(params[:, 1]),
            t64(params[:, 2]), 3, torch.as_tensor(index, device=dev))
    call = lambda out, ws: ops.moves_loglik_pop(*args, out={n: g.t for n, g in out.items()}, workspace=ws.t)
    # outputs pre-filled with NaN, the workspace with 0xA5; exactly the query's bytes
    out, ws = _guarded(dev, state, moves, params, index, 3)
    call(out, ws)
    torch.cuda.synchronize()
    GB.check_all(*out.items(), ('workspace', ws))
    assert _same({n: g.t.cpu().numpy() for n, g in out.items()}, full)
    # another poison: nothing read from the workspace before it is written
    ws.t.fill_(-1)
    call(out, ws)
    torch.cuda.synchronize()
    assert _same({n: g.t.cpu().numpy() for n, g in out.items()}, full)
    # a side stream
    out2, ws2 = _guarded(dev, state, moves, params, index, 3)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        call(out2, ws2)
    side.synchronize()
    GB.check_all(*out2.items(), ('workspace', ws2))
    assert _same({n: g.t.cpu().numpy() for n, g in out2.items()}, full)
    # captured in a graph and replayed
    out3, ws3 = _guarded(dev, state, moves, params, index, 3)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call(out3, ws3)
    for g in out3.values():
        g.t.fill_(7)
    graph.replay()
    torch.cuda.synchronize()
    GB.check_all(*out3.items(), ('workspace', ws3))
    assert _same({n: g.t.cpu().numpy() for n, g in out3.items()}, full)


# ---------------------------------------------------------------------------------------------------- the module
@pytest.fixture(scope='module')
def logs(dev):
    """A small log with structure: agents drift towards the topics that are already popular."""
    rs = np.random.RandomState(21)
    N, H, U, C = 2, 4, 600, 5
    topic = np.zeros((N, H, U), np.int32)
    topic[:, 0] = rs.choice(C, size=(N, U), p=[0.4, 0.25, 0.2, 0.1, 0.05])
    for h in range(1, H):
        move = rs.rand(N, U) < 0.3
        topic[:, h] = np.where(move, rs.choice(C, size=(N, U), p=[0.5, 0.25, 0.15, 0.07, 0.03]), topic[:, h - 1])
    return topic


@pytest.fixture(scope='module')
def demonstrations(dev, logs):
    from discrete_mean_field_game_amd import demos
    return demos.from_logs(logs, 3, categories=5, width=4, device=dev)


def test_gridsearch(dev, demonstrations, tmp_path):
    from discrete_mean_field_game_amd import likelihood as LK
    from discrete_mean_field_game_amd.population import grid_points
    ranges = ((1.0, 4.0, 8.0), (0.0, 0.1), (1.0, 50.0))
    points = grid_points(*ranges)
    ref = [R.loglik(demonstrations.state, demonstrations.moves, *p, 3) for p in points]
    totals = np.array([r['ll_day'].sum() for r in ref])
    bound = max(R.BOUND * r['S'].sum() for r in ref)
    order = np.argsort(totals)
    assert totals[order[-1]] - totals[order[-2]] > 100 * bound            # (the grid tells its two best points apart)
    outfile = tmp_path / 'grid.csv'
    table, best = LK.gridsearch(*ranges, demonstrations, outfile=str(outfile), device=dev)
    par = np.array(points)
    res = LK.loglik(demonstrations, par[:, 0], par[:, 1], par[:, 2], device=dev)
    assert np.array_equal(_bits(table[:, 0]), _bits(res.total())) and (table[:, 1] == 0).all()
    assert best[:3] == tuple(points[order[-1]]) and best[3] == table[order[-1], 0]
    assert np.abs(table[:, 0] - totals).max() <= bound
    lines = outfile.read_text().splitlines()
    assert len(lines) == len(points) and [float(x) for x in lines[3].split(',')[:4]] == list(points[3]) + [table[3, 0]]
    one = LK.loglik(demonstrations, par[:, 0], par[:, 1], par[:, 2], days=[1], device=dev)
    assert one.days == [1] and np.array_equal(_bits(one.ll_day[:, 0]), _bits(res.ll_day[:, 1]))


def _host_fit(dev, d, state, moves, p0, mask, steps, lr):
    """The documented loop: ops.moves_loglik_pop, the days added in order, moves_loglik_ref.adam_step in NumPy fp64."""
    p, m, v = p0.copy(), np.zeros_like(p0), np.zeros_like(p0)
    trace = np.zeros((steps, len(p0)))
    for t in range(1, steps + 1):
        got = _run(dev, state, moves, np.stack([p[:, 0], p[:, 1], np.exp(p[:, 2])], 1), d)
        assert not got['status'].any()
        value, g = np.zeros(len(p)), np.zeros((len(p), 3))
        for n in range(state.shape[1]):
            value, g = value + got['ll_day'][:, n], g + got['grad_day'][:, n]
        trace[t - 1] = value
        p, m, v = R.adam_step(p, g, m, v, t, lr, mask)
    return p, trace


def test_fit_follows_the_documented_loop(dev, demonstrations):
    from discrete_mean_field_game_amd import likelihood as LK
    start = np.array([(2.0, 0.0, 5.0), (6.0, 0.1, 40.0), (0.5, -0.1, 1.0)])
    steps, lr = 8, 0.05
    fit = LK.fit(demonstrations, start[:, 0], start[:, 1], start[:, 2], steps=steps, lr=lr, device=dev)
    p0 = np.stack([start[:, 0], start[:, 1], np.log(start[:, 2])], 1)
    p, trace = _host_fit(dev, 3, demonstrations.state[None], demonstrations.moves[None], p0, np.ones(3), steps, lr)
    assert fit.trace.shape == (steps, 3) and not fit.status.any() and (fit.frozen_at == -1).all()
    np.testing.assert_allclose(fit.trace, trace, rtol=1e-12, atol=0)
    np.testing.assert_allclose(fit.params, np.stack([p[:, 0], p[:, 1], np.exp(p[:, 2])], 1), rtol=1e-12, atol=1e-14)
    assert (fit.best_ll > fit.trace[0]).all() and (fit.best_ll >= fit.trace.max(0)).all()
    only = LK.fit(demonstrations, start[:, 0], start[:, 1], start[:, 2], steps=steps, lr=lr, free=('theta',), device=dev)
    assert np.array_equal(only.params[:, 1:], start[:, 1:]) and (only.params[:, 0] != start[:, 0]).all()
    assert np.array_equal(only.best_params[:, 1:], start[:, 1:])


def test_fit_bootstrap_is_five_fits(dev, logs):
    from discrete_mean_field_game_amd import demos
    from discrete_mean_field_game_amd import likelihood as LK
    boot = demos.bootstrap(logs, 3, 5, seed=9, categories=5, width=4, device=dev)
    res = LK.fit_bootstrap(boot, 3.0, 0.05, 10.0, steps=6, device=dev)
    assert res.estimates.shape == (5, 3) and res.used.all() and res.interval.shape == (2, 3)
    for r in range(5):
        one = LK.fit(boot.replicate(r), 3.0, 0.05, 10.0, steps=6, device=dev)
        assert np.array_equal(_bits(one.params[0]), _bits(res.estimates[r])), r
        assert np.array_equal(_bits(one.trace[:, 0]), _bits(res.fit.trace[:, r])), r
    assert len({tuple(e) for e in res.estimates}) == 5                    # (the replicates differ)
    assert np.array_equal(res.mean, res.estimates.mean(0)) and (res.interval[0] <= res.interval[1]).all()


def test_the_populations_score_their_policies(dev):
    from discrete_mean_field_game_amd import demos
    from discrete_mean_field_game_amd import likelihood as LK
    from discrete_mean_field_game_amd.irl_population import AC_IRLPopulation
    from discrete_mean_field_game_amd.population import ActorCriticPopulation, _Population
    rs = np.random.RandomState(2)
    d = 21
    dm = demos.from_logs(rs.randint(0, d, size=(1, 3, 2000)).astype(np.int32), d, categories=d, device=dev)
    pop = ActorCriticPopulation([8.86349, 8.64], [0.16, 0.0], [12000.0, 1e4], d, batch=8, pi0=dm.pi0(), device=dev)
    got = pop.loglik(dm)
    want = LK.loglik(dm, [8.86349, 8.64], [0.16, 0.0], [12000.0, 1e4], device=dev)
    assert np.array_equal(_bits(got.ll), _bits(want.ll)) and got.total().shape == (2,) and not got.status.any()
    assert AC_IRLPopulation.loglik is _Population.loglik
