"""-m gpu: the hazards of mfg_var_fit_pop.  Its stream is a member of the descriptor, so the header scan of
tests/test_stream_order_host.py does not ask for a row in the table of tests/stream_order.py; the procedures of that table are
run on it here, on rows built inside stream_order.extra_rows() (one small, one with m > 128):
  behind a delayed producer on a side stream and captured into a graph (every launch on the descriptor's stream, no allocation,
  no synchronisation); under the poisoned-workspace procedure with every fill byte (the workspace is scratch: no result may
  depend on what it held); and with every output and the workspace between guard bands, at offsets 0 and 8."""
import numpy as np
import pytest

torch = pytest.importorskip('torch')

import guard_bands as GB  # noqa: E402
import stale_workspace as W  # noqa: E402
import stream_order as S  # noqa: E402

pytestmark = pytest.mark.gpu
ENTRY = 'mfg_var_fit_pop'

# name: d, days of the table, then (lag, ridge, training days, test days, origin) per model
SHAPES = {'small': (3, 6, [(1, 1e-2, [0, 1], [4, 5], 0), (5, 1e-8, [2, 0, 1, 3], [5], 1), (2, 1e-2, [3, 2], [], 0)]),
          'm136': (15, 8, [(9, 1e-2, [0, 1, 2, 3, 4], [6, 7], 1), (2, 1e-2, [5, 4, 3], [7, 6, 5], 0)])}
HD = 16


def _tables(specs):
    K = len(specs)
    ntr, nte = [len(s[2]) for s in specs], [len(s[3]) for s in specs]
    tr, te = np.zeros((K, max(ntr)), np.int32), np.zeros((K, max(nte)), np.int32)
    for k, s in enumerate(specs):
        tr[k, :ntr[k]], te[k, :nte[k]] = s[2], s[3]
    return tr, ntr, te, nte


def _shapes(name):
    from discrete_mean_field_game_amd import ops
    d, D, specs = SHAPES[name]
    tr, ntr, te, nte = _tables(specs)
    K, _, _, _, M, S_max = ops.check_var_fit_args((D, HD, d), [s[0] for s in specs], [s[1] for s in specs], ntr, nte,
                                                  [s[4] for s in specs])
    return ops.var_fit_shapes(K, d, M, S_max, te.shape[1])


def _days(a, D, d, seed):
    """Day rows on the simplex (the decoy: other rows), fp64."""
    x = a.simplex((D, HD, d), seed).double()
    return x / x.sum(-1, keepdim=True)


def _row(name):
    with S.extra_rows() as rows:
        @S.row('var_fit_pop-' + name, ENTRY, work=((ENTRY, 'workspace', S.SCRATCH_KIND),))
        def build(a):
            ops = S._ops()
            d, D, specs = SHAPES[name]
            tr, ntr, te, nte = _tables(specs)
            lags, ridges, origins = [s[0] for s in specs], [s[1] for s in specs], [s[4] for s in specs]
            days = a.inp('days', _days(a, D, d, 81))
            # (the model table and the day lists are the same in the decoy: the workspace layout is read from them)
            table, nbytes = ops.var_models(lags, ridges, ntr, nte, origins, d)
            models = (table, a.inp('models', ops.var_models_device(table, a.dev)), nbytes)
            tr_dev, te_dev = a.inp('train_idx', torch.as_tensor(tr, device=a.dev)), a.inp('test_idx', torch.as_tensor(te, device=a.dev))
            out = {n: a.out(n, shape, dtype) for n, (shape, dtype) in _shapes(name).items()}
            ws = a.ws(nbytes)
            a.keep.append(table)
            return lambda: ops.var_fit_pop(days, lags, ridges, tr_dev, ntr, te_dev, nte, origins, out=out, workspace=ws, models=models)
    return rows[0]


class _Module:
    pass


@pytest.fixture(scope='module')
def M():
    if not torch.cuda.is_available():
        pytest.fail('-m gpu tests need a GPU: the HIP path has no CPU fallback')
    m = _Module()
    m.dev = torch.device('cuda:0')
    m.rows = {name: _row(name) for name in SHAPES}
    m.ref = {name: S.reference(r, m.dev) for name, r in m.rows.items()}
    m.cycles = int(max(20.0, 10e3 * max(r.enqueue_s for r in m.ref.values())) * S.sleep_cycles_per_ms())
    m.side = S.independent_side_stream(m.dev, m.cycles)
    return m


@pytest.mark.parametrize('name', sorted(SHAPES))
def test_the_reference_run_is_a_real_fit(M, name):
    want = M.ref[name].want
    assert not want['status'].any() and all(bool(torch.isfinite(want[n]).all()) for n in want if n not in ('status', 'metrics'))
    for k, s in enumerate(SHAPES[name][2]):                # (a model without a test day has NaN metrics, by definition)
        assert bool(torch.isfinite(want['metrics'][k]).all()) == bool(s[3])
    assert bool((want['coef'] != 0).any()) and bool((want['future'] != 0).any())


@pytest.mark.parametrize('name', sorted(SHAPES))
def test_call_runs_behind_a_delayed_producer(M, name):
    r = M.rows[name]
    pending, got = S.run_delayed(r, M.ref[name], M.dev, M.cycles, M.side)
    assert pending, '%s: inconclusive -- the producer had finished when the call returned, or the call waited for it' % name
    bad = S.differing(got, M.ref[name].want)
    assert not bad, '%s: %s differ from the default-stream run: part of the call ran ahead of the stream it was given' % (name, bad)


@pytest.mark.parametrize('name', sorted(SHAPES))
def test_call_is_capturable_and_replays(M, name):
    found = S.run_captured(M.rows[name], M.ref[name], M.dev, M.side)
    assert not found, '%s: %s' % (name, found)


@pytest.mark.parametrize('fill', W.FILLS, ids=lambda f: '0x%02X' % f)
@pytest.mark.parametrize('name', sorted(SHAPES))
def test_results_do_not_depend_on_what_the_workspace_held(M, name, fill):
    assert W.poisoned(M.rows[name], M.ref[name].want, M.dev, fill) == []


@pytest.mark.parametrize('offset', [0, 8])
@pytest.mark.parametrize('name', sorted(SHAPES))
def test_guard_bands_round_the_outputs_and_the_workspace(M, name, offset):
    from discrete_mean_field_game_amd import ops
    d, D, specs = SHAPES[name]
    tr, ntr, te, nte = _tables(specs)
    lags, ridges, origins = [s[0] for s in specs], [s[1] for s in specs], [s[4] for s in specs]
    a = S.Bufs(M.dev, 0)
    days = _days(a, D, d, 81)
    table, nbytes = ops.var_models(lags, ridges, ntr, nte, origins, d)
    g = {n: GB.Guarded(shape, dtype, M.dev, offset=offset, fill=float('nan') if dtype.is_floating_point else -7)
         for n, (shape, dtype) in _shapes(name).items()}
    ws = GB.Guarded(nbytes // 8, torch.float64, M.dev, offset=offset, fill=0.0)
    ops.var_fit_pop(days, lags, ridges, torch.as_tensor(tr, device=M.dev), ntr, torch.as_tensor(te, device=M.dev), nte, origins,
                    out={n: x.t for n, x in g.items()}, workspace=ws.t, models=(table, ops.var_models_device(table, M.dev), nbytes))
    torch.cuda.synchronize()
    GB.check_all(('workspace', ws), *g.items())
    want = M.ref[name].want
    assert S.differing({n: x.t for n, x in g.items()}, want) == []
