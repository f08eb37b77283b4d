"""-m gpu: the hazards of mfg_rnn_fit_pop.  Its stream is a member of the descriptor, so the header scan of
tests/test_stream_order_host.py does not ask for a row in the table of tests/stream_order.py; the procedures of that table are
run on it here, on rows built inside stream_order.extra_rows() (one small, one with H = 64, whose weights live in the workspace):
  behind a delayed producer on a side stream and captured into a graph (every launch on the descriptor's stream, no allocation,
  no synchronisation); under the poisoned-workspace procedure with every fill byte (the workspace is scratch: every byte the
  kernels read, the Adam moments included, must have been written by this call); and with every output and the workspace between
  guard bands, at offsets 0 and 8."""
import numpy as np
import pytest

torch = pytest.importorskip('torch')

import guard_bands as GB  # noqa: E402
import rnn_ref as R  # noqa: E402
import stale_workspace as W  # noqa: E402
import stream_order as S  # noqa: E402

pytestmark = pytest.mark.gpu
ENTRY = 'mfg_rnn_fit_pop'

# name: d, days of the table, eval_every, then (H, epochs, lr, wd, clip, training, validation, test days) per model
SHAPES = {'small': (3, 7, 2, [(4, 5, 1e-2, 0.0, 0.0, [0, 1], [2], [4, 5]), (8, 4, 3e-3, 1e-3, 0.02, [2, 0, 1, 3, 6], [5, 4], [6]),
                              (4, 3, 1e-2, 0.0, 0.0, [3, 2], [], [])]),
          'h64': (15, 8, 1, [(64, 3, 1e-2, 1e-3, 0.02, [0, 1, 2, 3, 4], [5], [6, 7]), (16, 4, 1e-2, 0.0, 0.0, [5, 4, 3], [0, 1], [7, 6, 5])])}
HD = 16


def _tables(specs):
    K = len(specs)
    out = []
    for col in (5, 6, 7):
        n = [len(s[col]) for s in specs]
        t = np.zeros((K, max(n)), np.int32)
        for k, s in enumerate(specs):
            t[k, :n[k]] = s[col]
        out += [t, n]
    return out


def _columns(specs):
    return [[s[q] for s in specs] for q in range(5)]


def _w0(d, specs):
    w = np.zeros((len(specs), max(R.weight_count(s[0], d) for s in specs)))
    for k, s in enumerate(specs):
        w[k, :R.weight_count(s[0], d)] = R.init_weights(s[0], d, [4, k])
    return torch.as_tensor(w)


def _shapes(name):
    from discrete_mean_field_game_amd import ops
    d, D, every, specs = SHAPES[name]
    tr, ntr, va, nva, te, nte = _tables(specs)
    K, _, _, _, W_max, E_max, C_max = ops.check_rnn_fit_args((D, HD, d), *_columns(specs), ntr, nva, nte, 'adam', every)
    return ops.rnn_fit_shapes(K, HD, d, W_max, E_max, C_max, te.shape[1])


def _days(a, D, d, seed):
    """Day rows on the simplex (the decoy: other rows), fp64."""
    x = a.simplex((D, HD, d), seed).double()
    return x / x.sum(-1, keepdim=True)


def _row(name):
    with S.extra_rows() as rows:
        @S.row('rnn_fit_pop-' + name, ENTRY, work=((ENTRY, 'workspace', S.SCRATCH_KIND),))
        def build(a):
            ops = S._ops()
            d, D, every, specs = SHAPES[name]
            tr, ntr, va, nva, te, nte = _tables(specs)
            cols = _columns(specs)
            days = a.inp('days', _days(a, D, d, 83))
            w0 = a.inp('w0', _w0(d, specs).to(a.dev))
            # (the model table and the day lists are the same in the decoy: the workspace layout is read from them)
            table, nbytes = ops.rnn_models(*cols, ntr, nva, nte, d, HD)
            models = (table, a.inp('models', ops.rnn_models_device(table, a.dev)), nbytes)
            tr_dev, va_dev, te_dev = (a.inp(n, torch.as_tensor(t, device=a.dev)) for n, t in (('train_idx', tr), ('val_idx', va), ('test_idx', te)))
            out = {n: a.out(n, shape, dtype) for n, (shape, dtype) in _shapes(name).items()}
            ws = a.ws(nbytes)
            a.keep.append(table)
            return lambda: ops.rnn_fit_pop(days, w0, *cols, tr_dev, ntr, va_dev, nva, te_dev, nte, eval_every=every, out=out,
                                           workspace=ws, models=models)
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
    specs = SHAPES[name][3]
    assert not want['status'].any() and bool(torch.isfinite(want['weights']).all()) and bool(torch.isfinite(want['future']).all())
    for k, s in enumerate(specs):
        assert bool(torch.isfinite(want['loss'][k, :s[1]]).all()) and bool(torch.isnan(want['loss'][k, s[1]:]).all())
        assert bool(torch.isfinite(want['metrics'][k]).all()) == bool(s[7])       # (no test day: NaN metrics, by definition)
        assert int(torch.isfinite(want['val'][k]).sum()) == (-(-s[1] // SHAPES[name][2]) if s[6] else 0)
        assert 1 <= int(want['best_epoch'][k]) <= s[1]
    assert bool((want['weights'] != 0).any()) and bool((want['future'] != 0).any())


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
    d, D, every, specs = SHAPES[name]
    tr, ntr, va, nva, te, nte = _tables(specs)
    cols = _columns(specs)
    a = S.Bufs(M.dev, 0)
    days = _days(a, D, d, 83)
    table, nbytes = ops.rnn_models(*cols, ntr, nva, nte, d, HD)
    g = {n: GB.Guarded(shape, dtype, M.dev, offset=offset, fill=float('nan') if dtype.is_floating_point else -7)
         for n, (shape, dtype) in _shapes(name).items()}
    ws = GB.Guarded(nbytes // 8, torch.float64, M.dev, offset=offset, fill=0.0)
    ops.rnn_fit_pop(days, _w0(d, specs).to(M.dev), *cols, torch.as_tensor(tr, device=M.dev), ntr, torch.as_tensor(va, device=M.dev), nva,
                    torch.as_tensor(te, device=M.dev), nte, eval_every=every, out={n: x.t for n, x in g.items()}, workspace=ws.t,
                    models=(table, ops.rnn_models_device(table, M.dev), nbytes))
    torch.cuda.synchronize()
    GB.check_all(('workspace', ws), *g.items())
    want = M.ref[name].want
    assert S.differing({n: x.t for n, x in g.items()}, want) == []
