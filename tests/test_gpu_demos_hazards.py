"""-m gpu: the hazards of mfg_demos_from_logs.  Its stream is a member of the descriptor, so the header scan of
tests/test_stream_order_host.py does not ask for a row in the table of tests/stream_order.py; the procedures of that table are
run on it here, on rows built inside stream_order.extra_rows() (one small shape, one with several workgroups per day and a
ragged last one):
  behind a delayed producer on a side stream and captured into a graph (every launch and both memsets on the descriptor's
  stream, no allocation, no synchronisation); under the poisoned-workspace procedure with every fill byte (the workspace is
  scratch and is zeroed inside the call: no result may depend on what it held); and with every output and the workspace
  between guard bands, at offsets 0 and 8.  The yardstick of the reference run is the restatement, tests/demos_ref.py."""
import numpy as np
import pytest

torch = pytest.importorskip('torch')

import demos_ref as R  # noqa: E402
import guard_bands as GB  # noqa: E402
import stale_workspace as W  # noqa: E402
import stream_order as S  # noqa: E402

pytestmark = pytest.mark.gpu
ENTRY = 'mfg_demos_from_logs'

# name: N, H, U, C, d, width, order
SHAPES = {'small': (2, 3, 257, 6, 2, 3, 'first_hour'),
          'chunks': (3, 4, 2 * 8192 + 1028, 47, 15, 20, 'total'),
          'given': (2, 3, 8192 + 5, 6, 3, 4, 'given')}
GIVEN = [3, -1, 0, 2, 1, -1]


def _log(name, salt):
    N, H, U, C = SHAPES[name][:4]
    rs = np.random.RandomState(91 + 1000 * salt)
    return np.minimum(rs.pareto(0.7, (N, H, U)).astype(np.int64), C - 1).astype(np.int32) - (rs.random_sample((N, H, U)) < 0.05)


def _call(ops, name, topic, given, out, ws):
    N, H, U, C, d, width, order = SHAPES[name]
    return lambda: ops.demos_from_logs(topic, C, d, width=width, order=order, order_given=given, out=out, workspace=ws)


def _row(name):
    with S.extra_rows() as rows:
        @S.row('demos_from_logs-' + name, ENTRY, work=((ENTRY, 'workspace', S.SCRATCH_KIND),))
        def build(a):
            ops = S._ops()
            N, H, U, C, d, width, order = SHAPES[name]
            topic = a.inp('topic', torch.as_tensor(_log(name, a.salt).astype(np.int32), device=a.dev))
            given = None
            if order == 'given':        # (the decoy ranks the categories the other way round)
                given = a.inp('order_given', torch.tensor([GIVEN[::-1] if a.salt else GIVEN], dtype=torch.int32, device=a.dev))
            out = {n: a.out(n, shape, dtype) for n, (shape, dtype) in ops.demos_shapes(N, H, C, d, width).items()}
            ws = a.ws(ops.demos_workspace_bytes(N, H, C, width))
            return _call(ops, name, topic, given, out, ws)
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
def test_the_reference_run_is_the_restatement(M, name):
    N, H, U, C, d, width, order = SHAPES[name]
    want = R.from_logs(_log(name, 0), C, d, width, order, np.array([GIVEN]) if order == 'given' else None)
    assert R.differing(M.ref[name].want, want) == []
    decoy = R.from_logs(_log(name, 1), C, d, width, order, np.array([GIVEN[::-1]]) if order == 'given' else None)
    assert all(not R.same(want[n], decoy[n]) for n in ('state', 'action', 'counts', 'moves'))


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
    N, H, U, C, d, width, order = SHAPES[name]
    topic = torch.as_tensor(_log(name, 0).astype(np.int32), device=M.dev)
    given = torch.tensor([GIVEN], dtype=torch.int32, device=M.dev) if order == 'given' else None
    g = {n: GB.Guarded(shape, dtype, M.dev, offset=offset, fill=float('nan') if dtype.is_floating_point else -7)
         for n, (shape, dtype) in ops.demos_shapes(N, H, C, d, width).items()}
    ws = GB.Guarded(ops.demos_workspace_bytes(N, H, C, width), torch.uint8, M.dev, offset=offset, fill=0xFF)
    _call(ops, name, topic, given, {n: x.t for n, x in g.items()}, ws.t)()
    torch.cuda.synchronize()
    GB.check_all(('workspace', ws), *g.items())
    assert S.differing({n: x.t for n, x in g.items()}, M.ref[name].want) == []
