"""-m gpu: mfg_demos_bootstrap and mfg_replicate_bands against their NumPy restatement (tests/demos_boot_ref.py), bit for bit --
every output with demos_ref.same (NaN equal to NaN), no tolerance; the mean and std of the bands too, because the restatement
adds in the call's order.  The shapes are the smallest at which the kernel can go wrong: agent counts round the wave, the
workgroup and the chunk, with and without the 16-byte load path; replicate counts round the Philox quad and the replicate
block; width 64, where a workgroup holds one replicate and the hours go in blocks; weighted cells past 65 535; a day of one
agent, where some replicates are empty.  Then the hazards (side stream, graph, stale workspace, guard bands) by the helper
modules of the existing hazard tests, and the Python layer with its consumers."""
import numpy as np
import pytest

torch = pytest.importorskip('torch')

import demos_boot_ref as B  # noqa: E402
import demos_ref as R  # noqa: E402
import guard_bands as GB  # noqa: E402
import stale_workspace as W  # noqa: E402
import stream_order as S  # noqa: E402

pytestmark = pytest.mark.gpu
CHUNK = 8192      # _lib.DEMOS_CHUNK
ENTRY = 'mfg_demos_bootstrap'


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.fail('-m gpu tests need a GPU: the HIP path has no CPU fallback')
    return torch.device('cuda:0')


def _ops():
    from discrete_mean_field_game_amd import ops
    return ops


def perm(seed, C):
    return np.random.RandomState(seed).permutation(C).astype(np.int32)[None]


def random_log(seed, N, H, U, lo, hi):
    return np.random.RandomState(seed).randint(lo, hi, size=(N, H, U)).astype(np.int32)


def run(dev, topic, rank, C, d, Rn, seed, **kw):
    got = _ops().demos_bootstrap(torch.as_tensor(topic, device=dev), torch.as_tensor(np.atleast_2d(rank).astype(np.int32), device=dev),
                                 C, d, Rn, seed, **kw)
    torch.cuda.synchronize()
    return {n: (None if t is None else t.cpu().numpy()) for n, t in got.items()}


def check(dev, topic, rank, C, d, Rn, seed, names=None, **kw):
    """The call on `topic` (NumPy) against the restatement; returns (device result as NumPy, restatement)."""
    got = run(dev, topic, rank, C, d, Rn, seed, **kw)
    kw.pop('groups', None)
    want = B.bootstrap(topic, rank, C, d, Rn, seed, **kw)
    assert R.differing(got, want, names or B.OUTPUTS) == []
    return got, want


@pytest.mark.parametrize('U', [1, 63, 64, 65, 257, 1025, CHUNK, CHUNK + 1, 2 * CHUNK + 1028])
def test_agent_counts_round_every_width_of_the_kernel(dev, U):
    from discrete_mean_field_game_amd import _lib
    assert _lib.DEMOS_CHUNK == CHUNK
    got, _ = check(dev, random_log(U, 2, 3, U, -1, 5), perm(1, 5), 5, 3, 5, 77)
    assert not (got['status'] & R.BAD_VALUE).any() and (got['present'] <= 12 * U).all()


@pytest.mark.parametrize('Rn', [1, 3, 4, 5, 9, 17])
def test_replicate_counts_round_the_quad_and_the_block(dev, Rn):
    """A partial Philox quad, a partial replicate block, more than two blocks (9 = 2 x 4 + 1); at width 64 a block is one
    replicate, so every R > 2 spans more than two there (test_widths)."""
    got, _ = check(dev, random_log(30 + Rn, 2, 3, 1025, -1, 7), perm(2, 7), 7, 3, Rn, 5, width=4)
    if Rn > 1:
        assert not R.same(got['counts'][0], got['counts'][Rn - 1])


@pytest.mark.parametrize('H', [2, 3, 16])
def test_hours(dev, H):
    check(dev, random_log(40 + H, 2, H, CHUNK + 257, -1, 6), perm(3, 6), 6, 3, 5, 6, width=5)


@pytest.mark.parametrize('width, C, d, H', [(1, 1, 1, 3), (1, 9, 1, 3), (20, 47, 15, 16), (64, 4096, 64, 6), (64, 100, 21, 7)])
def test_widths(dev, width, C, d, H):
    """width = 64: the tiles of three transitions of ONE replicate fit in LDS: blocks of 3 + 2 and 3 + 3 hours, the first hour
    of a block read again, and R = 3 is three replicate blocks."""
    lo = 0 if C == 1 else -2
    topic = np.minimum(np.random.RandomState(50 + width + H).pareto(0.5, (2, H, CHUNK + 77)).astype(np.int64), C - 1).astype(np.int32)
    topic[:, :, ::7] = lo
    check(dev, topic, perm(4, C), C, d, 3, 8, width=width)


@pytest.mark.parametrize('groups', [1, 2, 3])
def test_groups_change_nothing(dev, groups):
    check(dev, random_log(20, 2, 4, 4 * CHUNK + 331, -1, 7), perm(5, 7), 7, 3, 5, 9, width=5, groups=groups)


@pytest.mark.parametrize('unit', B.UNITS)
def test_units_and_a_seed_past_2_to_the_32(dev, unit):
    seed = (0xABCD << 32) | 0x1234
    topic = random_log(60, 3, 3, 1025, -1, 6)
    got, _ = check(dev, topic, perm(6, 6), 6, 3, 4, seed, unit=unit, day_offset=5)
    low = run(dev, topic, perm(6, 6), 6, 3, 4, seed & 0xFFFFFFFF, unit=unit, day_offset=5)
    assert not R.same(got['counts'], low['counts'])
    same_log = np.broadcast_to(topic[:1], topic.shape).copy()
    got = run(dev, same_log, perm(6, 6), 6, 3, 4, seed, unit=unit)
    assert R.same(got['counts'][:, 0], got['counts'][:, 1]) == (unit == 'agent')


def test_days_in_chunks_by_day_offset(dev):
    topic, rank = random_log(61, 4, 3, CHUNK + 5, -1, 6), np.stack([perm(s, 6)[0] for s in range(4)])
    whole, _ = check(dev, topic, rank, 6, 3, 5, 12, day_offset=(1 << 33) + 1)
    a = run(dev, topic[:2], rank[:2], 6, 3, 5, 12, day_offset=(1 << 33) + 1)
    b = run(dev, topic[2:], rank[2:], 6, 3, 5, 12, day_offset=(1 << 33) + 3)
    for name in B.OUTPUTS:
        assert R.same(np.concatenate([a[name], b[name]], axis=1), whole[name]), name


def test_weighted_cells_past_65535(dev):
    U = 70_001
    one = np.full((1, 3, U), 2, np.int32)
    got, _ = check(dev, one, np.array([1, 2, 0, 3, 4]), 5, 3, 4, 21)
    cell = got['moves'][:, 0, 0, 0, 0]
    assert (cell > 65_535).all() and len(set(cell.tolist())) == 4 and (got['counts'][:, 0, 2, 0] == cell).all()
    two = np.broadcast_to(((np.arange(U) // 4) % 2).astype(np.int32) * 3, (1, 3, U)).copy()
    check(dev, two, np.arange(5), 5, 4, 4, 22)


def test_absent_and_bad_values_and_ranks(dev):
    topic = random_log(62, 3, 3, 1025, -3, 8)                          # values 6, 7 >= C
    topic[1] = np.clip(topic[1], -1, 5)
    rank = np.array([[2, -1, 0, 4, 1, 3]] * 3)                         # a dropped category; rank 4 >= width
    got, _ = check(dev, topic, rank, 6, 2, 5, 13, width=4)
    assert (got['status'] & R.BAD_VALUE).T.tolist() == [[1] * 5, [0] * 5, [1] * 5]
    rank[1] = [0, 1, 6, -2, 2, 3]                                      # outside [-1, C): dropped, bit 0
    got, _ = check(dev, topic, rank, 6, 2, 5, 13, width=4)
    assert (got['status'] & R.BAD_VALUE).all()
    check(dev, topic, rank[:1], 6, 2, 5, 13, width=4)                  # one row for every day


def test_empty_replicates_are_nan_rows(dev):
    """U = 1: the replicates in which the one agent has weight 0 are empty at every hour.  Seed 1 gives both kinds on both days
    (checked with the restatement)."""
    w = B.weights(8, 2, 1, 1)[:, :, 0]
    assert (w == 0).any(0).all() and (w > 0).any(0).all()
    got, _ = check(dev, np.zeros((2, 3, 1), np.int32), [0, 1], 2, 2, 8, 1)
    assert ((got['status'] & R.EMPTY_HOUR) != 0).tolist() == (w == 0).tolist()
    assert np.isnan(got['state'][w == 0]).all() and not np.isnan(got['state'][w > 0]).any()


def test_null_outputs_change_no_other_output(dev):
    topic, rank = random_log(63, 2, 4, CHUNK + 3, -1, 6), perm(7, 6)
    full, _ = check(dev, topic, rank, 6, 3, 5, 14, width=4)
    for want in (('state',), ('action', 'left'), ('counts',), ('moves', 'entered', 'present'), ()):
        got = run(dev, topic, rank, 6, 3, 5, 14, width=4, want=want)
        for name in B.OUTPUTS:
            if name in want or name == 'status':
                assert R.same(got[name], full[name]), (want, name)
            else:
                assert got[name] is None


# ------------------------------------------------------------------------------------------------------------------ hazards
# name: N, H, U, C, d, width, R, unit
SHAPES = {'small': (2, 3, 257, 6, 2, 3, 5, 'agent_day'),
          'chunks': (3, 4, 2 * CHUNK + 1028, 47, 15, 20, 6, 'agent'),
          'wide': (1, 6, CHUNK + 5, 100, 21, 64, 2, 'agent_day')}


def _log(name, salt):
    N, H, U, C = SHAPES[name][:4]
    rs = np.random.RandomState(91 + 1000 * salt)
    return np.minimum(rs.pareto(0.7, (N, H, U)).astype(np.int64), C - 1).astype(np.int32) - (rs.random_sample((N, H, U)) < 0.05)


def _rank(name, salt):
    C = SHAPES[name][3]
    return np.arange(C, dtype=np.int32)[None, ::-1].copy() if salt else np.arange(C, dtype=np.int32)[None]


def _call(ops, name, topic, rank, out, ws):
    N, H, U, C, d, width, Rn, unit = SHAPES[name]
    return lambda: ops.demos_bootstrap(topic, rank, C, d, Rn, 0x500000007, width=width, unit=unit, out=out, workspace=ws)


def _row(name):
    with S.extra_rows() as rows:
        @S.row('demos_bootstrap-' + name, ENTRY, work=((ENTRY, 'workspace', S.SCRATCH_KIND),))
        def build(a):
            ops = S._ops()
            N, H, U, C, d, width, Rn, unit = SHAPES[name]
            topic = a.inp('topic', torch.as_tensor(_log(name, a.salt).astype(np.int32), device=a.dev))
            rank = a.inp('rank', torch.as_tensor(_rank(name, a.salt), device=a.dev))
            out = {n: a.out(n, shape, dtype) for n, (shape, dtype) in ops.demos_boot_shapes(Rn, N, H, d, width).items()}
            ws = a.ws(ops.demos_bootstrap_workspace_bytes(Rn, N, H, C, width))
            return _call(ops, name, topic, rank, out, ws)
    return rows[0]


class _Module:
    pass


@pytest.fixture(scope='module')
def M(dev):
    m = _Module()
    m.dev = dev
    m.rows = {name: _row(name) for name in SHAPES}
    m.ref = {name: S.reference(r, m.dev) for name, r in m.rows.items()}
    m.cycles = int(max(20.0, 10e3 * max(r.enqueue_s for r in m.ref.values())) * S.sleep_cycles_per_ms())
    m.side = S.independent_side_stream(m.dev, m.cycles)
    return m


@pytest.mark.parametrize('name', sorted(SHAPES))
def test_the_reference_run_is_the_restatement(M, name):
    N, H, U, C, d, width, Rn, unit = SHAPES[name]
    want = B.bootstrap(_log(name, 0), _rank(name, 0), C, d, Rn, 0x500000007, width, unit)
    assert R.differing(M.ref[name].want, want) == []
    decoy = B.bootstrap(_log(name, 1), _rank(name, 1), C, d, Rn, 0x500000007, width, unit)
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
    ops = _ops()
    N, H, U, C, d, width, Rn, unit = SHAPES[name]
    topic = torch.as_tensor(_log(name, 0).astype(np.int32), device=M.dev)
    rank = torch.as_tensor(_rank(name, 0), device=M.dev)
    g = {n: GB.Guarded(shape, dtype, M.dev, offset=offset, fill=float('nan') if dtype.is_floating_point else -7)
         for n, (shape, dtype) in ops.demos_boot_shapes(Rn, N, H, d, width).items()}
    ws = GB.Guarded(ops.demos_bootstrap_workspace_bytes(Rn, N, H, C, width), torch.uint8, M.dev, offset=offset, fill=0xFF)
    _call(ops, name, topic, rank, {n: x.t for n, x in g.items()}, ws.t)()
    torch.cuda.synchronize()
    GB.check_all(('workspace', ws), *g.items())
    assert S.differing({n: x.t for n, x in g.items()}, M.ref[name].want) == []
    # the tables in the workspace instead of the caller's arrays: the same floats, the workspace still inside its bands
    for n in ('counts', 'moves'):
        g.pop(n)
    for x in g.values():
        x.t.fill_(float('nan') if x.t.dtype.is_floating_point else -7)
    ops.demos_bootstrap(topic, rank, C, d, Rn, 0x500000007, width=width, unit=unit, out={n: x.t for n, x in g.items()}, workspace=ws.t,
                        want=tuple(g))
    torch.cuda.synchronize()
    GB.check_all(('workspace', ws), *g.items())
    assert S.differing({n: x.t for n, x in g.items()}, {n: M.ref[name].want[n] for n in g}) == []


# -------------------------------------------------------------------------------------------------------------------- bands
@pytest.mark.parametrize('Rn', [1, 2, 17, 64, 1024])
def test_replicate_bands(dev, Rn):
    """Against NumPy: sums in the order r = 0 .. R - 1 (np.cumsum), so mean and std are bit exact too; quantiles are
    np.sort(...)[rank].  Ties (values on a grid of 8), a NaN cell, repeated and unsorted ranks, 37 cells (16 + 16 + 5)."""
    rs = np.random.RandomState(Rn)
    x = (rs.randint(0, 8, (Rn, 37)) / np.float32(8)).astype(np.float32)
    x[:, 20:] = rs.random_sample((Rn, 17)).astype(np.float32)
    x[Rn // 2, 5] = np.nan
    x[:, 7] = 0.25
    ranks = [Rn - 1, 0, Rn // 2, 0, Rn // 3]
    got = _ops().replicate_bands(torch.as_tensor(x.reshape(Rn, 37, 1), device=dev), ranks)
    want = B.bands(x.reshape(Rn, 37, 1), ranks)
    for g, w, name in zip(got, want, ('mean', 'std', 'quant')):
        assert R.same(g.cpu().numpy(), w), name
    mean, std, quant = (t.cpu().numpy() for t in _ops().replicate_bands(torch.as_tensor(x, device=dev)))
    assert R.same(mean, want[0][:, 0]) and R.same(std, want[1][:, 0]) and quant.shape == (0, 37)
    assert np.isnan(mean[5]) and std[7] == 0


# ------------------------------------------------------------------------------------------------------------ the Python layer
@pytest.fixture(scope='module')
def boot(dev):
    from discrete_mean_field_game_amd import demos as D
    rs = np.random.RandomState(14)
    P, pi0 = rs.dirichlet(2 * np.ones(15), (15, 15)), rs.dirichlet(5 * np.ones(15))
    t = np.stack([R.simulate_logs(P, pi0, 3000, 16, seed) for seed in range(6)])
    return t, D.bootstrap(t, 15, 3, seed=7, device=dev)


def test_bootstrap_is_the_restatement_and_its_sample_is_from_logs(dev, boot):
    from discrete_mean_field_game_amd import demos as D
    t, b = boot
    sample = D.from_logs(t, 15, device=dev)
    for name in D.ARRAYS:
        assert R.same(getattr(b.sample, name), getattr(sample, name)), name
    ref = R.from_logs(t, 15, 15)
    rank = np.empty_like(ref['order'])
    for n in range(6):
        rank[n, ref['order'][n]] = np.arange(15)
    want = B.bootstrap(t, rank, 15, 15, 3, 7)
    assert b.R == 3
    for r in range(3):
        rep = b.replicate(r)
        for name in B.OUTPUTS:
            assert R.same(getattr(rep, name), want[name][r]), (name, r)
        assert R.same(rep.order, sample.order)
    assert R.same(b.emp([1, 4]), want['state'][:, [1, 4]].astype(np.float64))
    assert R.same(b.days_table()[b.day_index(2, [0, 5])], b.replicate(2).emp([0, 5]))
    bands = b.bands((0, 2))
    for name in ('state', 'action'):
        for g, w in zip(bands[name], B.bands(want[name], (0, 2))):
            assert R.same(g, w), name
    low, high = b.interval(0.9)['state']
    assert b.interval_ranks(0.9) == (0, 2) and (low <= b.sample.state).mean() > 0.5 and (low <= high).all()


def test_chunked_and_transposed_calls_change_no_bit(dev, boot):
    from discrete_mean_field_game_amd import demos as D
    t, b = boot
    per_day = D.bootstrap_day_bytes(16, 3000, 15, 15, 3)
    small = D.bootstrap(t, 15, 3, seed=7, device=dev, budget=2 * per_day + 1)
    nuh = D.bootstrap(np.ascontiguousarray(t.transpose(0, 2, 1)), 15, 3, seed=7, device=dev, layout='nuh')
    for other in (small, nuh):
        for name in D.BOOT_ARRAYS:
            assert R.same(getattr(other, name), getattr(b, name)), name
        assert R.same(other.sample.state, b.sample.state)
    with pytest.raises(ValueError):
        D.bootstrap(t, 15, 3, order='total', device=dev, budget=2 * per_day + 1)
    given = D.bootstrap(t, 15, 3, seed=7, order='given', order_given=np.arange(15), device=dev)
    assert R.same(given.counts, B.bootstrap(t, np.arange(15), 15, 15, 3, 7)['counts'])


def test_consumers_take_replicates(dev, boot):
    import random
    from discrete_mean_field_game_amd import var
    from discrete_mean_field_game_amd.ac_irl import AC_IRL
    t, b = boot
    table = b.days_table()
    assert table.shape == (18, 16, 15)
    one = var.fit_population(table, [1, 1, 1], 1e-2, [b.day_index(r, [0, 1, 2, 3]) for r in range(3)],
                             [b.day_index(r, [4, 5]) for r in range(3)], 'rolling', device=dev)
    for r in range(3):
        alone = var.fit_population(b.replicate(r).emp(), [1], 1e-2, [0, 1, 2, 3], [4, 5], 'rolling', device=dev)
        for name in ('coef', 'sse', 'insample', 'future', 'per_day', 'metrics', 'status'):
            assert R.same(np.asarray(getattr(one, name))[r], np.asarray(getattr(alone, name))[0]), (name, r)
    rep = b.replicate(1)
    np.random.seed(11); torch.manual_seed(11); random.seed(3)
    ac = AC_IRL(d=15, pi0=rep.pi0(), demonstrations=rep.demonstrations(), batch=8, seed=5, verbose=0)
    ac.list_generated = ac.generate_trajectories(5)
    before = ac._trainer.flat.clone()
    ac.update_reward()
    assert bool(torch.isfinite(ac._trainer.flat).all()) and not torch.equal(before, ac._trainer.flat)
