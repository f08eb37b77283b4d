"""-m gpu: mfg_demos_from_logs against its NumPy restatement (tests/demos_ref.py), bit for bit -- integers and floats alike are
compared with array_equal (NaN equal to NaN); no tolerance appears.  The shapes are the smallest at which the kernels can go
wrong: agent counts round the wave, the workgroup and the chunk, with and without the 16-byte load path (U a multiple of 4 or
not); one cell past 65 535 flushed from several workgroups; ties, C = 1 and C = 4 096; the second mode on the integers of
ops.agents_step_pop; the consumers; and one log past 2^31 elements whose counts have a closed form."""
import numpy as np
import pytest

torch = pytest.importorskip('torch')

import demos_ref as R  # noqa: E402
import large_buffers as LB  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.fail('-m gpu tests need a GPU: the HIP path has no CPU fallback')
    return torch.device('cuda:0')


def _ops():
    from discrete_mean_field_game_amd import _lib, ops
    return ops, _lib


def check(dev, topic, C, d, names=None, **kw):
    """The call on `topic` (NumPy) against the restatement; returns (device result as NumPy, restatement)."""
    ops, _ = _ops()
    dkw = dict(kw)
    if dkw.get('order_given') is not None:
        dkw['order_given'] = torch.as_tensor(np.atleast_2d(dkw['order_given']).astype(np.int32), device=dev)
    got = ops.demos_from_logs(torch.as_tensor(topic, device=dev), C, d, **dkw)
    torch.cuda.synchronize()
    got = {n: (None if t is None else t.cpu().numpy()) for n, t in got.items()}
    kw.pop('lds_update', None), kw.pop('groups', None)
    want = R.from_logs(topic, C, d, **kw)
    assert R.differing(got, want, names) == []
    return got, want


def random_log(seed, N, H, U, lo, hi):
    return np.random.RandomState(seed).randint(lo, hi, size=(N, H, U)).astype(np.int32)


CHUNK = 8192      # _lib.DEMOS_CHUNK (asserted below)


@pytest.mark.parametrize('U', [1, 63, 64, 65, 255, 257, 1025, CHUNK, CHUNK + 1, 3 * CHUNK + 77, 2 * CHUNK + 1028])
@pytest.mark.parametrize('lds_update', ['combine', 'plain'])
def test_agent_counts_round_every_width_of_the_kernel(dev, U, lds_update):
    assert _ops()[1].DEMOS_CHUNK == CHUNK
    got, _ = check(dev, random_log(U, 2, 3, U, -1, 5), 5, 3, lds_update=lds_update)
    assert not (got['status'] & R.BAD_VALUE).any() and (got['present'] <= U).all()


@pytest.mark.parametrize('groups', [1, 2, 3])
def test_workgroups_that_take_several_chunks_and_hours_in_blocks(dev, groups):
    """Five chunks of a day (the last one ragged) on 1, 2 and 3 workgroups; then width = 64 with H = 7, where the tiles of three
    transitions fit in LDS at a time: blocks of 3 + 3 hours, and with H = 6 of 3 + 2, the first hour of a block read again."""
    check(dev, random_log(20, 2, 4, 4 * CHUNK + 331, -1, 7), 7, 3, width=5, groups=groups)
    check(dev, random_log(21, 2, 4, 4 * CHUNK + 332, -1, 7), 7, 3, width=5, groups=groups, order='total')
    for H in (6, 7):
        check(dev, random_log(22 + H, 1, H, 2 * CHUNK + 77, -2, 100), 100, 64, groups=groups)


@pytest.mark.parametrize('U', [70_000, 70_001])
@pytest.mark.parametrize('lds_update', ['combine', 'plain'])
def test_one_cell_past_65535_and_two_cells_alternating(dev, U, lds_update):
    """Every agent in ONE category at every hour: one diagonal cell of 70 000, flushed from nine workgroups; then two
    categories alternating by agent parity, and by the parity of the agent's group of four (the 16-byte path gives a lane four
    consecutive agents)."""
    one = np.full((1, 3, U), 2, np.int32)
    got, _ = check(dev, one, 5, 3, lds_update=lds_update)
    assert got['moves'][0, 0, 0, 0] == U and got['counts'][0, 2, 0] == U
    u = np.arange(U)
    for pattern in (u % 2, (u // 4) % 2, (u // 64) % 2):
        two = np.broadcast_to(pattern.astype(np.int32) * 3, (1, 3, U)).copy()
        two[0, 1] = 3 - two[0, 1]                                        # everybody changes category and changes back
        got, _ = check(dev, two, 5, 3, lds_update=lds_update)
        assert got['moves'][0, 0].sum() == U and got['moves'][0, 0, 0, 0] == 0


def test_absent_and_bad_values(dev):
    t = random_log(1, 2, 4, 300, -3, 5)                                  # negative values: absent
    got, _ = check(dev, t, 5, 3)
    assert not got['status'].any() and got['left'].any() and got['entered'].any()
    t[0, 2, 17], t[0, 0, 299] = 5, 2 ** 31 - 1                           # values >= C: absent, bit 0, the other day clean
    got, _ = check(dev, t, 5, 3)
    assert got['status'].tolist() == [R.BAD_VALUE, 0]
    t = random_log(2, 2, 4, 300, 0, 5)
    t[1, 2] = -1                                                         # an hour with nobody present
    got, _ = check(dev, t, 5, 3)
    assert got['status'].tolist() == [0, R.EMPTY_HOUR] and np.isnan(got['state'][1, 2]).all() and got['present'][1, 2] == 0


@pytest.mark.parametrize('empty_row', ['uniform', 'identity'])
def test_empty_rows(dev, empty_row):
    ident = np.arange(4)
    t = random_log(3, 1, 3, 200, 0, 2)                                   # ranks 2 and 3: a row nobody is in
    t[0, 0, :5] = 2
    t[0, 1, :5] = -1                                                     # rank 2 at hour 0: all its agents leave
    got, _ = check(dev, t, 4, 4, order='given', order_given=ident, empty_row=empty_row)
    a = got['action'][0, 0]
    assert a[2].tolist() == [0, 0, 1, 0]                                 # counts > 0: identity under either setting
    assert a[3].tolist() == ([0.25] * 4 if empty_row == 'uniform' else [0, 0, 0, 1])
    assert got['left'][0, 0].tolist() == [0, 0, 5, 0]


def test_ordering(dev):
    # ties, ties at 0 included: 8 categories, three of them populated equally at hour 0
    t = np.repeat(np.array([6, 1, 4], np.int32), 50)[None, None, :].repeat(3, 1)
    t[0, 1] = t[0, 1, ::-1]
    got, _ = check(dev, t, 8, 3, width=5)
    assert got['order'].tolist() == [[1, 4, 6, 0, 2, 3, 5, 7]]
    got, _ = check(dev, np.zeros((2, 3, 70), np.int32), 1, 1)                                   # C = 1
    assert (got['state'] == 1).all() and (got['action'] == 1).all()
    zipf = lambda seed, C, shape: np.minimum((np.random.RandomState(seed).pareto(0.6, shape)).astype(np.int64), C - 1).astype(np.int32)
    check(dev, zipf(0, 4096, (2, 3, 30_000)), 4096, 64)                                         # C = 4 096, width = 64 = d
    check(dev, zipf(1, 47, (2, 4, 9_000)), 47, 15, width=20)                                    # the reference's own widths
    # days whose first hours disagree: 'total' gives one ranking, 'first_hour' one per day
    t = random_log(5, 2, 3, 500, 0, 6)
    t[0, 0, :400], t[1, 0, :400] = 4, 1
    a, _ = check(dev, t, 6, 3, order='total')
    b, _ = check(dev, t, 6, 3, order='first_hour')
    assert (a['order'][0] == a['order'][1]).all() and b['order'][0, 0] == 4 and b['order'][1, 0] == 1
    # a given table with dropped categories (one row for all days), and with an out-of-range rank on one day only
    got, _ = check(dev, t, 6, 2, width=3, order='given', order_given=np.array([2, -1, 0, -1, 1, 3]))
    assert got['order'].tolist() == [[2, 4, 0, 5, -1, -1]] * 2 and not got['status'].any()
    got, _ = check(dev, t, 6, 2, width=3, order='given', order_given=np.array([[2, -1, 0, -1, 1, 3], [2, 6, 0, -7, 1, 3]]))
    assert got['status'].tolist() == [0, R.BAD_VALUE]


def test_two_hours_and_one_topic(dev):
    check(dev, random_log(6, 3, 2, 333, -1, 4), 4, 2, width=3)                                  # H = 2
    check(dev, random_log(7, 2, 5, 333, -1, 4), 4, 1)                                           # d = 1 = width
    check(dev, random_log(8, 2, 5, 333, -1, 4), 4, 1, width=4)


def test_a_day_does_not_depend_on_its_neighbours_or_its_position(dev):
    ops, _ = _ops()
    t = random_log(9, 5, 4, 2 * CHUNK + 5, -1, 7)
    t[3, 1, 0] = 9                                                       # a bad value on day 3 only
    whole, _ = check(dev, t, 7, 3, width=5)
    assert whole['status'].tolist() == [0, 0, 0, R.BAD_VALUE, 0]
    for n in range(5):
        alone = ops.demos_from_logs(torch.as_tensor(t[n:n + 1], device=dev), 7, 3, width=5)
        assert R.differing(alone, {name: a[n:n + 1] for name, a in whole.items()}) == []


def test_agent_major_input_is_transposed_on_the_device(dev):
    from discrete_mean_field_game_amd import demos as D
    t = random_log(10, 3, 4, 777, -1, 6)
    a = D.from_logs(t, 3, categories=6, width=4, device=dev)
    b = D.from_logs(np.ascontiguousarray(t.transpose(0, 2, 1)), 3, categories=6, width=4, layout='nuh', device=dev)
    c = D.from_logs(torch.as_tensor(t, device=dev).long(), 3, width=4, budget=4 * 777 * 4)      # a tensor, max + 1, a day per chunk
    want = R.from_logs(t, 6, 3, 4)
    for dm in (a, b, c):
        assert R.differing({n: getattr(dm, n) for n in want}, want) == []
    g = D.from_logs(t, 3, categories=6, order='given', order_given=[0, 1, 2, -1, -1, -1], budget=2 * 4 * 777 * 4, device=dev)
    want = R.from_logs(t, 6, 3, order='given', order_given=np.array([0, 1, 2, -1, -1, -1]))
    assert R.differing({n: getattr(g, n) for n in want}, want) == []
    with pytest.raises(ValueError):
        D.from_logs(t, 3, categories=6, order='total', budget=4 * 777 * 4, device=dev)


def test_outputs_left_null_change_no_other_output(dev):
    ops, _ = _ops()
    t = random_log(11, 2, 4, CHUNK + 9, -1, 6)
    want = R.from_logs(t, 6, 3, 4)
    td = torch.as_tensor(t, device=dev)
    for names in (('state',), ('action', 'left'), ('counts', 'entered'), ('moves', 'present'), ()):
        got = ops.demos_from_logs(td, 6, 3, width=4, want=names)
        keep = tuple(names) + ('order', 'status')
        assert all(got[n] is None for n in want if n not in keep) and R.differing(got, want, keep) == []


def test_second_mode_on_the_integers_of_a_finite_population_step(dev):
    ops, L = _ops()
    K, B, d, A = 2, 3, 21, 1000
    rs = np.random.RandomState(12)
    counts = torch.as_tensor(rs.multinomial(A, rs.dirichlet(np.ones(d)), size=(K, B)).astype(np.int32), device=dev)
    P = torch.as_tensor(rs.dirichlet(np.ones(d), size=(K, B, d)).astype(np.float32), device=dev)
    P[1, 2, int(counts[1, 2].argmax())] = 0.0                            # an unusable row: member (1, 2) fails
    seeds = torch.tensor([11, 12], dtype=torch.int64, device=dev)
    nxt, _, moves = ops.agents_step_pop(counts, P, A, seeds, want_moves=True)
    both = torch.stack([counts.reshape(K * B, d), nxt.reshape(K * B, d)], 1).contiguous()
    mv = moves.reshape(K * B, 1, d, d).contiguous()
    for empty_row in ('uniform', 'identity'):
        got = ops.demos_from_moves(both, mv, empty_row=empty_row)
        want = R.finish(both.cpu().numpy(), mv.cpu().numpy(), d, empty_row)
        assert R.differing(got, want) == []
    st = got['status'].cpu().numpy()
    assert st.tolist() == [0] * 5 + [L.DEMOS_FAILED] and bool(torch.isnan(got['state'][5]).all()) and bool(torch.isnan(got['action'][5]).all())
    assert not got['left'][:5].any() and not got['entered'][:5].any() and bool((got['present'][:5] == A).all())
    from discrete_mean_field_game_amd import demos as D
    dm = D.from_agents_step(counts, nxt, moves)
    assert R.differing({n: getattr(dm, n) for n in want}, R.finish(both.cpu().numpy(), mv.cpu().numpy(), d)) == []
    assert dm.closed().tolist() == [True] * 5 + [False] and dm.order is None


def test_a_closed_population(dev):
    rs = np.random.RandomState(13)
    P, pi0 = rs.dirichlet(2 * np.ones(5), (3, 5)), rs.dirichlet(5 * np.ones(5))
    t = np.stack([R.simulate_logs(P, pi0, 5000, 4, seed) for seed in (0, 1)])
    got, _ = check(dev, t, 5, 5)
    assert not got['left'].any() and not got['entered'].any()
    ratio = np.float32(np.float64(got['counts'][:, 1:]) / np.float64(5000))
    assert R.same(got['state'][:, 1:], ratio[:, :, :])                   # (rank order: the columns of counts are the state's)


@pytest.fixture(scope='module')
def recorded(dev):
    """d = 15, H = 16, 6 days of U = 5 000 simulated agents."""
    from discrete_mean_field_game_amd import demos as D
    rs = np.random.RandomState(14)
    P, pi0 = rs.dirichlet(2 * np.ones(15), (15, 15)), rs.dirichlet(5 * np.ones(15))
    t = np.stack([R.simulate_logs(P, pi0, 5000, 16, seed) for seed in range(6)])
    return D.from_logs(t, 15, device=dev)


def test_consumer_ac_irl_takes_the_demonstrations(dev, recorded):
    import random
    from discrete_mean_field_game_amd.ac_irl import AC_IRL
    trajs = recorded.demonstrations()
    assert len(trajs) == 6 and all(len(tr) == 15 for tr in trajs) and trajs[0][0][0].dtype == np.float64
    assert recorded.closed().all() and recorded.pi0().shape == (6, 15)
    np.random.seed(11); torch.manual_seed(11); random.seed(3)
    ac = AC_IRL(d=15, pi0=recorded.pi0(), demonstrations=trajs, batch=8, seed=5, verbose=0)
    ac.list_generated = ac.generate_trajectories(5)
    before = ac._trainer.flat.clone()
    ac.update_reward()
    after = ac._trainer.flat
    assert bool(torch.isfinite(after).all()) and not torch.equal(before, after)


def test_consumers_var_and_rnn_take_the_day_table(dev, recorded):
    from discrete_mean_field_game_amd import rnn, var
    emp = recorded.emp()
    assert emp.shape == (6, 16, 15) and np.abs(emp.sum(-1) - 1).max() < 1e-6
    fits = var.fit_population(emp, [1, 2], 1e-2, [0, 1, 2, 3], [4, 5], 'rolling', device=dev)
    assert not np.asarray(fits.status).any()
    fits = rnn.fit_population(emp, [8], 1e-2, 2, [0, 1, 2, 3], [4], [5], device=dev)
    assert not np.asarray(fits.status).any()


def test_a_log_past_2_to_the_31_elements(dev):
    """N = 1, H = 17, U = 2^27 + 1, C = width = d = 8, a given identity order, topic = (u + h) mod 8 written hour by hour on the
    device: every agent of i moves to (i + 1) mod 8, so counts and moves have a closed form; nothing of that size is rebuilt on
    the host.  9.1 GB."""
    ops, _ = _ops()
    H, U = 17, 2 ** 27 + 1
    assert H * U > 2 ** 31
    LB.require_free(H * U * 4 + 3 * U * 8)
    topic = torch.empty((1, H, U), dtype=torch.int32, device=dev)
    u = torch.arange(U, dtype=torch.int32, device=dev)
    for h in range(H):
        torch.remainder(u + h, 8, out=topic[0, h])
    del u
    got = ops.demos_from_logs(topic, 8, 8, order='given', order_given=torch.arange(8, dtype=torch.int32, device=dev)[None])
    torch.cuda.synchronize()
    del topic
    torch.cuda.empty_cache()
    i = np.arange(8)
    counts = np.stack([2 ** 24 + (i == (2 ** 27 + h) % 8) for h in range(H)]).astype(np.int32)[None]     # agent 2^27 is the odd one
    moves = np.zeros((1, H - 1, 8, 8), np.int32)
    for h in range(H - 1):
        moves[0, h, i, (i + 1) % 8] = counts[0, h]
    want = R.finish(counts, moves, 8)
    want.update(counts=counts, moves=moves, order=np.arange(8, dtype=np.int32)[None])
    assert R.differing(got, want) == [] and not want['left'].any() and not want['entered'].any() and not want['status'].any()
