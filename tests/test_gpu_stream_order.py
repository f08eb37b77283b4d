"""-m gpu: every entry point enqueues all of its work on the stream it is given, and neither allocates nor synchronises.

Almost every other test runs on torch's default stream -- the null stream -- where a launch site that passes 0 instead of the
caller's stream, a driver that puts one launch of its chain elsewhere, or a hidden synchronise all give the same bits as correct
code.  Here every row of the call table (tests/stream_order.py; tests/test_stream_order_host.py checks that it covers the header)
runs twice off the default stream:

  A. behind a delayed producer on a non-blocking side stream: sleep kernel, device copies of the true inputs over valid decoys,
     the call, clones.  The producer must still be pending when the call returns (else the case fails as inconclusive), and the
     clones must equal, bit for bit, the default-stream reference.
  B. captured into a graph on decoy buffers (nothing may run at capture; a synchronise, an allocation or a legacy-stream launch is
     a capture error), then replayed twice on the true data, the second time without re-zeroing the workspace.

The delay is 10 x the slowest non-draining row's warm enqueue time, at least 20 ms, in cycles of torch.cuda._sleep's measured
clock.  Two negative controls hand the call the default stream's handle while the producer sits on the side stream: the harness
must report the differing buffers by name.
"""
import numpy as np
import pytest

torch = pytest.importorskip('torch')

import stream_order as S

pytestmark = pytest.mark.gpu

MIN_DELAY_MS, JITTER = 20.0, 10.0
IDS = [r.name for r in S.ROWS]


class _Module:
    pass


@pytest.fixture(scope='module')
def M():
    """The device, every row's reference (computed once, read only) and the delay."""
    if not torch.cuda.is_available():
        pytest.fail('-m gpu tests need a GPU: the HIP path has no CPU fallback')
    S._ops().init()             # the lazy h-table fit is by design a stream-0 launch and a device synchronise: not in any case
    m = _Module()
    m.dev = torch.device('cuda:0')
    m.ref = {r.name: S.reference(r, m.dev) for r in S.ROWS}
    m.cycles_per_ms = S.sleep_cycles_per_ms()
    slow = max((r for r in S.ROWS if not r.drains), key=lambda r: m.ref[r.name].enqueue_s)
    m.slowest_ms = 1e3 * m.ref[slow.name].enqueue_s
    m.delay_ms = max(MIN_DELAY_MS, JITTER * m.slowest_ms)
    m.cycles = int(m.delay_ms * m.cycles_per_ms)
    m.side = S.independent_side_stream(m.dev, m.cycles)
    print('\nstream order: %d rows; _sleep clock %.0f cycles/ms; slowest enqueue %.3f ms (%s); delay %.1f ms'
          % (len(S.ROWS), m.cycles_per_ms, m.slowest_ms, slow.name, m.delay_ms))
    return m


@pytest.mark.parametrize('r', S.ROWS, ids=IDS)
def test_call_runs_behind_a_delayed_producer(M, r):
    pending, got = S.run_delayed(r, M.ref[r.name], M.dev, M.cycles, M.side)
    if not r.drains:
        assert pending, ('%s: inconclusive -- the producer (%.1f ms) had finished when the call returned, or the call waited '
                         'for it: a hidden synchronise' % (r.name, M.delay_ms))
    bad = S.differing(got, M.ref[r.name].want)
    assert not bad, '%s: %s differ from the default-stream run: part of the call ran ahead of the stream it was given' % (r.name, bad)


@pytest.mark.parametrize('r', [r for r in S.ROWS if not r.drains], ids=[r.name for r in S.ROWS if not r.drains])
def test_call_is_capturable_and_replays(M, r):
    found = S.run_captured(r, M.ref[r.name], M.dev, M.side)
    assert not found, '%s: %s' % (r.name, found)


@pytest.mark.parametrize('name,buffers', [('step_given_P-d21-B13', ['pi_next', 'reward']),
                                          ('td_pg_accumulate-d21-acc0', ['G', 'delta', 'g'])])
def test_a_call_on_the_wrong_stream_is_seen(M, name, buffers):
    """The same procedure with the default stream's handle in the call: it runs at once, on the decoy."""
    r = next(r for r in S.ROWS if r.name == name)
    _, got = S.run_delayed(r, M.ref[name], M.dev, M.cycles, M.side, call_stream=torch.cuda.default_stream().cuda_stream)
    assert S.differing(got, M.ref[name].want) == buffers


def _table(d, seed):
    return np.random.RandomState(seed).dirichlet(np.ones(d), size=S.NUM_START)


def _class_case(M, make, train, state):
    """make() -> a fresh instance over the true start table; train(obj) -> what it returns; state(obj) -> device tensors.
    Default stream first; then a second instance whose device table holds a decoy until a delayed producer on a side stream
    writes the true one, with train() and every read inside that stream."""
    np.random.seed(11)              # (the constructors draw the critic's start weights from np.random, as the reference does)
    a = make()
    ra = train(a)
    np.random.seed(11)
    want = [t.cpu() for t in state(a)]
    b = make()
    true = b._mat_pi0_dev.clone()
    b._mat_pi0_dev.copy_(torch.as_tensor(_table(b.d, 1), dtype=torch.float32))
    torch.cuda.synchronize()
    side = M.side
    with torch.cuda.stream(side):
        torch.cuda._sleep(M.cycles)
        b._mat_pi0_dev.copy_(true)
        rb = train(b)
        got = [t.cpu() for t in state(b)]
    torch.cuda.synchronize()
    for x, y in zip(want, got):
        assert S.same(x, y)
    return ra, rb


@pytest.mark.parametrize('update_every', ['step', 'rollout'])
def test_actor_critic_train_on_a_side_stream(M, update_every):
    from discrete_mean_field_game_amd.mfg_ac2 import actor_critic

    def make():
        return actor_critic(d=21, pi0=_table(21, 0), batch=13, seed=3, update_every=update_every, verbose=0, episode_steps=3)

    _class_case(M, make, lambda o: o.train(num_episodes=4), lambda o: (o._theta, o._w))


@pytest.mark.parametrize('update_every', ['step', 'rollout'])
def test_population_train_on_a_side_stream(M, update_every):
    from discrete_mean_field_game_amd.population import ActorCriticPopulation

    def make():
        return ActorCriticPopulation([8.0, 8.5, 9.0], d=21, batch=13, pi0=_table(21, 0), update_every=update_every,
                                     episode_steps=3)

    ra, rb = _class_case(M, make, lambda o: o.train(4), lambda o: (o._theta, o._w))
    assert np.array_equal(ra, rb) and ra.shape == (3, 4)
