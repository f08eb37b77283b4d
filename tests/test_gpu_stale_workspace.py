"""-m gpu: no result depends on what scratch memory holds.

include/mfg_hip.h: a workspace from mfg_workspace_bytes is zeroed ONCE, only its control block (64 bytes; one per slice in the
population forms) has to be zero, every call leaves it zero again, and "one workspace sized for the largest N serves calls with
any smaller N"; the other workspaces' "contents are scratch".  The rest of the suite hands every call a zeroed workspace, where a
reducer that reads one partial row more than was written, a first step that reads the previous step's rows or a slice rebased
by the wrong stride all add 0.0.  Here (tests/stale_workspace.py, on the call table of tests/stream_order.py):

  P  every row that owns a work buffer, with every byte outside the ranges the header requires to be zero set to 0xFF, 0x7F and
     0xFE (why three: tests/test_stale_workspace_host.py), in guard bands, run twice in the same buffers.
  R  per family a BIG shape, then a small one in the same buffers with its own workspace_bytes, nothing re-zeroed, then the
     big one again (and once small -> big): the stale word is a plausible partial row of the right magnitude.
After every call: (a) all outputs and in/out buffers bit for bit those of the call on a fresh zeroed workspace, (b) every
declared range zero again, (c) the guard bands of the work buffers untouched.

Row counts of an R pair are restated here from the launch rules (grad_geometry, core_sums_rows, irl_step_ws, the reward
network's grid) and asserted: the big call writes strictly more partial rows than the small one reads.
"""
import pytest

torch = pytest.importorskip('torch')

import stale_workspace as W
import stream_order as S

pytestmark = pytest.mark.gpu

WORK_ROWS = [r for r in S.ROWS if r.work]


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.fail('-m gpu tests need a GPU: the HIP path has no CPU fallback')
    S._ops().init()
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def ref(dev):
    """name -> the row's outputs on a fresh, fully zeroed workspace (stream_order.reference), computed once, read only."""
    cache = {}

    def get(r):
        if r.name not in cache:
            cache[r.name] = S.reference(r, dev).want
        return cache[r.name]
    return get


def test_no_row_with_a_work_buffer_is_left_out():
    assert len(WORK_ROWS) == W.N_WORK_ROWS == 47        # (tests/test_stale_workspace_host.py derives the count from the header)
    assert all(r in WORK_ROWS for r in S.ROWS if r.drains)


# ---------------------------------------------------------------------------------------------------- P
@pytest.mark.parametrize('fill', W.FILLS, ids=lambda f: '0x%02X' % f)
@pytest.mark.parametrize('r', WORK_ROWS, ids=[r.name for r in WORK_ROWS])
def test_poisoned_scratch(dev, ref, r, fill):
    found = W.poisoned(r, ref(r), dev, fill)
    assert not found, '%s: %s' % (r.name, found)


# ---------------------------------------------------------------------------------------------------- R: the launch rules
WAVES, GS_CH = 4, 64


def _ceil(a, b):
    return -(-a // b)


FUSE_MAX_ROWS = 32        # MFG_GRAD_FUSE_MAX_ROWS: up to this many rows the last block of k_grad_mfma_small reduces them itself


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _FO(d):
    return d * (d + 1) // 2 + d + 1 + 3


def nsb_of(N, d):
    """grad_geometry: super blocks of `chunk` samples, capped by the 72 MB of rows (at most 1 024, at least 16)."""
    chunk = min(max(8192 // d, 8), 64)
    return max(min(_ceil(N, chunk), min(max((72 << 20) // (_FO(d) * 8), 16), 1024)), 1)


def grad_rows(N, d):
    """Partial rows launch_grad writes and its reducer reads for N samples.  d <= 28, k_grad_mfma_small: a row per block of four
    64-sample chunks, two blocks per CU at most.  d = 128 / 256, k_grad_mfma2: nsb capped by `want` = 3 (d = 128) / 1 (d = 256)
    blocks per CU.  Otherwise nsb."""
    nsb = nsb_of(N, d)
    if d <= 28:
        return max(min(_ceil(_ceil(N, GS_CH), WAVES), 2 * _cus(), nsb), 1)
    if d in (128, 256):
        return min(nsb, _cus() * 3 if d == 128 else _cus())
    return nsb


def sums_rows(B, d):
    """core_sums_rows: a row per tile of k_core_small<.., SUMS> (T = 1, d = 21 / 15)."""
    return _ceil(B, WAVES * (64 // d))


def irl_rows(B):
    """irl_step_ws: a row per 16-sample block of k_reward_net_mfma<.., SUMS>."""
    return min(_ceil(B, 16), 256)


def runs_rows(B):
    """A row per eight-sample block of k_reward_net_runs<.., SUMS> (the three-launch env step)."""
    return _ceil(B, 8)


def restated_workspace_bytes(N, d):
    """mfg_workspace_bytes from the functions above: control block + max(nsb, SUMS rows, reward-network rows) rows + the value
    buffer of k_value_mfma* (d > 64, d % 16 == 0)."""
    rows = nsb_of(N, d)
    if d in (21, 15) and sums_rows(N, d) <= 512:
        rows = max(rows, sums_rows(N, d))
    if d <= 32:
        rows = max(rows, min(runs_rows(N), 512))
    return S.CONTROL_BYTES + rows * _FO(d) * 8 + (16 * N if d > 64 and d % 16 == 0 else 0)


WS_SHAPES = [(1200, 21), (13, 21), (1200, 15), (13, 15), (300, 128), (12, 128), (300, 80), (12, 80), (300, 100), (10, 100), (700, 21),
             (65, 21), (37, 128), (50000, 128), (8300, 21), (200, 21), (39, 21), (800, 21), (26, 21), (100, 21)]


@pytest.mark.parametrize('N,d', WS_SHAPES)
def test_the_restated_launch_rules_are_the_library_s(N, d):
    """The row counts in this file's docstrings come from Python restatements of the host arithmetic.  What the library itself
    reports of that arithmetic is mfg_workspace_bytes: for every (samples, d) of an R pair it must equal the restatement --
    nsb of grad_geometry at d > 32, the rows of k_core_small<.., SUMS> and of the reward-network launch below.  (Host only.)"""
    assert S.wsb(N, d) == restated_workspace_bytes(N, d)


def _rows_of(make, *args, **kw):
    with S.extra_rows() as out:
        make(*args, **kw)
    assert len(out) == 1
    return out[0]


def _pair(dev, ref, big, small, small_first=False):
    if small_first:
        found = W.leftovers_small_first(big, small, ref(big), ref(small), dev)
    else:
        found = W.leftovers([big, small, big], [ref(big), ref(small), ref(big)], dev)
    assert not found, found


# ---------------------------------------------------------------------------------------------------- R: mfg_rollout TD + G
ROLLOUT = {21: ((400, 3), (13, 1)), 15: ((400, 3), (13, 1)), 128: ((150, 2), (6, 2)), 80: ((150, 2), (6, 2)), 100: ((150, 2), (5, 2))}


@pytest.mark.parametrize('small_first', [False, True], ids=['big-small-big', 'small-big'])
@pytest.mark.parametrize('d', sorted(ROLLOUT))
def test_rollout_after_a_larger_rollout(dev, ref, d, small_first):
    """d = 21, 15: B = 400, T = 3 leaves 5 rows of k_grad_mfma_small (1 200 samples, 19 chunks); B = 13, T = 1 reads the 2 (d = 21)
    / 1 (d = 15) rows of k_core_small<.., SUMS>.  d = 128 (k_grad_mfma2 + k_value_mfma2 + k_td_delta), d = 80 (k_grad_mfma +
    k_value_mfma), d = 100 (k_grad_partial, values in the kernel): 300 samples, 5 rows, against 12 / 10 samples, 1 row; at
    d = 128 and 80 the value buffer of the small call (64 + 1 row) lies inside the big call's rows."""
    (Bb, Tb), (Bs, Ts) = ROLLOUT[d]
    written = grad_rows(Bb * Tb, d)
    read = sums_rows(Bs, d) if Ts == 1 else grad_rows(Bs * Ts, d)
    assert (written, read) == {21: (5, 2), 15: (5, 1), 128: (5, 1), 80: (5, 1), 100: (5, 1)}[d]
    _pair(dev, ref, _rows_of(S._rollout_td, d, Bb, Tb), _rows_of(S._rollout_td, d, Bs, Ts), small_first)


# ---------------------------------------------------------------------------------------------------- R: the batch sums
SUMS = [(S._td_pg_accumulate, 0), (S._grad_accumulate, 0), (S._grad_accumulate, 1), (S._grad_apply, 0)]


@pytest.mark.parametrize('d', [21, 128])
@pytest.mark.parametrize('make,flag', SUMS, ids=['td_pg_accumulate', 'grad_accumulate', 'grad_accumulate-acc-add_reward', 'grad_apply'])
def test_batch_sums_after_larger_ones(dev, ref, make, flag, d):
    """d = 21: 700 samples, 3 rows, then the table's 65 samples, 1 row.  d = 128: 300 samples, 5 rows, then 37 samples, 1 row."""
    Nb, Ns = (700, 65) if d == 21 else (300, 37)
    assert (grad_rows(Nb, d), grad_rows(Ns, d)) == ((3, 1) if d == 21 else (5, 1))
    _pair(dev, ref, _rows_of(make, d, flag, Nb), _rows_of(make, d, flag, Ns))


@pytest.mark.parametrize('make,flag,d', [(S._grad_accumulate, 0, 128), (S._grad_apply, 0, 128), (S._td_pg_accumulate, 0, 21),
                                         (S._grad_accumulate, 1, 21), (S._grad_apply, 1, 21)],
                         ids=['grad_accumulate-d128', 'grad_apply-d128', 'td_pg_accumulate-d21', 'grad_accumulate-acc-d21',
                              'grad_apply-add_reward-d21'])
def test_batch_sums_after_ones_past_the_caps(dev, ref, make, flag, d):
    """The two writer / reader pairs that only a large batch reaches.
    d = 128, 50 000 samples: grad_geometry gives nsb = 782 super blocks, k_grad_mfma2 runs on `want` = 3 per CU (768 on 256 CUs)
    and k_reduce_partials must read that many rows, not 782; then 37 samples, 1 row.  (mfg_td_pg_accumulate is left to d = 21:
    its P [N, d, d] would be 3.3 GB here.)
    d = 21, 8 300 samples: 130 chunks, 33 blocks of k_grad_mfma_small -- one more than the last block reduces itself, so the rows
    go through k_reduce_partials; then 65 samples, 1 row, the fused form."""
    Nb, Ns = (50000, 37) if d == 128 else (8300, 65)
    if d == 128:
        assert nsb_of(Nb, d) == 782 and grad_rows(Nb, d) == min(782, 3 * _cus()) and grad_rows(Ns, d) == 1
        assert grad_rows(Nb, d) < 782, 'this device has %d CUs: the cap of k_grad_mfma2 is not reached' % _cus()
    else:
        assert grad_rows(Nb, d) == 33 > FUSE_MAX_ROWS >= grad_rows(700, d) and grad_rows(Ns, d) == 1
    _pair(dev, ref, _rows_of(make, d, flag, Nb), _rows_of(make, d, flag, Ns))


# ---------------------------------------------------------------------------------------------------- R: the training loops, d = 21
def test_train_episode_after_a_larger_one(dev, ref):
    """B = 200: 17 rows of k_core_small<.., SUMS> per step; B = 13: 2."""
    assert (sums_rows(200, 21), sums_rows(13, 21)) == (17, 2)
    _pair(dev, ref, _rows_of(S._train_episode, 21, 200, 3), _rows_of(S._train_episode, 21, 13, 3))


def test_train_episodes_after_larger_ones(dev, ref):
    """As above, three episodes each."""
    _pair(dev, ref, _rows_of(S._train_episodes, 200, 3), _rows_of(S._train_episodes, 13, 3))


@pytest.mark.parametrize('make', [S._train_rollouts, lambda B, T: S._train_rollout_deferred(21, B, T)], ids=['train_rollouts', 'deferred'])
def test_train_rollouts_after_larger_ones(dev, ref, make):
    """B = 400, T = 3: 5 rows of k_grad_mfma_small; B = 13, T = 3: 1."""
    assert (grad_rows(1200, 21), grad_rows(39, 21)) == (5, 1)
    _pair(dev, ref, _rows_of(make, 400, 3), _rows_of(make, 13, 3))


# ---------------------------------------------------------------------------------------------------- R: the IRL drivers, d = 21
@pytest.mark.parametrize('draw', [False, True], ids=['given', 'draw'])
@pytest.mark.parametrize('n3', [8, 24], ids=['mfma-two-launch', 'runs-three-launch'])
def test_irl_episode_after_a_larger_one(dev, ref, draw, n3):
    """Two env steps each.  n3 = 8, the two-launch flow: B = 200 leaves 13 rows (and the column in front of them) of
    k_reward_net_mfma<.., SUMS> per step, B = 13 reads 1; its first step kernel must not read the rows the big episode left.
    n3 = 24, three launches: k_reward_net_runs<.., SUMS> leaves 25 rows (RnSums::room = 25), B = 13 reads 2 (room 2)."""
    if n3 == 8:
        assert (irl_rows(200), irl_rows(13)) == (13, 1)
    else:
        assert (runs_rows(200), runs_rows(13)) == (25, 2)
    _pair(dev, ref, _rows_of(S._irl_episode, draw, 200, 2, n3), _rows_of(S._irl_episode, draw, 13, 2, n3))


def test_irl_rollout_after_a_larger_one(dev, ref):
    """B = 400, T = 2: 4 rows of the batch sums over 800 samples; B = 13, T = 2: 1."""
    assert (grad_rows(800, 21), grad_rows(26, 21)) == (4, 1)
    _pair(dev, ref, _rows_of(S._irl_rollout, 400, 2), _rows_of(S._irl_rollout, 13, 2))


# ---------------------------------------------------------------------------------------------------- R: populations, K = 3
BIG_POP = dict(S.POP, B=100)


@pytest.mark.parametrize('case', ['episodes_pop', 'episodes_pop-control', 'episodes_pop_resident', 'rollouts_pop', 'episodes_irl_pop',
                                  'rollouts_irl_pop'])
def test_population_after_a_larger_one(dev, ref, case):
    """K = 3, T = 2.  The C ABI has ONE B for all learners, so the slices of a call are equally long; what makes a learner meet a
    neighbour's rows is the other call's slice length: B = 100 has slices of pop_workspace_slice(100), B = 13 of
    pop_workspace_slice(13), so learners 1 and 2 of the small call work inside the rows learner 0 (and 1) of the big call left,
    and back.  (The two control blocks of the small call that lay in those rows are the caller's to zero; nothing else is.)
    Rows per learner and update: step mode 9 against 2 (k_core_small<.., SUMS>; the resident form the same tiles), IRL step mode
    7 against 1, rollout mode 1 against 1 of k_grad_mfma_small (200 / 26 samples) -- there the stale rows are the neighbour's.
    -control: learner 1 retires after its first episode."""
    assert (sums_rows(100, 21), sums_rows(13, 21), irl_rows(100), irl_rows(13)) == (9, 2, 7, 1)
    ops = S._ops()
    assert ops.pop_workspace_slice(100, 21, 2) > ops.pop_workspace_slice(13, 21, 2)

    def make(shape):
        if case.startswith('episodes_pop'):
            return _rows_of(S._pop_step, 'mfg_train_' + case.replace('-control', ''), case.endswith('-control'), shape)
        if case == 'rollouts_pop':
            return _rows_of(S._pop_rollouts, shape)
        return _rows_of(S._irl_pop, case == 'episodes_irl_pop', shape)
    _pair(dev, ref, make(BIG_POP), make(S.POP))


# ---------------------------------------------------------------------------------------------------- R: validation + evolve
def test_validated_population_after_a_larger_one(dev, ref):
    """mfg_train_episodes_pop under a validation block with scores and an evolve block, TWO checks in one call (the table's
    row).  Big: B = 100 and checks of 6 held-out files (18 members per learner); small: B = 13 and 2 files (6 members).  The small
    call's validation workspace is the head of the big one's: every section of its layout (start-row tables, per-member metrics,
    members, metrics, scores) starts at another offset, inside what the big call's second check left, and its own second check
    runs over what its first one left.  Metrics, curve, ranks and the rates the evolve steps wrote must be those of the fresh
    call."""
    ops = S._ops()
    assert ops.pop_validate_workspace_bytes(6, S.VAL['L'], 21, 3, S.VAL['R'], True) > ops.pop_validate_workspace_bytes(
        2, S.VAL['L'], 21, 3, S.VAL['R'], True)
    big, small = _rows_of(S._pop_validated, BIG_POP, 6), _rows_of(S._pop_validated, S.POP)
    want = ref(small)
    assert (want['val_checks'] == 2).all() and torch.isfinite(want['val_curve']).all() and (want['evo_rank'] >= 0).all()
    _pair(dev, ref, big, small)
