"""CPU: the index arithmetic of tests/large_buffers.py and the case table of tests/test_gpu_large_buffers.py (no GPU, no library).

For every case of the table: the batch fills the slab past 2^31 + 2^24 floats and is ragged against the kernel's tile; the
boundary windows lie inside the batch, are pairwise disjoint and each contains the float offset it is named after; the chunks
tile the batch once in pieces below 2^28 floats that start on aligned items, of unequal sizes, with a chunk boundary on each
side of every window.  The table names every entry point and case the module is meant to cover."""
import pytest

import large_buffers as LB

torch = pytest.importorskip('torch')

_INITIALISED_BEFORE = torch.cuda.is_initialized()
import test_gpu_large_buffers as T
_INITIALISED_AFTER = torch.cuda.is_initialized()

CASES = T.CASES
IDS = [c['id'] for c in CASES]


def test_the_table_imports_without_touching_a_device():
    assert _INITIALISED_AFTER == _INITIALISED_BEFORE


def test_slab_size():
    assert LB.SLAB_FLOATS == 2 ** 31 + 2 ** 25 and LB.MARGIN_FLOATS == 2 ** 31 + 2 ** 24
    assert LB.BOUNDARIES == (2 ** 29, 2 ** 30, 2 ** 31)                 # 2 GiB, 4 GiB, 8 GiB of fp32


@pytest.mark.parametrize('c', CASES, ids=IDS)
def test_batch_fills_the_slab_and_is_ragged(c):
    B = LB.batch_for(c['per_item'], c['tile'])
    assert LB.MARGIN_FLOATS < B * c['per_item'] <= LB.SLAB_FLOATS
    assert c['tile'] == 1 or B % c['tile'] != 0
    assert (B + c['tile']) * c['per_item'] > LB.SLAB_FLOATS             # the largest such batch, up to the ragged tail
    total = T.case_batch(c)
    assert LB.MARGIN_FLOATS < total * c['per_item'] <= LB.SLAB_FLOATS
    if c['halves']:
        assert total % 2 == 0 and (total // 2) * c['per_item'] < 2 ** 31 < total * c['per_item']
    # many super tiles lie wholly past the last boundary (at d = 21 a super tile is 96 trajectories, 42 336 floats)
    assert total * c['per_item'] - 2 ** 31 > 100 * 42336


def test_batch_for_refuses_items_that_leave_no_batch():
    with pytest.raises(ValueError):
        LB.batch_for(2 ** 30)
    with pytest.raises(ValueError):
        LB.batch_for(0)
    assert LB.batch_for(441, 12) % 12 != 0 and LB.batch_for(441, 12) <= LB.batch_for(441)


@pytest.mark.parametrize('c', CASES, ids=IDS)
def test_boundary_windows(c):
    B, per, W = T.case_batch(c), c['per_item'], c['W']
    assert 5 * W * per >= LB.MIN_WINDOW_ELEMENTS or c['entry'] == 'mfg_traj_log_z_pop'    # (its row list is fixed: 5 x 8 rows)
    if c['entry'] == 'mfg_traj_log_z_pop':
        assert W == 8
    else:
        assert W == LB.window_items(per) and 5 * (W - 1) * per < LB.MIN_WINDOW_ELEMENTS
    wins = LB.boundary_windows(B, per, W)
    assert len(wins) == 5 and all(len(w) == W for w in wins)
    assert wins[0].start == 0 and wins[-1].stop == B
    for a, b in zip(wins[:-1], wins[1:]):
        assert 0 <= a.start < a.stop <= b.start < b.stop <= B          # in range, increasing, pairwise disjoint
    for w, off in zip(wins[1:4], LB.BOUNDARIES):
        item = off // per
        assert item in w and item * per <= off < (item + 1) * per      # the item that CONTAINS the offset is inside its window
        assert w.start * per <= off < w.stop * per
    idx = LB.window_index(wins)
    assert idx.shape == (5 * W,) and len(set(idx.tolist())) == 5 * W


def test_boundary_windows_refuse_a_batch_they_do_not_fit():
    with pytest.raises(ValueError):
        LB.boundary_windows(2 ** 29 // 441 + 3, 441, 8)                  # the batch ends before the 4 GiB window
    with pytest.raises(ValueError):
        LB.boundary_windows(17, 2 ** 27, 5)                              # windows of five items round items 4, 8, 16 overlap


def _chunk_floats(c):
    """Floats per item a case's chunks are cut for: an fp64 output counts twice."""
    return 2 * c['per_item'] if c['entry'] in ('mfg_alpha', 'mfg_features') else c['per_item']


@pytest.mark.parametrize('c', CASES, ids=IDS)
def test_chunks(c):
    B = T.case_batch(c)
    if c['halves']:
        B //= 2                                                         # (chunks run per group)
    per = _chunk_floats(c)
    cks = LB.chunks(B, per, align=4)
    assert cks[0][0] == 0 and cks[-1][1] == B
    for (lo, hi), (lo2, _) in zip(cks, cks[1:] + [(B, B)]):
        assert lo < hi == lo2                                           # consecutive: [0, B) exactly once
        assert (hi - lo) * per < LB.CHUNK_FLOATS
        assert lo % 4 == 0 and (lo * per * 4) % 16 == 0
    sizes = [hi - lo for lo, hi in cks[:-1]]
    assert len(cks) >= (5 if c['halves'] else 9) and len(set(sizes)) >= 4   # > 2^31 floats in chunks below 2^28; unequal sizes
    assert (cks[-1][1] - cks[-1][0]) * per <= LB.TAIL_FLOATS + 4 * per
    # a chunk boundary on each side of every window: an INNER one, but for the batch's two ends
    inner = [hi for _, hi in cks[:-1]]
    wins = LB.boundary_windows(B, c['per_item'], c['W']) if not c['halves'] else []
    for k, w in enumerate(wins):
        assert k == 0 or any(b <= w.start for b in inner), (k, w)
        assert k == len(wins) - 1 or any(b >= w.stop for b in inner), (k, w)


def test_chunks_of_a_small_batch():
    assert LB.chunks(5, 441) == [(0, 5)]
    with pytest.raises(ValueError):
        LB.chunks(10, 2 ** 28)


# what the module is meant to cover: entry point -> the (d, variant) cases
EXPECTED = {
    'mfg_step_given_P': {'step-d21', 'step-d15', 'step-d40', 'step-d100', 'step-d128', 'step-d256', 'step-d21-unaligned'},
    'mfg_score+mfg_td_pg_accumulate': {'score-d21-f64', 'score-d21-mixed', 'score-d128-mixed'},
    'mfg_policy_logpdf': {'logpdf-d21-K2'},
    'mfg_consistency_given': {'consistency-d21-T15'},
    'mfg_sample_dirichlet': {'sample-d21-mixed', 'sample-d21-f64', 'sample-d128-mixed'},
    'mfg_rollout': {'rollout-d21-T15', 'rollout-d128-T3'},
    'mfg_reward_net_forward': {'reward-net-d21', 'reward-net-d21-dropout'},
    'mfg_traj_log_z_pop': {'logz-d21-K1-shared', 'logz-d21-K2-per-learner'},
    'mfg_agents_step_pop': {'agents-d21-K2'},
    'mfg_alpha': {'alpha-d21'},
    'mfg_dirichlet_from_gamma': {'dirichlet-from-gamma-d21'},
    'mfg_features': {'features-d21'},
}
GROUPS = {'A': {'mfg_step_given_P', 'mfg_score+mfg_td_pg_accumulate', 'mfg_policy_logpdf', 'mfg_consistency_given'},
          'B': {'mfg_sample_dirichlet', 'mfg_rollout'},
          'C': {'mfg_reward_net_forward', 'mfg_traj_log_z_pop', 'mfg_agents_step_pop'},
          'D': {'mfg_alpha', 'mfg_dirichlet_from_gamma', 'mfg_features'}}


def test_the_table_is_complete():
    assert len(set(IDS)) == len(IDS)
    got = {}
    for c in CASES:
        got.setdefault(c['entry'], set()).add(c['id'])
        assert c['entry'] in GROUPS[c['group']], c['id']
    assert got == EXPECTED
    by_id = {c['id']: c for c in CASES}
    assert by_id['step-d21-unaligned']['offset'] == 1                   # the P view starts one float into the slab
    assert by_id['features-d21']['per_item'] == 253                     # phi [B, 253] fp64 with B 253 > 2^31
    assert [by_id[i]['T'] for i in ('consistency-d21-T15', 'rollout-d21-T15', 'rollout-d128-T3')] == [15, 15, 3]
    assert by_id['logz-d21-K2-per-learner']['halves'] and by_id['agents-d21-K2']['halves']


def test_every_case_has_a_test_and_every_entry_point_is_in_the_header():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, 'include', 'mfg_hip.h')) as f:
        header = f.read()
    with open(os.path.join(root, 'tests', 'test_gpu_large_buffers.py')) as f:
        module = f.read()
    for entry in EXPECTED:
        assert "_by('%s')" % entry in module, entry                      # a parametrised test takes the entry point's cases
        for name in entry.split('+'):
            assert re.search(r'\bint %s\(' % name, header), name
            assert "_call('%s'" % name in module, name                   # ... and calls the C ABI itself
