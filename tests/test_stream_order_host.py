"""CPU: the call table of tests/stream_order.py covers include/mfg_hip.h.  Every function of the header with an mfg_stream_t
parameter has a row, or stands on NEEDS_COMM; the DRAINS entries have rows and the header's own comment says that they drain the
stream.  A new entry point without a row fails here."""
import os
import re

import pytest

pytest.importorskip('torch')

import stream_order as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, 'include', 'mfg_hip.h')).read()


def stream_functions(text):
    """Names of the declared functions whose parameter list has an mfg_stream_t (comments removed first)."""
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    return sorted(name for name, params in re.findall(r'\b(mfg_[a-zA-Z0-9_]+)\s*\(([^;{}]*?)\)\s*;', text, flags=re.S)
                  if re.search(r'\bmfg_stream_t\b', params))


def uncovered(functions, rows):
    covered = {e for r in rows for e in r.entries}
    return sorted(set(functions) - covered - set(S.NEEDS_COMM))


def test_the_header_is_read():
    fns = stream_functions(_header())
    assert len(fns) >= 50, fns                                  # (50 when this test was written)
    assert 'mfg_step_given_P' in fns and 'mfg_init' not in fns and 'mfg_workspace_bytes' not in fns


def test_every_stream_entry_point_has_a_row_or_is_listed():
    fns = stream_functions(_header())
    assert uncovered(fns, S.ROWS) == []
    covered = {e for r in S.ROWS for e in r.entries}
    assert covered <= set(fns), sorted(covered - set(fns))               # (no row names a function the header does not have)
    assert not covered & set(S.NEEDS_COMM)
    assert set(S.NEEDS_COMM) <= set(fns) and set(S.DRAINS) <= covered


def test_the_lists_are_exactly_the_documented_ones():
    assert sorted(S.NEEDS_COMM) == ['mfg_dist_all_reduce', 'mfg_train_rollouts_dist']
    assert sorted(S.DRAINS) == ['mfg_reward_net_forward_pop', 'mfg_reward_net_train_steps_pop', 'mfg_reward_net_train_steps_pop_z',
                                'mfg_traj_log_z_pop']


def test_a_missing_row_and_a_new_entry_point_are_seen():
    fns = stream_functions(_header())
    assert uncovered(fns, [r for r in S.ROWS if 'mfg_jsd' not in r.entries]) == ['mfg_jsd']
    more = _header().replace('#ifdef __cplusplus\n}', 'int mfg_new_thing(const float* x, int64_t n,\n    mfg_stream_t stream);\n'
                             '#ifdef __cplusplus\n}')
    assert uncovered(stream_functions(more), S.ROWS) == ['mfg_new_thing']


def test_the_required_rows_are_there():
    """The shapes and paths the table must hold whatever else it holds."""
    names = {r.name for r in S.ROWS}
    for want in ('step_given_P-d21-B13', 'step_given_P-d128-B6', 'sample_dirichlet-d21-B13-mixed', 'sample_dirichlet-d21-B13-f64',
                 'sample_dirichlet-d130-B3-mixed', 'rollout-td-G-d21-B13-T3', 'rollout-td-G-d128-B6-T2', 'rollout-td-G-d100-B5-T2',
                 'rollout-external+grad_accumulate-d21', 'train_rollout-apply-idx', 'train_rollout-apply-drawn',
                 'train_rollout_deferred-x2-d21', 'train_rollout_deferred-x2-d128', 'train_episode-d21-T3', 'train_episode-d47-T2',
                 'train_episodes_pop-control', 'reward_net_forward-mfma', 'reward_net_forward-runs', 'forecast_pop-R3',
                 'forecast_score-R65-energy', 'forecast_agents_pop-H4'):
        assert want in names, want
    for base in ('td_pg_accumulate', 'grad_accumulate', 'grad_apply'):
        assert len([n for n in names if n.startswith(base + '-d')]) == 4, base
    assert len(names) == len(S.ROWS)


def _comment_before(text, name):
    """The comment block that precedes the declaration of `name` (the nearest one above it)."""
    at = re.search(r'^int\s+%s\s*\(' % re.escape(name), text, flags=re.M).start()
    blocks = [m for m in re.finditer(r'/\*.*?\*/', text[:at], flags=re.S)]
    return re.sub(r'\s*\n\s*\*\s*', ' ', blocks[-1].group(0))            # (one line: a phrase may wrap)


@pytest.mark.parametrize('name', S.DRAINS)
def test_the_header_says_that_a_drainer_drains(name):
    text = _header()
    # (the _z form refers to the call it extends: its comment names it, and that call's comment says it)
    doc = _comment_before(text, name)
    if 'drained' not in doc and name.endswith('_z'):
        base = name[:-2]
        assert base in doc
        doc = _comment_before(text, base)
    assert re.search(r'the stream is drained once before the (first )?launch', doc), name
