"""CPU: the call table of tests/large_populations.py covers include/mfg_hip.h, its comparison sees a wrong learner, and the
inputs of procedure E can tell the header's tie-break from a tile-local one.  A new population entry point without a row fails
here."""
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip('torch')

import large_populations as LP
import pop_evolve_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, 'include', 'mfg_hip.h')).read()


def population_functions(text):
    """Names of the declared functions that take K learners: a parameter named K, or a pointer to a struct with a member K."""
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    structs = {name for body, name in re.findall(r'typedef\s+struct\s+\w+\s*\{([^{}]*)\}\s*(\w+)\s*;', text)
               if re.search(r'\bK\b', body)}
    out = []
    for name, params in re.findall(r'\b(mfg_[a-zA-Z0-9_]+)\s*\(([^;{}]*?)\)\s*;', text, flags=re.S):
        if re.search(r'\bK\b', params) or any(re.search(r'\b%s\b' % s, params) for s in structs):
            out.append(name)
    return sorted(out), sorted(structs)


def uncovered(functions, covered):
    return sorted(set(functions) - set(covered) - set(LP.EXEMPT))


def test_the_header_is_read():
    fns, structs = population_functions(_header())
    assert structs == ['mfg_pop_control_t', 'mfg_pop_evolve_t', 'mfg_pop_validate_t', 'mfg_rn_input_grad_t', 'mfg_rnn_fit_t',
                       'mfg_var_fit_t'], structs
    assert len(fns) >= 35, fns                                  # (35 when this test was written)
    for want in ('mfg_train_episodes_pop', 'mfg_ctx_set_pop_evolve', 'mfg_var_fit_pop', 'mfg_policy_logpdf',
                 'mfg_evaluate_pop_workspace_bytes'):
        assert want in fns, want
    assert 'mfg_train_episodes' not in fns and 'mfg_row_distribution' not in fns


def test_every_population_entry_point_has_a_row():
    fns, _ = population_functions(_header())
    covered = LP.covered_entries()
    assert uncovered(fns, covered) == []
    all_fns = set(re.findall(r'\b(mfg_[a-zA-Z0-9_]+)\s*\(', _header()))
    assert set(covered) <= all_fns, sorted(set(covered) - all_fns)       # (no row names a function the header does not have)
    assert LP.EXEMPT == {}                                                 # every entry needs a reason; none is needed
    assert 'mfg_row_distribution' in covered                               # R rows in the place of K learners


def test_a_missing_row_and_a_new_entry_point_are_seen():
    fns, _ = population_functions(_header())
    covered = [e for e in LP.covered_entries() if e != 'mfg_traj_log_z_pop']
    assert uncovered(fns, covered) == ['mfg_traj_log_z_pop']
    more = _header().replace('#ifdef __cplusplus\n}', 'int mfg_new_pop(const float* x, int K,\n    mfg_stream_t stream);\n'
                             'typedef struct mfg_new_block { float* x; int32_t d, K; } mfg_new_block_t;\n'
                             'int mfg_ctx_set_new_block(mfg_ctx_t* ctx, const mfg_new_block_t* block);\n#ifdef __cplusplus\n}')
    assert uncovered(population_functions(more)[0], LP.covered_entries()) == ['mfg_ctx_set_new_block', 'mfg_new_pop']


def test_the_required_rows_are_there():
    names = [r.name for r in LP.ROWS]
    assert len(set(names)) == len(names)
    for want in ('train_episodes_pop-d21', 'train_episodes_pop-d5', 'train_episodes_pop_resident-d21', 'train_rollouts_pop-d21',
                 'train_rollouts_pop-d5', 'evaluate_pop-d21', 'evaluate_pop-d5', 'train_episodes_irl_pop-nets',
                 'train_episodes_irl_pop-shared_net', 'train_rollouts_irl_pop-nets', 'rn_input_grad', 'row_distribution',
                 'var_fit_pop', 'rnn_fit_pop'):
        assert want in names, want
    assert LP.P == 7 and all(np.gcd(LP.P, n) == 1 for n in (64, 256))


# --------------------------------------------------- the comparison
def _cycled(K, shape=(3, 2), dtype=torch.float64):
    small = torch.arange(LP.P * int(np.prod(shape)), dtype=dtype).view((LP.P,) + shape) * 0.5
    if dtype.is_floating_point:
        small[1, 0, 0] = float('nan')
    return small, small[torch.arange(K) % LP.P].contiguous()


@pytest.mark.parametrize('K', [7, 8, 257, 700])
def test_a_cycled_result_passes(K):
    small, big = _cycled(K)
    LP.assert_cycled('x', big, small)                     # (NaN equals NaN of the same bits)
    small, big = _cycled(K, dtype=torch.int32)
    LP.assert_cycled('x', big, small)


@pytest.mark.parametrize('K,k', [(257, 0), (257, 100), (257, 251), (257, 252), (257, 256), (700, 699), (8, 7), (5, 4)])
def test_one_wrong_slice_fails_and_is_named(K, k):
    """In the whole cycles, in the remainder, and slice K - 1."""
    small, big = _cycled(K)
    big[k, 2, 1] += 1.0
    assert LP.differing_learners(big, small) == [k]
    with pytest.raises(AssertionError, match=r'learner %d \(set %d\)' % (k, k % LP.P)):
        LP.assert_cycled('x', big, small)


def test_a_bit_is_a_difference():
    small = torch.zeros(LP.P, 2, dtype=torch.float32)
    big = small[torch.arange(30) % LP.P].contiguous()
    big[29, 1] = -0.0
    assert LP.differing_learners(big, small) == [29]
    nan = torch.full((LP.P, 1), float('nan'))
    other = nan[torch.arange(30) % LP.P].contiguous()
    other.view(torch.int32)[13, 0] += 1                   # another NaN
    assert LP.differing_learners(other, nan) == [13]


def test_a_learner_that_took_its_neighbours_set_fails():
    small, big = _cycled(257)
    big[130] = small[(130 + 1) % LP.P]
    assert LP.differing_learners(big, small) == [130]


def test_coinciding_sets_fail():
    small, _ = _cycled(7)
    LP.assert_distinct('x', {'a': small, 'b': torch.zeros(LP.P, 2)})       # (one buffer that tells them apart is enough)
    small[5] = small[2]
    assert LP.coinciding_sets({'a': small, 'b': torch.zeros(LP.P, 2)}) == [(2, 5)]
    with pytest.raises(AssertionError, match='cannot see learners collapse'):
        LP.assert_distinct('x', {'a': small})


# --------------------------------------------------- the Python layer past the largest population
def _cycle(values, n):
    return [values[k % LP.P] for k in range(n)]


def test_fit_population_takes_more_models_than_one_call():
    """The argument rules of one call (at most POP_MAX_K models) are applied per chunk: POP_MAX_K + 3 models are accepted, a
    bad model behind the seam is still refused."""
    from discrete_mean_field_game_amd import _lib, ops, rnn, var
    from discrete_mean_field_game_amd.population import consistency_chunks
    n = _lib.POP_MAX_K + 3
    days = np.full((6, LP.BHD, LP.BD), 1.0 / LP.BD)
    V, Rn = LP.VAR_SETS, LP.RNN_SETS
    args = [_cycle(V[k], n) for k in ('lag', 'ridge', 'train', 'test')]
    shape = var.check_population_args(days, *args, 'rolling')[-1]
    assert shape == (n, 6, LP.BHD, LP.BD, 1 + 2 * LP.BD, LP.BHD)
    assert consistency_chunks(n, var.model_bytes(*shape[4:], 1, LP.BD), 1 << 40) == [(0, _lib.POP_MAX_K), (_lib.POP_MAX_K, 3)]
    args[0][n - 1] = 0
    with pytest.raises(ValueError, match='lag=0'):
        var.check_population_args(days, *args, 'rolling')
    with pytest.raises(ValueError, match='at most %d in one call' % _lib.POP_MAX_K):
        ops.check_var_fit_args(days.shape, [1] * n, [1.0] * n, [2] * n, [1] * n, [0] * n)
    hidden = _cycle(Rn['hidden'], n)
    out = rnn.check_population_args(days, hidden, _cycle(Rn['lr'], n), LP.RNN_EPOCHS, _cycle(Rn['train'], n), _cycle(Rn['val'], n),
                                    _cycle(Rn['test'], n), _cycle(Rn['wd'], n), _cycle(Rn['clip'], n), 'adam', 1)
    assert out[-1] == (n, 6, LP.BHD, LP.BD, ops.rnn_weight_count(8, LP.BD), LP.RNN_EPOCHS, LP.RNN_EPOCHS)
    ones = np.ones(n, dtype=np.int64)
    per = rnn.model_bytes(np.asarray(hidden), LP.RNN_EPOCHS * ones, 2 * ones, ones, ones, LP.BD, LP.BHD)
    assert per == rnn.model_bytes(np.asarray(hidden[:LP.P]), LP.RNN_EPOCHS * ones[:LP.P], 2 * ones[:LP.P], ones[:LP.P], ones[:LP.P],
                                  LP.BD, LP.BHD)


def test_the_input_gradient_sets_are_admitted():
    """The rule of tests/test_reward_grad_host.py for that module's own GPU cases, on the P sets of the rn_input_grad row: no
    ReLU on a kink, at least half the samples live, a plain fp32 evaluation within half the GPU tolerance."""
    import reward_grad_ref as G
    from oracle import reward_net_oracle as RO
    nets, state, action = LP.grad_case()
    assert state.shape == (LP.P, LP.RN_N, 21) and action.shape == (LP.P, LP.RN_N, 21, 21)
    for s in range(LP.P):
        prm = RO.params_from_torch(nets[s])
        masks = G.masks_of(G.keep_of(nets[s]), LP.grad_keys()[s], LP.RN_N, LP.N3, LP.N4)
        assert G.keep_of(nets[s]) == LP.GRAD_KEEP and masks is not None
        ref = G.input_grad(prm, state[s], action[s], masks)
        assert ref['kink'] >= G.KINK_MIN and ref['live'] >= G.LIVE_MIN and np.abs(ref['grad_state']).max() > 0, s
        rs_, ra_ = G.ratios(*G.f32_input_grad(prm, state[s], action[s], masks), ref)
        assert rs_ <= 0.5 and ra_ <= 0.5, (s, rs_, ra_)


# --------------------------------------------------- procedure E's inputs
def _values(K):
    """The check values of cycled sets: one value per set, the retired set's not finite."""
    v = np.array([0.31, 0.12, 0.25, np.nan, 0.07, 0.5, 0.19])
    return v[np.arange(K) % LP.P]


@pytest.mark.parametrize('K', LP.E_K + (65535,))
def test_the_counts_of_procedure_e(K):
    active = LP.expected_active(K)
    A = int(active.sum())
    n_top, n_bottom = LP.evolve_counts(K, True)
    assert 1 <= n_top and 1 <= n_bottom and n_top + n_bottom <= A
    n_top, n_bottom = LP.evolve_counts(K, False)
    assert A < n_top + n_bottom <= K and n_top >= 1 and n_bottom >= 1
    off = LP.caller_inactive(K)
    assert not active[off].any() and not active[np.arange(K) % LP.P == LP.RETIRED_SET].any()
    if K >= 513:
        assert off[256:512].all() and not active[256:512].any()


def test_the_cycled_inputs_tell_the_tie_break_by_k_from_a_tile_local_one():
    """At K = 513 the header's order (ties to the smaller k) differs from the order of a rank kernel that compared positions
    inside a 256-key tile."""
    K = 513
    values, active = _values(K), LP.expected_active(K)
    n_top, n_bottom = LP.evolve_counts(K, True)
    out = pop_evolve_ref.step(values, active, np.zeros(K), np.zeros((K, 1)), np.full(K, 0.1), np.full(K, 0.001), s=0, seed=LP.E_SEED,
                              n_top=n_top, n_bottom=n_bottom)
    assert out['replaced']
    wrong = LP.order_with_tile_local_ties(values, active)
    assert np.array_equal(wrong == -1, out['rank'] == -1)
    assert not np.array_equal(wrong, out['rank'])
    assert wrong[512] < out['rank'][512]                 # learner 512 sits at position 0 of its tile: ahead of its whole set
    # with all keys different the two agree everywhere: the ties are what differs
    distinct = np.random.RandomState(3).permutation(K).astype(np.float64)
    ref = pop_evolve_ref.step(distinct, active, np.zeros(K), np.zeros((K, 1)), np.full(K, 0.1), np.full(K, 0.001), s=0,
                              seed=LP.E_SEED, n_top=n_top, n_bottom=n_bottom)
    assert np.array_equal(LP.order_with_tile_local_ties(distinct, active), ref['rank'])
