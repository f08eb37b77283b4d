"""-m gpu: every population entry point at K = 257 and K = MFG_POP_MAX_K = 65535 (tests/large_populations.py).

Procedure C: a population of K learners cycled over P = 7 parameter sets gives, in every output and in/out buffer, slice k equal
bit for bit to slice k mod P of the call with K = P -- the header's own promise ("the same bits whatever K is") is the oracle for
all 65 535 learners at once.  Outputs start as NaN / negative, outputs and workspaces have guard bands at exactly the
advertised size, and the P sets are asserted to give pairwise different results.
Procedure E: mfg_train_episodes_pop under a control, a validation and an evolve block at K = 255, 256, 257, 513 and 65535:
ranks, order, donors, rates and every learner's arrays against tests/pop_evolve_ref.py on the device's own check values.
The Python layer at the seam of POP_MAX_K: gridsearch, forecast, var.fit_population and rnn.fit_population over POP_MAX_K + 3.

EVERY row's small (K = 7) call is held once against the reference, under the assertions of the operation's own test module
(imported, not restated), or bit for bit against the single-learner entry point, which that module holds against the oracle:
  reference     evaluate_pop, forecast_pop, forecast_score, agents_step_pop, forecast_agents_pop (taken apart: sample_dirichlet,
                tests/agents_ref.py and the reductions), action_mean_pop, the consistency pair, row_distribution, policy_logpdf,
                traj_log_z_pop, rn_input_grad (tests/reward_grad_ref.py), var_fit_pop, rnn_fit_pop, and the check rows of
                procedure E (tests/test_gpu_pop_validate.py's _check_rows: ops.evaluate_pop on the thetas of the check, which
                tests/test_gpu_evaluate_pop.py holds against NumPy)
  single call   mfg_train_episodes_pop (mfg_train_episodes), mfg_train_rollouts_pop (mfg_train_rollouts), the resident form
                (the plain population call), the four IRL driver rows (mfg_train_episode_irl_draw / mfg_train_rollout_irl through
                tests/test_gpu_irl_population.py's _single), mfg_reward_net_forward_pop (mfg_reward_net_forward),
                mfg_reward_net_train_steps_pop / _z (mfg_reward_net_train_step / _z)
Every row's small call also equals 7 calls with K = 1.  The single-call comparisons read their arguments from the rows' own
builders (LP.built).
No time is asserted; docs/HISTORY.md has the record.
"""
import os
import time

import numpy as np
import pytest

torch = pytest.importorskip('torch')

import large_populations as LP
import stream_order as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.fail('-m gpu tests need a GPU: the HIP path has no CPU fallback')
    from discrete_mean_field_game_amd import ops
    ops.init()
    return torch.device('cuda:0')


def _max_k():
    from discrete_mean_field_game_amd import _lib
    return _lib.POP_MAX_K


def _report(what, t0):
    torch.cuda.synchronize()
    print('%-44s %7.2f s  peak %6.2f GiB' % (what, time.perf_counter() - t0, torch.cuda.max_memory_allocated() / 2.0 ** 30))


# --------------------------------------------------- procedure C
@pytest.mark.parametrize('big', [False, True], ids=['K257', 'Kmax'])
@pytest.mark.parametrize('r', LP.ROWS, ids=lambda r: r.name)
def test_a_cycled_population_repeats_its_sets_bit_for_bit(dev, r, big):
    K = _max_k() if big else 257
    LP.small(r, dev)
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    a = LP.cycled(r, dev, K)
    _report('%s K=%d' % (r.name, K), t0)
    assert not any(LP.unwritten(t) for t in a.compared().values())
    del a
    torch.cuda.empty_cache()


def test_the_comparison_sees_one_wrong_learner_on_the_device(dev):
    """The helper on device tensors of the largest K (its CPU form is tested in tests/test_large_populations_host.py)."""
    K = _max_k()
    small = torch.arange(LP.P * 3, dtype=torch.float64, device=dev).view(LP.P, 3)
    small[2, 1] = float('nan')
    big = small[torch.arange(K, device=dev) % LP.P].contiguous()
    assert LP.differing_learners(big, small) == []
    big[K - 1, 2] += 1.0
    big[K // 2, 0] = -0.0 if float(big[K // 2, 0]) == 0.0 else -float(big[K // 2, 0])
    assert LP.differing_learners(big, small) == [K // 2, K - 1]
    with pytest.raises(AssertionError, match='learner %d ' % (K // 2)):
        LP.assert_cycled('x', big, small)


@pytest.mark.parametrize('r', LP.ROWS, ids=lambda r: r.name)
def test_a_set_alone_gives_the_bits_it_gives_among_others(dev, r):
    """The small call against P calls with K = 1 (for mfg_traj_log_z_pop the header calls that the single-learner form)."""
    assert LP.alone(r, dev) == []


# --------------------------------------------------- the small call against the single-learner call
def _single_pop_step(dev, r, d, s, small):
    """Set s through mfg_train_episodes: the names of the buffers that differ from slice s of the small population call.  Every
    argument is read from the row's own builder."""
    L, ops = S._L(), S._ops()
    a = LP.built(r, dev)
    F = ops.num_features(d)
    i = a.inputs
    th, w = a.cmp['theta'][0][s:s + 1].clone(), a.cmp['w'][0][s].clone()
    B, T, E = LP.B, LP.T, LP.E
    pi = torch.full((B, d), S.NAN, device=dev)
    scratch = torch.zeros(B, d, device=dev)
    r_, delta, g = torch.full((B,), S.NAN, device=dev), torch.full((B,), S.NAN, dtype=S.F64, device=dev), torch.full((B,), S.NAN, dtype=S.F64, device=dev)
    G, acc = torch.full((F + 3,), S.NAN, dtype=S.F64, device=dev), a.cmp['reward_acc'][0][s].clone()
    n = ops.pop_workspace_slice(B, d, T)             # ("the same traj_offset and workspace_bytes")
    ws = torch.zeros(n, dtype=S.U8, device=dev)
    S.call('mfg_train_episodes', S.p(i['mat_pi0']), int(i['mat_pi0'].shape[0]), S.p(pi), S.p(scratch), B, d, T, E, 0, 0, S.p(th),
           float(i['shifts'][s]), float(i['alphas'][s]), S.p(w), S.GAMMA, L.REWARD_MFG_AC2, int(i['seeds'][s]), 3, 100,
           L.PRECISION_MIXED, float(i['lr_critic'][s]), float(i['lr_actor'][s]), S.p(r_), S.p(delta), S.p(g), S.p(G), S.p(acc),
           S.p(ws), n)
    torch.cuda.synchronize()
    got = dict(theta=th[0], w=w, G=G, reward_acc=acc, pi_io=pi, reward=r_, delta=delta, g=g)
    return [n_ for n_, t in got.items() if not S.same(t, small[n_][s])]


@pytest.mark.parametrize('d', [21, 5])
def test_the_small_training_call_equals_single_learner_calls(dev, d):
    """"Learner k of a population call gives, bit for bit in every output, what the single-learner call gives": the K = P call
    of the step-mode row against P calls of mfg_train_episodes."""
    r = next(r for r in LP.ROWS if r.name == 'train_episodes_pop-d%d' % d)
    small = LP.small(r, dev)
    for s in range(LP.P):
        assert _single_pop_step(dev, r, d, s, small) == [], 'set %d' % s


def test_the_small_resident_call_equals_the_plain_population_call(dev):
    a = LP.small(next(r for r in LP.ROWS if r.name == 'train_episodes_pop-d21'), dev)
    b = LP.small(next(r for r in LP.ROWS if r.name == 'train_episodes_pop_resident-d21'), dev)
    assert S.differing(b, a) == []


# --------------------------------------------------- the small call against the operation's own restatement
def _row(name):
    return next(r for r in LP.ROWS if r.name == name)


def test_the_small_agents_step_is_the_restatements(dev):
    import test_gpu_agents as TA                  # (its exact comparison against tests/agents_ref.py)
    r = _row('agents_step_pop')
    got, inp = LP.small(r, dev), LP.small_inputs(r, dev)
    seeds = inp['seeds'].cpu().numpy().view(np.uint64)
    TA._same_as_ref([got[n].cpu().numpy() for n in ('counts_next', 'pi_next', 'moves')], inp['counts'].cpu().numpy(),
                    inp['P'].cpu().numpy(), LP.AGENTS, seeds, 5, 1000)


def test_the_small_forecast_score_is_within_the_restatements_bounds(dev):
    import forecast_score_ref
    import test_gpu_forecast_score as TS          # (its bounds, derived from the restatement)
    r = _row('forecast_score')
    got, inp = LP.small(r, dev), LP.small_inputs(r, dev)
    want = forecast_score_ref.score(inp['traj'].cpu().numpy(), inp['emp32'].cpu().numpy(), inp['emp64'].cpu().numpy(), LP.N, LP.R)
    TS._check_against_ref({n: t.cpu().numpy() for n, t in got.items()}, want, LP.R, 'large-population small call')


def test_the_small_action_mean_is_numpys(dev):
    import test_gpu_action_mean as TM             # (its bound: N u)
    r = _row('action_mean_pop')
    got, inp = LP.small(r, dev), LP.small_inputs(r, dev)
    a = inp['action'].cpu().numpy()
    assert np.abs(got['mean'].cpu().numpy() - np.mean(a.astype(np.float64), axis=1)).max() <= a.shape[1] * TM.U


def _np(t):
    return t.cpu().numpy()


@pytest.mark.parametrize('d', [21, 5])
def test_the_small_evaluation_is_the_restatements(dev, d):
    import test_gpu_evaluate_pop as TE            # (_assert_metrics: the restatement on the call's own trajectories)
    from discrete_mean_field_game_amd import ops
    r = _row('evaluate_pop-d%d' % d)
    got, inp = LP.small(r, dev), LP.small_inputs(r, dev)
    th, sh, al = inp['policies']
    metrics, traj = ops.evaluate_pop(inp['emp32'], inp['emp64'], th.contiguous(), sh.contiguous(), al.contiguous(), inp['seeds'],
                                     first_step=37, repeats=LP.R, want_traj=True)
    assert S.same(metrics, got['metrics'])         # (with and without the trajectories: the same bits)
    for s in range(LP.P):
        TE._assert_metrics(_np(metrics[s]), _np(inp['emp64']), _np(traj[s]), 'set %d' % s)


def test_the_small_forecast_is_the_restatements(dev):
    import test_gpu_forecast_pop as TF            # (_check_moments, _check_quant, _assert_curves)
    from discrete_mean_field_game_amd import ops
    r = _row('forecast_pop')
    got, inp = LP.small(r, dev), LP.small_inputs(r, dev)
    assert LP.RANKS == TF._ranks(LP.R)
    th, sh, al = inp['policies']
    out = ops.forecast_pop(inp['start32'], th.contiguous(), sh.contiguous(), al.contiguous(), inp['seeds'], LP.H, first_step=37,
                           repeats=LP.R, ranks=LP.RANKS, emp32=inp['emp32'], emp64=inp['emp64'], want_traj=True)
    for n in ('mean', 'std', 'quant', 'curves'):
        assert S.same(out[n], got[n]), n
    f = {n: _np(got[n]) for n in ('mean', 'std', 'quant', 'curves')}
    f.update(traj=_np(out['traj']), emp=_np(inp['emp64']))
    TF._check_moments(f, LP.P, LP.N, LP.R)
    TF._check_quant(f, LP.P, LP.N, LP.R)
    for s in range(LP.P):
        TF._assert_curves(f['curves'][s], f['emp'], f['traj'][s], 'set %d' % s)


def test_the_small_consistency_calls_are_the_oracles(dev):
    import test_gpu_consistency_pop as TC         # (_check_steps: the oracle on the same actions; _check_metrics)
    from discrete_mean_field_game_amd import ops
    r = _row('consistency_given')
    got, inp = LP.small(r, dev), LP.small_inputs(r, dev)
    out = ops.consistency_given(inp['P'])
    assert S.same(out['metrics'], got['metrics'])
    TC._check_steps(_np(out['steps']), _np(out['V']), _np(inp['P']), 'large-population small call')
    TC._check_metrics(dict(steps=_np(out['steps']), metrics=_np(got['metrics'])), 'large-population small call')
    r = _row('consistency_pop')
    got, inp = LP.small(r, dev), LP.small_inputs(r, dev)
    th, sh, al = inp['policies']
    out = ops.consistency_pop(inp['start32'], th.contiguous(), sh.contiguous(), al.contiguous(), inp['seeds'], LP.H, first_step=37,
                              repeats=LP.R, want_steps=True, want_V=True, want_actions=True)
    assert S.same(out['metrics'], got['metrics']) and S.same(out['steps'], got['steps'])
    TC._check_steps(_np(got['steps']), _np(out['V']), _np(out['actions']), 'rolled small call')
    TC._check_metrics(dict(steps=_np(got['steps']), metrics=_np(got['metrics'])), 'rolled small call')


def test_the_small_row_distribution_is_numpys(dev):
    import test_gpu_reward_dist as TD             # (_check_hist, _check_moments)
    r = _row('row_distribution')
    got, inp = LP.small(r, dev), LP.small_inputs(r, dev)
    x = _np(inp['values'])[:, :257]
    g = {n: _np(t) for n, t in got.items()}
    TD._check_hist(g, x, 16)
    TD._check_moments(g, x)
    assert not g['status'].any() and np.isfinite(g['density']).all()


def test_the_small_var_fit_is_within_the_restatements_bounds(dev):
    import test_gpu_var_pop as TVAR               # (backward_error: the solve's bound)
    import rnn_ref
    got = LP.small(_row('var_fit_pop'), dev)
    days, V = rnn_ref.dirichlet_days(6, LP.BHD, LP.BD, 4001), LP.VAR_SETS
    assert not _np(got['status']).any()
    for s in range(LP.P):
        p = V['lag'][s]
        m = 1 + p * LP.BD
        coef = _np(got['coef'][s])
        eta, bound = TVAR.backward_error(days, V['train'][s], p, V['ridge'][s], coef[:m], 2 * LP.BHD - p)
        print('set %d: eta %.3e (bound %.3e)' % (s, eta, bound))
        assert eta <= bound and np.all(coef[m:] == 0)


def test_the_small_rnn_fit_is_within_the_restatements_bounds(dev):
    import rnn_ref as RR                          # (model: the restatement; bound: its own float64-against-longdouble gap)
    got = LP.small(_row('rnn_fit_pop'), dev)
    days, Rn = RR.dirichlet_days(6, LP.BHD, LP.BD, 4002), LP.RNN_SETS
    assert not _np(got['status']).any()
    for s in range(LP.P):
        w0 = RR.init_weights(Rn['hidden'][s], LP.BD, [77, s])
        a, b = (RR.model(days, Rn['train'][s], Rn['val'][s], Rn['test'][s], Rn['hidden'][s], w0, LP.RNN_EPOCHS, dtype=dt,
                         lr=Rn['lr'][s], wd=Rn['wd'][s], clip=Rn['clip'][s]) for dt in (np.float64, np.longdouble))
        assert int(got['best_epoch'][s]) == a['best_epoch'] == b['best_epoch']
        for what, have in (('weights', _np(got['weights'][s])[:w0.size]), ('loss', _np(got['loss'][s])), ('val', _np(got['val'][s]))):
            bound, err = RR.bound(a[what], b[what]), float(np.abs(have - a[what]).max())
            print('set %d %s: err %.3e bound %.3e' % (s, what, err, bound))
            assert err <= bound, (s, what)


def test_the_small_reward_forward_is_the_single_call(dev):
    """mfg_reward_net_forward_pop "bit for bit" mfg_reward_net_forward with learner k's weights and key, the call that
    tests/test_gpu_reward_net_forward_paths.py and test_gpu_parity.py hold against the oracle."""
    r = _row('reward_net_forward_pop')
    got, inp = LP.small(r, dev), LP.small_inputs(r, dev)
    names = ('conv1_w', 'conv1_b', 'conv2_w', 'conv2_b', 'fc3_w', 'fc3_b', 'fc4_w', 'fc4_b', 'out_w', 'out_b')
    for s in range(LP.P):
        out = torch.full((LP.RN_N,), S.NAN, device=dev)
        S.call('mfg_reward_net_forward', S.p(inp['state'][s]), S.p(inp['action'][s]), LP.RN_N, 21, 5, 2, 3, LP.N3, LP.N4,
               *[S.p(inp['net_' + n][s]) for n in names], 0.8, int(inp['keys'][s]), 0, S.p(out))
        torch.cuda.synchronize()
        assert S.same(out, got['reward'][s]), s


@pytest.mark.parametrize('z', [False, True], ids=['plain', 'z'])
def test_the_small_reward_training_steps_are_single_steps(dev, z):
    """"exactly mfg_reward_net_train_step(_z) ... the same bits": the two updates of every set through the single step, the call
    that tests/test_gpu_reward_train.py and test_gpu_importance_weights.py hold against the autograd oracle."""
    import ctypes as C
    entry = 'mfg_reward_net_train_step' + ('_z' if z else '')
    r = _row('reward_net_train_steps_pop' + ('_z' if z else ''))
    want = LP.small(r, dev)
    a = LP.built(r, dev)                           # (not issued: the start values of the in/out buffers, the inputs, the plan)
    RN, dims = LP.RN, LP._rn_dims()
    rows, T, nd, ng = RN['rows'], RN['T'], RN['nd'], RN['ng']
    n = int(S._L().lib().mfg_reward_net_train_workspace_bytes(*dims, (nd + ng) * T))
    for s in range(LP.P):
        prm, m, v = (a.cmp[k][0][s].clone() for k in ('params', 'adam_m', 'adam_v'))
        stats = torch.full((4,), S.NAN, device=dev)
        ws = torch.zeros((n + 3) // 4 * 4, dtype=S.U8, device=dev)
        for u in range(RN['U']):
            e = [e for e in a.plan[u * LP.P:(u + 1) * LP.P] if int(e['learner']) == s][0]      # the set's entry of update u
            dr, gr = (C.c_int32 * nd)(*e['demo_rows'][:nd].tolist()), (C.c_int32 * ng)(*e['gen_rows'][:ng].tolist())
            logz = (S.p(a.inputs['gen_log_z'][s]),) if z else ()
            S.call(entry, S.p(prm), S.p(m), S.p(v), *dims, S.p(a.inputs['demo_state']), S.p(a.inputs['demo_action']), dr, nd,
                   S.p(a.inputs['gen_state'][s]), S.p(a.inputs['gen_action'][s]), gr, ng, T, 5, 0.8, 1, int(e['key']),
                   float(e['lr']), 0.9, 0.999, 1e-8, int(e['adam_step']), 0, None, S.p(stats), S.p(ws), ws.numel(), *logz)
            torch.cuda.synchronize()
        NP = int(S._L().lib().mfg_reward_net_num_params(*dims))
        have = dict(params=prm, adam_m=m, adam_v=v, stats=stats)
        bad = [k for k, t in have.items() if not S.same(t[:NP] if k != 'stats' else t, want[k][s][:NP] if k != 'stats' else want[k][s])]
        assert bad == [], 'set %d' % s


def test_the_small_log_densities_are_the_oracles(dev):
    import test_gpu_launch_once_kernels as TL     # (_assert_logpdf: the oracle and its bound)
    import test_gpu_importance_weights as TW      # (_assert_log_z: calc_z and its bound)
    from oracle import mfg_oracle as O
    r = _row('policy_logpdf')
    got, inp = LP.small(r, dev), LP.small_inputs(r, dev)
    TL._assert_logpdf(_np(got['logpdf']).T, _np(inp['pi']), _np(inp['P']), _np(inp['thetas']), LP.LOGPDF, 'large-population', 'K=7')
    for name, per_learner in (('traj_log_z_pop-stores', True), ('traj_log_z_pop-shared_store', False)):
        r = _row(name)
        got, inp = LP.small(r, dev), LP.small_inputs(r, dev)
        for s in range(LP.P):
            st, ac = (inp[k][s] if per_learner else inp[k] for k in ('state', 'action'))
            want = O.calc_z(_np(st), _np(ac), _np(inp['thetas'][s]), float(inp['shifts'][s]), LP.LOGZ_STARTS, alpha_floor=0.0)
            TW._assert_log_z(_np(got['log_z'][s]), want)


@pytest.mark.parametrize('d', [21, 5])
def test_the_small_rollout_training_call_equals_single_learner_calls(dev, d):
    """mfg_train_rollouts_pop against P calls of mfg_train_rollouts."""
    L, ops = S._L(), S._ops()
    r = _row('train_rollouts_pop-d%d' % d)
    small = LP.small(r, dev)
    a = LP.built(r, dev)                           # (every argument is read from the row's own builder)
    i = a.inputs
    F = ops.num_features(d)
    B, T, E = LP.B, LP.T, LP.E
    n = ops.pop_workspace_slice(B, d, T)
    for s in range(LP.P):
        th, w, acc = a.cmp['theta'][0][s:s + 1].clone(), a.cmp['w'][0][s].clone(), a.cmp['reward_acc'][0][s].clone()
        nan = lambda shape, dt=S.F32: torch.full(shape, S.NAN, dtype=dt, device=dev)
        traj, last, rew, delta, g = nan((B, T + 1, d)), nan((B, d)), nan((B, T)), nan((B, T), S.F64), nan((B, T), S.F64)
        G, ws = nan((F + 3,), S.F64), torch.zeros(n, dtype=S.U8, device=dev)
        S.call('mfg_train_rollouts', S.p(i['mat_pi0']), int(i['mat_pi0'].shape[0]), B, d, T, E, 0, 0, S.p(th), float(i['shifts'][s]),
               float(i['alphas'][s]), S.p(w), S.GAMMA, L.REWARD_MFG_AC2, int(i['seeds'][s]), 3, 100, 0, float(i['lr_critic'][s]),
               float(i['lr_actor'][s]), S.p(traj), S.p(last), S.p(rew), S.p(delta), S.p(g), S.p(G), S.p(acc), S.p(ws), n)
        torch.cuda.synchronize()
        have = dict(theta=th[0], w=w, G=G, reward_acc=acc, pi_traj=traj, pi_last=last, reward=rew, delta=delta, g=g)
        assert [k for k, t in have.items() if not S.same(t, small[k][s])] == [], 'set %d' % s


@pytest.mark.parametrize('per_learner', [True, False], ids=['nets', 'shared_net'])
@pytest.mark.parametrize('mode', ['step', 'rollout'])
def test_the_small_irl_calls_equal_single_learner_calls(dev, mode, per_learner):
    """The four IRL driver rows against tests/test_gpu_irl_population.py's _single: mfg_train_episode_irl_draw per episode /
    mfg_train_rollout_irl per episode with learner k's settings and network, bit for bit in every output."""
    import copy
    import test_gpu_irl_population as TI
    step = mode == 'step'
    r = _row('train_%s_irl_pop-%s' % ('episodes' if step else 'rollouts', 'nets' if per_learner else 'shared_net'))
    small = LP.small(r, dev)
    a = LP.built(r, dev)
    i = a.inputs
    assert torch.equal(i['mat_pi0'].cpu(), torch.as_tensor(TI._table(21).astype(np.float32)))
    for s in range(LP.P):
        net = copy.deepcopy(LP.irl_nets()[s if per_learner else 0]).to(dev)
        ref = TI._single(mode, 21, LP.B, 'mixed', net, int(i['seeds'][s]), float(a.cmp['theta'][0][s]), float(i['shifts'][s]),
                         float(i['alphas'][s]), _np(a.cmp['w'][0][s]), LP.E, S.GAMMA, 0, float(i['lr_critic'][s]),
                         float(i['lr_actor'][s]), 0, dev, T=LP.T)
        torch.cuda.synchronize()
        got = dict(theta=small['theta'][s:s + 1], w=small['w'][s], G=small['G'][s], P=small['P'][s], reward=small['reward'][s],
                   delta=small['delta'][s], g=small['g'][s], pi=small['pi_out' if step else 'pi_last'][s],
                   acc=small['reward_acc'][s] if step else small['reward_acc'][s] * LP.T)
        if not step:
            got['pi_traj'] = small['pi_traj'][s]
        bad = [k for k, v in got.items() if not S.same(v, ref[k].view(v.shape))]
        assert bad == [], 'set %d' % s


def test_the_small_input_gradients_are_the_restatements(dev):
    import types
    import reward_grad_ref as G                   # (input_grad, ratios: the error over the restatement's own tolerance)
    import test_gpu_reward_grad as TG             # (_check_means)
    from oracle import reward_net_oracle as RO
    got = LP.small(_row('rn_input_grad'), dev)
    nets, state, action = LP.grad_case()
    su = types.SimpleNamespace(inputs_of=lambda q: (state[q], action[q]))
    for s in range(LP.P):
        masks = G.masks_of(G.keep_of(nets[s]), LP.grad_keys()[s], LP.RN_N, LP.N3, LP.N4)
        ref = G.input_grad(RO.params_from_torch(nets[s]), state[s], action[s], masks)
        ga = _np(got['grad_action'][s])
        rs, ra = G.ratios(_np(got['grad_state'][s]), ga, ref)
        print('set %d: ratio state %.4f action %.4f' % (s, rs, ra))
        assert rs <= 1.0 and ra <= 1.0, s
        assert float(np.mean(np.abs(ga).reshape(LP.RN_N, -1).max(1) > 0)) == ref['live'], s
        TG._check_means(got, su, s, LP.RN_N)


def test_the_small_agents_forecast_is_taken_apart(dev):
    import test_gpu_agents as TA                  # (_check_taken_apart: sample_dirichlet, tests/agents_ref.py, the reductions)
    from discrete_mean_field_game_amd import ops
    r = _row('forecast_agents_pop')
    got, inp = LP.small(r, dev), LP.small_inputs(r, dev)
    th, sh, al = (t.contiguous() for t in inp['policies'])
    out = ops.forecast_agents_pop(inp['counts0'], LP.AGENTS, th, sh, al, inp['seeds'], LP.H, first_step=37, repeats=LP.R,
                                  ranks=LP.RANKS, emp32=inp['emp32'], emp64=inp['emp64'], want_traj=True, want_counts=True,
                                  want_actions=True)
    for n, m in (('mean', 'mean'), ('std', 'std'), ('quant', 'quant'), ('curves', 'curves'), ('counts', 'counts_traj'),
                 ('actions', 'actions')):
        assert S.same(out[n], got[m]), n
    TA._check_taken_apart(dev, out, _np(inp['emp64']), _np(inp['counts0']), LP.AGENTS, tuple(_np(t) for t in (th, sh, al, inp['seeds'])),
                          LP.RANKS, LP.R, 'mixed')


# --------------------------------------------------- procedure E
@pytest.mark.parametrize('replace', [True, False], ids=['replaced', 'too_few_active'])
@pytest.mark.parametrize('K', LP.E_K + ('max',))
def test_control_validation_and_evolve_blocks(dev, K, replace):
    K = _max_k() if K == 'max' else K
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    out = LP.evolved(dev, K, replace)
    _report('evolve K=%d %s' % (K, 'replaced' if replace else 'logged only'), t0)
    if K >= 513:                                   # a whole rank tile without an active learner
        assert (out['rank'][256:512] == -1).all() and (out['parent'][256:512] == -1).all()
    active = LP.expected_active(K)
    rank = out['rank'][active]
    assert sorted(rank.tolist()) == list(range(int(active.sum())))
    # ties across a tile seam were decided by k: among the learners of one set the rank ascends with k
    for s in range(LP.P):
        ks = np.flatnonzero(active & (np.arange(K) % LP.P == s))
        if ks.size:
            assert (np.diff(out['rank'][ks]) == 1).all(), 'set %d' % s


# --------------------------------------------------- the Python layer at the seam
def test_gridsearch_splits_a_grid_past_the_largest_population(dev, tmp_path, monkeypatch):
    from discrete_mean_field_game_amd import ops, population
    Kmax, d, Lr = _max_k(), 5, 3
    assert population.GRID_CHUNK == Kmax
    emp = np.random.RandomState(11).dirichlet(np.ones(d), size=(2, Lr))
    os.makedirs(tmp_path / 'test_files')
    for i, m in enumerate(emp):
        np.savetxt(tmp_path / 'test_files' / ('day%d.txt' % i), m, delimiter=' ', fmt='%.17g')
    monkeypatch.chdir(tmp_path)
    n = Kmax + 3
    thetas = (6.0 + 3.0 * np.arange(n) / n).tolist()
    calls, real = [], ops.evaluate_pop
    monkeypatch.setattr(ops, 'evaluate_pop', lambda *a, **kw: calls.append(real(*a, **kw)) or calls[-1])
    t0 = time.perf_counter()
    population.gridsearch(thetas, [0.16], [12000.0], 'test_files', str(tmp_path / 'grid.csv'), d=d, seed=5, episode_length=Lr, repeats=2)
    monkeypatch.setattr(ops, 'evaluate_pop', real)
    _report('gridsearch %d points' % n, t0)
    assert [int(c.shape[0]) for c in calls] == [Kmax, 3]
    table = torch.cat(calls)
    with open(tmp_path / 'grid.csv') as f:
        assert sum(1 for _ in f) == n
    emp_read = population.load_empirical('test_files', d, Lr)
    pick = [0, Kmax - 1, Kmax, Kmax + 2]
    f64 = lambda v: torch.tensor(v, dtype=torch.float64, device=dev)
    direct = ops.evaluate_pop(torch.as_tensor(emp_read.astype(np.float32), device=dev), torch.as_tensor(emp_read, device=dev),
                              f64([thetas[i] for i in pick]), f64([0.16] * 4), f64([12000.0] * 4),
                              torch.full((4,), 5, dtype=torch.int64, device=dev), first_step=0, repeats=2)
    assert S.same(table[pick], direct)
    assert len({tuple(row) for row in direct.cpu().numpy().tolist()}) == 4


def test_forecast_splits_policies_past_the_largest_population(dev, monkeypatch):
    from discrete_mean_field_game_amd import ops, population
    Kmax, d, H = _max_k(), 5, 3
    assert population.FORECAST_CHUNK == Kmax
    n = Kmax + 3
    thetas = 6.0 + 3.0 * np.arange(n) / n
    emp = np.random.RandomState(12).dirichlet(np.ones(d), size=(2, H))
    calls, real = [], ops.forecast_pop
    monkeypatch.setattr(ops, 'forecast_pop', lambda *a, **kw: calls.append(int(a[1].shape[0])) or real(*a, **kw))
    t0 = time.perf_counter()
    fc = population.forecast(thetas, 0.16, 12000.0, None, H, d=d, seed=5, repeats=2, probs=(0.0, 1.0), emp=emp)
    monkeypatch.setattr(ops, 'forecast_pop', real)
    _report('forecast %d policies' % n, t0)
    assert calls == [Kmax, 3]
    pick = [0, Kmax - 1, Kmax, Kmax + 2]
    f64 = lambda v: torch.tensor(v, dtype=torch.float64, device=dev)
    direct = ops.forecast_pop(torch.as_tensor(emp[:, 0].astype(np.float32), device=dev), f64(thetas[pick]), f64([0.16] * 4),
                              f64([12000.0] * 4), torch.full((4,), 5, dtype=torch.int64, device=dev), H, first_step=0, repeats=2,
                              ranks=population.forecast_ranks((0.0, 1.0), 2), emp32=torch.as_tensor(emp.astype(np.float32), device=dev),
                              emp64=torch.as_tensor(emp, device=dev))
    for name, got in (('mean', fc.mean), ('std', fc.std), ('quant', fc.quantiles), ('curves', fc.curves)):
        assert got.shape[0] == n
        assert S.same(torch.as_tensor(got[pick]), direct[name].cpu()), name
    assert len({tuple(row.reshape(-1)) for row in fc.mean[pick]}) == 4


def _cycle(values, n):
    return [values[k % LP.P] for k in range(n)]


def _assert_cycled_numpy(name, got, want):
    LP.assert_cycled(name, torch.as_tensor(np.ascontiguousarray(got)), torch.as_tensor(np.ascontiguousarray(want)))


def test_var_fit_population_across_the_chunk_seam(dev, monkeypatch):
    import rnn_ref
    from discrete_mean_field_game_amd import ops, var
    n, V = _max_k() + 3, LP.VAR_SETS
    days = rnn_ref.dirichlet_days(6, LP.BHD, LP.BD, 4001)
    origin = ['rolling' if o else 'train_end' for o in V['origin']]
    want = var.fit_population(days, V['lag'], V['ridge'], V['train'], V['test'], origin, budget=1 << 40)
    calls, real = [], ops.var_fit_pop
    monkeypatch.setattr(ops, 'var_fit_pop', lambda *a, **kw: calls.append(len(a[1])) or real(*a, **kw))
    t0 = time.perf_counter()
    got = var.fit_population(days, _cycle(V['lag'], n), _cycle(V['ridge'], n), _cycle(V['train'], n), _cycle(V['test'], n),
                             _cycle(origin, n), budget=1 << 40)
    monkeypatch.setattr(ops, 'var_fit_pop', real)
    _report('var.fit_population %d models' % n, t0)
    assert calls == [_max_k(), 3]
    assert not want.status.any()
    for name in ('coef', 'sse', 'insample', 'future', 'per_day', 'metrics', 'status'):
        _assert_cycled_numpy(name, getattr(got, name), getattr(want, name))
    LP.assert_distinct('var', {n_: torch.as_tensor(getattr(want, n_)) for n_ in ('coef', 'metrics')})


def test_rnn_fit_population_across_the_chunk_seam(dev, monkeypatch):
    import rnn_ref
    from discrete_mean_field_game_amd import ops, rnn
    n, Rn = _max_k() + 3, LP.RNN_SETS
    days = rnn_ref.dirichlet_days(6, LP.BHD, LP.BD, 4002)
    w0 = [rnn_ref.init_weights(Hn, LP.BD, [77, s]) for s, Hn in enumerate(Rn['hidden'])]
    kw = dict(optimizer='adam', eval_every=1, budget=1 << 40)
    want = rnn.fit_population(days, Rn['hidden'], Rn['lr'], LP.RNN_EPOCHS, Rn['train'], Rn['val'], Rn['test'], wd=Rn['wd'], clip=Rn['clip'],
                              w0=w0, **kw)
    calls, real = [], ops.rnn_fit_pop
    monkeypatch.setattr(ops, 'rnn_fit_pop', lambda *a, **k: calls.append(len(a[2])) or real(*a, **k))
    t0 = time.perf_counter()
    got = rnn.fit_population(days, _cycle(Rn['hidden'], n), _cycle(Rn['lr'], n), LP.RNN_EPOCHS, _cycle(Rn['train'], n),
                             _cycle(Rn['val'], n), _cycle(Rn['test'], n), wd=_cycle(Rn['wd'], n), clip=_cycle(Rn['clip'], n),
                             w0=_cycle(w0, n), **kw)
    monkeypatch.setattr(ops, 'rnn_fit_pop', real)
    _report('rnn.fit_population %d models' % n, t0)
    assert calls == [_max_k(), 3]
    assert not want.status.any()
    for name in ('weights', 'loss', 'val', 'best_epoch', 'future', 'per_day', 'metrics', 'status'):
        _assert_cycled_numpy(name, getattr(got, name), getattr(want, name))
    LP.assert_distinct('rnn', {n_: torch.as_tensor(getattr(want, n_)) for n_ in ('weights', 'metrics')})
