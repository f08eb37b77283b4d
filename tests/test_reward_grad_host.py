"""CPU checks of the reward input gradients: the reference of tests/reward_grad_ref.py against torch.autograd and central
differences, the admission of every GPU case (tests/test_gpu_reward_grad.py), the prototypes of reward_heatmap against a
literal restatement, and the argument checks of ops.reward_input_grad_pop.  No GPU."""
import numpy as np
import pytest

torch = pytest.importorskip('torch')

from oracle import reward_net_oracle as RO  # noqa: E402
import reward_grad_ref as G  # noqa: E402


def _masks(d, N, n3, n4, seed):
    return RO.dropout_masks(0.4, 1000 + seed, 5, N, n3, n4)


@pytest.mark.parametrize('d', [15, 21])
@pytest.mark.parametrize('drop', [False, True])
def test_reference_equals_autograd(d, drop):
    N, n3, n4 = 6, 8, 4
    net = G.make_net(d, 'none', n3, n4, 40 + d).double()
    state, action = G.make_inputs(d, N, d)
    masks = _masks(d, N, n3, n4, d) if drop else None
    ref = G.input_grad(RO.params_from_torch(net), state, action, masks)
    s = torch.tensor(state, dtype=torch.float64, requires_grad=True)
    a = torch.tensor(action, dtype=torch.float64, requires_grad=True)
    x = torch.relu(net.conv1(a.reshape(N, 1, d, d)))
    x = torch.relu(net.conv2(x)).permute(0, 2, 3, 1).reshape(N, -1)
    x = torch.relu(net.fc3(x))
    if drop:
        x = x * torch.tensor(masks[0])
    x = torch.relu(net.fc4(torch.cat([x, s], 1)))
    if drop:
        x = x * torch.tensor(masks[1])
    r = torch.tanh(net.out(x))
    if not drop:
        assert float((r - net(s, a)).detach().abs().max()) <= 1e-14     # the restated graph IS networks.RewardNet.forward
    gs, ga = torch.autograd.grad(r.sum(), (s, a))
    assert np.abs(r.detach().numpy()[:, 0] - ref['r']).max() <= 1e-14
    assert np.abs(gs.numpy() - ref['grad_state']).max() <= 1e-14
    assert np.abs(ga.numpy() - ref['grad_action']).max() <= 1e-14


@pytest.mark.parametrize('d', [15, 21])
@pytest.mark.parametrize('drop', [False, True])
def test_reference_equals_central_differences(d, drop):
    N, n3, n4, h = 3, 8, 4, 1e-6
    net = G.make_net(d, 'none', n3, n4, 60 + d)
    prm = RO.params_from_torch(net)
    state, action = (x.astype(np.float64) for x in G.make_inputs(d, N, 2 * d))
    masks = _masks(d, N, n3, n4, d) if drop else None
    ref = G.input_grad(prm, state, action, masks)
    assert ref['kink'] > 1e-4                                  # (no ReLU within reach of the step)
    fwd = lambda s, a: RO.forward_cache(prm, s, a, masks)[0][:, 0]
    worst = 0.0
    rs = np.random.RandomState(d)
    for j in range(d):
        e = np.zeros((N, d)); e[:, j] = h
        worst = max(worst, np.abs((fwd(state + e, action) - fwd(state - e, action)) / (2 * h) - ref['grad_state'][:, j]).max())
    for i, j in zip(rs.randint(0, d, 40), rs.randint(0, d, 40)):
        e = np.zeros((N, d, d)); e[:, i, j] = h
        worst = max(worst, np.abs((fwd(state, action + e) - fwd(state, action - e)) / (2 * h) - ref['grad_action'][:, i, j]).max())
    assert worst <= 1e-9, worst


@pytest.mark.parametrize('name', sorted(G.CASES))
def test_gpu_case_is_admitted(name):
    """Every learner of every GPU case: no ReLU on a kink, at least half the samples live (a kernel that wrote zeros must
    not pass), and a plain fp32 evaluation of the chain rule within HALF the GPU tolerance."""
    K = len(G.CASES[name][2])
    for k in range(K):
        ref, prm, st, ac, masks = G.case_reference(name, k)
        assert ref['kink'] >= G.KINK_MIN, (k, ref['kink'])
        assert ref['live'] >= G.LIVE_MIN, (k, ref['live'])
        assert np.abs(ref['grad_state']).max() > 0
        gs, ga = G.f32_input_grad(prm, st, ac, masks)
        rs_, ra_ = G.ratios(gs, ga, ref)
        print('%s learner %d: kink %.2e live %.2f fp32 ratios state %.4f action %.4f' % (name, k, ref['kink'], ref['live'], rs_, ra_))
        assert rs_ <= 0.5 and ra_ <= 0.5, (k, rs_, ra_)


def test_heatmap_prototypes_against_a_literal_restatement():
    from discrete_mean_field_game_amd import reward_dist
    for d in (15, 21):
        rs = np.random.RandomState(d)
        table = rs.dirichlet(np.ones(d), size=4)
        states = reward_dist.heatmap_states(table, d)
        assert states.dtype == np.float32 and states.shape == (3, d)
        assert np.array_equal(states[0], table[0].astype(np.float32))
        s2 = np.array([2.0 ** (d - i) for i in range(d)], dtype=np.float32)     # topic i has weight 2^(d-i)
        s2 = s2 / np.sum(s2, dtype=np.float32)
        assert np.array_equal(states[1], s2)
        assert np.array_equal(states[2], np.full(d, 1.0 / d, dtype=np.float32))
        a1 = rs.dirichlet(np.ones(d), size=(2, d)).astype(np.float32)
        acts = reward_dist.heatmap_actions(a1)
        assert acts.shape == (2, 3, d, d) and acts.dtype == np.float32
        for k in range(2):
            assert np.array_equal(acts[k, 0], a1[k])
            assert np.array_equal(acts[k, 1], np.full((d, d), 1.0 / d, dtype=np.float32))
            for i in range(d):
                for j in range(d):
                    assert acts[k, 2, i, j] == a1[k, i, d - 1 - j]


def test_argument_checks():
    from discrete_mean_field_game_amd import ops
    chk = ops.check_reward_input_grad_args
    want = ('mean_state', 'mean_action')
    assert chk(3, (5, 15), (5, 15, 15), [2, 0], 2, want) == (True, 5, 15)
    assert chk(3, (3, 5, 21), (3, 5, 21, 21), [1], 1, ops.RN_INPUT_GRAD_OUTPUTS) == (False, 5, 21)
    for args in ((0, (5, 15), (5, 15, 15), [], 0, want),                   # K
                 (3, (5, 15), (5, 15, 14), [0], 1, want),                  # action shape
                 (3, (2, 5, 15), (2, 5, 15, 15), [0], 1, want),            # leading K
                 (3, (5, 16), (5, 16, 16), [0], 1, want),                  # d
                 (3, (0, 15), (0, 15, 15), [0], 1, want),                  # N
                 (3, (5, 15), (5, 15, 15), [3], 1, want),                  # learner id
                 (3, (5, 15), (5, 15, 15), [1, 1], 2, want),               # twice
                 (3, (5, 15), (5, 15, 15), [1, 2], 1, want),               # keys
                 (3, (5, 15), (5, 15, 15), [1], 1, ()),                    # nothing wanted
                 (3, (5, 15), (5, 15, 15), [1], 1, ('reward',))):          # unknown output
        with pytest.raises(ValueError):
            chk(*args)


def test_block_checks_when_set():
    """mfg_ctx_set_rn_input_grad refuses without a context, and the workspace size is what the layout says (no GPU needed)."""
    import ctypes as C
    from discrete_mean_field_game_amd import _lib as L
    h = L.lib()
    blk = L.RnInputGradStruct(0, 0, 8, 0, 8, 64, 5, 3, 15, 0)
    assert h.mfg_ctx_set_rn_input_grad(None, C.byref(blk)) == -1
    assert h.mfg_ctx_set_rn_input_grad(None, None) == -1
    K, N, d = 3, 300, 15
    E = d + d * d
    chunks = 10                                                # ceil(300 / 32)
    assert h.mfg_rn_input_grad_workspace_bytes(K, N, d) == K * N * E * 4 + K * chunks * 2 * E * 8
    assert h.mfg_rn_input_grad_workspace_bytes(K, 33, d) == (K * 33 * E * 4 + 7) // 8 * 8 + K * 2 * 2 * E * 8
    assert h.mfg_rn_input_grad_workspace_bytes(0, N, d) == 0
    assert C.sizeof(L.RnInputGradStruct) == 72
