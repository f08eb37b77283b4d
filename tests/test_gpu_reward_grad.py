"""Reward input gradients on the GPU (mfg_rn_input_grad_t riding on mfg_reward_net_forward_pop) against the fp64 reference of
tests/reward_grad_ref.py, case by case (admitted on the CPU in tests/test_reward_grad_host.py).

Per sample: |got - ref| <= 1e-5 max(|ref|_max, scale_max).  Worst ratio |got - ref| / bound per case, measured on an MI355X
(state / action; the plain fp32 NumPy evaluation of the same chain rule sits at 0.002-0.07 / 0.0005-0.009):
  d15-n1 0.009 / 0.002   d21-n2 0.009 / 0.006    d15-n17 0.014 / 0.0006   d21-n31 0.008 / 0.001   d15-n32 0.012 / 0.002
  d21-n33 0.024 / 0.004  d21-n300 0.026 / 0.004  d15-mixed 0.045 / 0.007  d21-mixed 0.025 / 0.003  d15-drop 0.053 / 0.006
(every ratio is below 0.2: no operation of the kernel needs naming).
Means: against the fp64 mean of the returned fp32 samples (and of their exact products with the inputs) within
N 2^-52 max|term|; bit-equal with and without the per-sample arrays, and for learner k at K = 1 and K = 3.
"""
import ctypes as C
import functools

import numpy as np
import pytest

torch = pytest.importorskip('torch')

import reward_grad_ref as G  # noqa: E402

pytestmark = pytest.mark.gpu
EINVAL, EWORKSPACE = -1, -4
STRIDE_PAD = 37          # floats of NaN behind every learner's inputs in the per-learner cases


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.fail('-m gpu tests need a GPU')
    return torch.device('cuda:0')


@functools.lru_cache(maxsize=None)
def _reference(name, k):
    return G.case_reference(name, k)[0]


class Setup:
    """A case on the device: the flat parameter rows, the struct, the geometry table, the (strided) inputs."""

    def __init__(self, name, dev, learners=None):
        from discrete_mean_field_game_amd import _lib as L, ops
        from discrete_mean_field_game_amd.irl_population import NET_TENSORS, net_row_offsets
        d, N, nets, state, action, shared, mixed = G.build_case(name)
        ids = list(range(len(nets))) if learners is None else list(learners)      # K = 1: one learner of the case on its own
        nets = [nets[k] for k in ids]
        K = len(nets)
        self.name, self.d, self.N, self.K, self.ids, self.shared, self.nets = name, d, N, K, ids, shared, nets
        rows = [net_row_offsets(d, n.fc3.out_features, n.fc4.out_features) for n in nets]
        self.stride = (max(r[10] for r in rows) + 63) // 64 * 64
        self.flat = torch.full((K, self.stride), float('nan'), device=dev)
        for k, n in enumerate(nets):
            for i, (_, pname) in enumerate(NET_TENSORS):
                self.flat[k, rows[k][i]:rows[k][i + 1]] = n.get_parameter(pname).detach().reshape(-1).to(dev)
        st = L.RewardNetStruct()
        st.k1, st.f2, st.k2 = 5, 2, 3
        self.geom = None
        if mixed:
            _, geoms = ops.irl_pop_net_geometries(nets)
            self.geom = ops.rn_geom_table(geoms, dev)
            st.n3, st.n4, st.keep_prob = max(g[0] for g in geoms), max(g[1] for g in geoms), 1.0
            for f, _ in NET_TENSORS:
                setattr(st, f, self.flat.data_ptr())
        else:
            st.n3, st.n4, st.keep_prob = nets[0].fc3.out_features, nets[0].fc4.out_features, G.keep_of(nets[0])
            for i, (f, _) in enumerate(NET_TENSORS):
                setattr(st, f, self.flat.data_ptr() + 4 * rows[0][i])
        self.struct = st
        if shared:
            self.state, self.action = torch.from_numpy(state).to(dev), torch.from_numpy(action).to(dev)
        else:       # strides larger than needed, NaN in the gaps
            sb = torch.full((K, N * d + STRIDE_PAD), float('nan'), device=dev)
            ab = torch.full((K, N * d * d + STRIDE_PAD), float('nan'), device=dev)
            self.state, self.action = sb[:, :N * d].view(K, N, d), ab[:, :N * d * d].view(K, N, d, d)
            self.state.copy_(torch.from_numpy(state[ids]))
            self.action.copy_(torch.from_numpy(action[ids]))
        self.inputs_np = (state, action) if shared else (state[ids], action[ids])

    def listed(self):
        """(positions in this population, keys): learner 1 of a K = 3 case is left out."""
        pos = [p for p, k in enumerate(self.ids) if k in G.LISTED] if self.K > 1 else [0]
        pos = sorted(pos, reverse=True)
        return pos, [G.KEYS[self.ids[p]] for p in pos]

    def run(self, want_samples=True, **kw):
        from discrete_mean_field_game_amd import ops
        pos, keys = self.listed()
        return ops.reward_input_grad_pop(self.struct, True, self.K, self.state, self.action, pos, keys, net_stride=self.stride,
                                         geom=self.geom, want_samples=want_samples, **kw)

    def forward(self):
        from discrete_mean_field_game_amd import ops
        pos, keys = self.listed()
        st, ac = self.state, self.action
        if not self.shared:
            st, ac = st.contiguous(), ac.contiguous()
        out = torch.full((self.K, self.N), float('nan'), device=st.device)
        return ops.reward_net_forward_pop(self.struct, True, self.K, st, ac, pos, keys, out=out, net_stride=self.stride,
                                          geom=self.geom)

    def inputs_of(self, p):
        s, a = self.inputs_np
        return (s, a) if self.shared else (s[p], a[p])


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int64)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _check_means(res, su, p, N):
    """mean_*[p] against the fp64 mean of the returned fp32 samples and of their exact products with the inputs."""
    s, a = su.inputs_of(p)
    for name, grad, x in (('mean_state', res['grad_state'][p], s), ('mean_action', res['grad_action'][p], a)):
        g = grad.cpu().numpy().astype(np.float64)
        got = res[name][p].cpu().numpy()
        for q, terms in enumerate((g, g * x.astype(np.float64))):
            bound = N * 2.0 ** -52 * np.abs(terms).max()
            assert np.abs(got[q] - terms.mean(0)).max() <= bound, (name, q)


@pytest.mark.parametrize('name', sorted(G.CASES))
def test_case_against_the_reference(dev, name):
    su = Setup(name, dev)
    N, K = su.N, su.K
    res = su.run()
    torch.cuda.synchronize()
    pos, _ = su.listed()
    worst = [0.0, 0.0]
    for p in pos:
        ref = _reference(name, su.ids[p])
        rs, ra = G.ratios(res['grad_state'][p].cpu().numpy(), res['grad_action'][p].cpu().numpy(), ref)
        worst = [max(worst[0], rs), max(worst[1], ra)]
        live = float(np.mean(np.abs(res['grad_action'][p].cpu().numpy()).reshape(N, -1).max(1) > 0))
        assert live == ref['live'], (p, live, ref['live'])
        _check_means(res, su, p, N)
    print('%s: worst ratio state %.4f action %.4f' % (name, worst[0], worst[1]))
    assert worst[0] <= 1.0 and worst[1] <= 1.0, worst
    # the learner left out keeps the sentinel in all four outputs and in the rewards
    for p in range(K):
        if p not in pos:
            for n in ('grad_state', 'grad_action', 'mean_state', 'mean_action'):
                assert bool(torch.isnan(res[n][p]).all()), n
    # the rewards are those of the call without a block, bit for bit
    assert _same(res['reward'][pos], su.forward()[pos])
    # the means do not depend on whether the per-sample arrays are written, nor on which outputs are asked for
    lean = su.run(want_samples=False)
    only = su.run(want=('mean_action',))
    for n in ('mean_state', 'mean_action'):
        assert _same(lean[n][pos], res[n][pos]), n
    assert _same(only['mean_action'][pos], res['mean_action'][pos])
    assert set(lean) == {'reward', 'mean_state', 'mean_action'} and set(only) == {'reward', 'mean_action'}


@pytest.mark.parametrize('name', ['d15-n17', 'd21-n300', 'd15-mixed', 'd15-drop'])
def test_learner_is_the_same_bits_at_K_1_and_K_3(dev, name):
    full = Setup(name, dev).run()
    for k in G.LISTED:
        one = Setup(name, dev, learners=[k]).run()
        for n in ('reward', 'grad_state', 'grad_action', 'mean_state', 'mean_action'):
            assert _same(one[n][0], full[n][k]), (k, n)


def test_unbound_call_leaves_the_outputs_alone(dev):
    from discrete_mean_field_game_amd import ops
    su = Setup('d15-n17', dev)
    ctx = ops.Context(dev)
    res = su.run(ctx=ctx)
    torch.cuda.synchronize()
    keep = {n: res[n].clone() for n in ops.RN_INPUT_GRAD_OUTPUTS}
    for n in ops.RN_INPUT_GRAD_OUTPUTS:
        res[n].fill_(5.0)
    prev = ctx.bind_scoped()            # the same context, its block unbound by the call above
    try:
        su.forward()
    finally:
        ops.Context.restore(prev)
    torch.cuda.synchronize()
    for n in ops.RN_INPUT_GRAD_OUTPUTS:
        assert bool((res[n] == 5.0).all()), n
        assert bool(torch.isfinite(keep[n][0]).all()), n
    ctx.close()


def test_refusals_write_nothing(dev):
    """A K / N / d mismatch (MFG_EINVAL) and a short workspace (MFG_EWORKSPACE) are refused before anything is written."""
    from discrete_mean_field_game_amd import _lib as L, ops
    su = Setup('d15-n17', dev)
    K, N, d = su.K, su.N, su.d
    pos, keys = su.listed()
    need = ops.rn_input_grad_workspace_bytes(K, N, d)
    outs = {n: torch.full(ops._rn_input_grad_shape(n, K, N, d), 3.0, device=dev,
                          dtype=torch.float32 if n.startswith('grad') else torch.float64) for n in ops.RN_INPUT_GRAD_OUTPUTS}
    reward = torch.full((K, N), 3.0, device=dev)
    ws = torch.full((need // 8,), 3.0, dtype=torch.float64, device=dev)
    scratch = torch.zeros(2 * K, dtype=torch.float64, device=dev)
    lr = np.asarray(pos, dtype=np.int32)
    ky = np.asarray(keys, dtype=np.uint64)
    h = L.lib()
    ctx = ops.Context(dev)
    prev = ctx.bind_scoped()
    try:
        for (bK, bN, bd, bytes_), code in (((K + 1, N, d, need), EINVAL), ((K, N + 1, d, need), EINVAL), ((K, N, 21, need), EINVAL),
                                           ((K, N, d, need - 1), EWORKSPACE), ((K, N, d, 0), EWORKSPACE)):
            blk = L.RnInputGradStruct(outs['grad_state'].data_ptr(), outs['grad_action'].data_ptr(), outs['mean_state'].data_ptr(),
                                      outs['mean_action'].data_ptr(), ws.data_ptr(), bytes_, bN, bK, bd, 0)
            assert h.mfg_ctx_set_rn_input_grad(ctx._ptr, C.byref(blk)) == 0
            rc = h.mfg_reward_net_forward_pop(su.state.data_ptr(), su.action.data_ptr(), su.state.stride(0), su.action.stride(0), N,
                                              d, C.byref(su.struct), 1, su.stride, None, None, K, lr.ctypes.data, ky.ctypes.data,
                                              len(pos), 0, reward.data_ptr(), scratch.data_ptr(), 16 * K,
                                              torch.cuda.current_stream().cuda_stream)
            assert rc == code, (bK, bN, bd, bytes_, rc)
            torch.cuda.synchronize()
            for t in list(outs.values()) + [reward, ws]:
                assert bool((t == 3.0).all())
        # refused when it is set: all four outputs NULL, K or N out of range
        for blk in (L.RnInputGradStruct(None, None, None, None, ws.data_ptr(), need, N, K, d, 0),
                    L.RnInputGradStruct(outs['grad_state'].data_ptr(), None, None, None, ws.data_ptr(), need, N, 0, d, 0),
                    L.RnInputGradStruct(outs['grad_state'].data_ptr(), None, None, None, ws.data_ptr(), need, N, L.POP_MAX_K + 1, d, 0),
                    L.RnInputGradStruct(outs['grad_state'].data_ptr(), None, None, None, ws.data_ptr(), need, 0, K, d, 0)):
            assert h.mfg_ctx_set_rn_input_grad(ctx._ptr, C.byref(blk)) == EINVAL
    finally:
        h.mfg_ctx_set_rn_input_grad(ctx._ptr, None)
        ops.Context.restore(prev)
        ctx.close()
