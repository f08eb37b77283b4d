"""-m gpu: the batch-sum kernels of a parameter update (mfg_grad_accumulate) over the layouts their dispatch depends on --
trajectory strides (the 32-bit and the wide address form of k_grad_mfma_small), every tile layout of k_grad_mfma /
k_grad_mfma2 (d = 64, 80, ..., 512), the scalar staging fall-backs of a misaligned `pi` or stride, the chunk sizes of
k_grad_partial, and trajectories long enough for the fp32 index arithmetic to matter (oracle/grad_index_ref.py).

Every case lays its states out in a flat allocation of B + 1 strides addressed through torch.as_strided; everything the
layout skips holds a large FINITE sentinel (a masked lane may legally load a gap), so a read of a skipped float shows in the
sums.  Reference: G = [sum delta phi(x) | sum delta g | sum r | N] in fp64 over the addressed samples, together with the
magnitude sums sum |delta| |phi|.  Criteria, unless a family says otherwise, are those of
test_gpu_parity.py::test_grad_accumulate_all_kernels: quadratic block within 1e-12 max|ref|, the rest within
1e-11 max(1, max|ref|), exact count, `accumulate` adds onto G, `add_reward` returns delta + reward exactly.
"""
import numpy as np
import pytest

torch = pytest.importorskip('torch')

pytestmark = pytest.mark.gpu

SENTINEL = float(np.float32(1e30))
U = 2.0 ** -53


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.fail('-m gpu tests need a GPU: the HIP path has no CPU fallback')
    return torch.device('cuda:0')


def ops():
    from discrete_mean_field_game_amd import ops as _ops
    return _ops


def t32(x, dev):
    return torch.as_tensor(np.ascontiguousarray(x, dtype=np.float32), device=dev)


def t64(x, dev):
    return torch.as_tensor(np.ascontiguousarray(x, dtype=np.float64), device=dev)


def lay_out(x, stride_b, offset=0):
    """x [B, T, d] fp32 -> (flat allocation of (B + 1) stride_b + offset floats full of the sentinel, strided view of x in it)."""
    B, T, d = x.shape
    assert stride_b >= T * d
    flat = torch.full(((B + 1) * stride_b + offset,), SENTINEL, dtype=torch.float32, device=x.device)
    view = torch.as_strided(flat, (B, T, d), (stride_b, d, 1), storage_offset=offset)
    view.copy_(x)
    return flat, view


def reference(x, de, g, r):
    """fp64 sums over the samples x [N, d] (fp32 values), and the same sums of magnitudes."""
    N, d = x.shape
    x = x.double()
    iu = torch.triu_indices(d, d, device=x.device)
    out = []
    for dv, dg in ((de, de * g), (de.abs(), (de * g).abs())):
        M = (x * dv[:, None]).T @ x
        out.append(torch.cat([M[iu[0], iu[1]], (x * dv[:, None]).sum(0), dv.sum()[None], dg.sum()[None],
                              r.double().sum()[None], torch.tensor([float(N)], dtype=torch.float64, device=x.device)]))
    return out[0], out[1]


def inputs(dev, d, B, T, seed):
    rs = np.random.RandomState(seed)
    x = t32(rs.dirichlet(np.ones(d), size=(B, T)), dev)
    return x, t64(rs.randn(B, T), dev), t64(rs.randn(B, T), dev), t32(rs.rand(B, T), dev)


def within(G, ref, d, what, factor=1.0):
    Q = d * (d + 1) // 2
    scale = max(float(ref[:Q].abs().max()), 1e-300)
    e_q = float((G[:Q] - factor * ref[:Q]).abs().max())
    e_r = float((G[Q:] - factor * ref[Q:]).abs().max())
    lim_r = 1e-11 * max(1.0, float(ref[Q:].abs().max()))
    assert e_q <= 1e-12 * scale, (what, 'quadratic block', e_q / scale)
    assert e_r <= lim_r, (what, 'linear / scalar entries', e_r / lim_r)
    assert float(G[-1]) == factor * float(ref[-1]), (what, 'count')
    return e_q / (1e-12 * scale), e_r / lim_r


def run_case(dev, d, B, T, stride_b, add_reward, offset=0, seed=None, data=None, what=None):
    """One layout through mfg_grad_accumulate, every criterion of the module docstring; returns (G, ref)."""
    o_ = ops()
    x, delta, g, r = data if data is not None else inputs(dev, d, B, T, d * 3 + B + T if seed is None else seed)
    flat, pi = lay_out(x, stride_b, offset)
    N = B * T
    G = torch.full((o_.num_features(d) + 3,), 7.0, dtype=torch.float64, device=dev)
    ws = o_.workspace(N, d, dev)
    dl = delta.clone()
    o_.grad_accumulate(pi, dl, g, r, G, ws, T=T, stride_b=stride_b, add_reward=add_reward)
    de = (delta + r.double()) if add_reward else delta
    what = what or (d, B, T, stride_b, offset, add_reward)
    assert torch.equal(dl, de), what
    ref, mag = reference(x.reshape(N, d), de.reshape(N), g.reshape(N), r.reshape(N))
    rq, rr = within(G, ref, d, what)
    G1 = G.clone()
    o_.grad_accumulate(pi, de.clone(), g, r, G, ws, T=T, stride_b=stride_b, accumulate=True)
    within(G, ref, d, (what, 'accumulate'), factor=2.0)
    # (the a-priori bound N u sum |terms| for comparison: the criteria above are the tighter ones at these sizes)
    apriori = float(((G1 - ref).abs() / (N * U * mag).clamp_min(1e-300))[:-1].max())
    print('batch sums %r: error / criterion %.3g (quadratic) %.3g (rest); error / (N u sum|terms|) %.3g' % (what, rq, rr, apriori))
    assert float(flat.max()) == SENTINEL                                  # (the spare stride: the layout was left alone)
    return G1, ref


def agree(Ga, Gb, ref, d, what):
    """Two launches over the same values (different kernels or address forms): the module's tolerance, relative to the reference."""
    Q = d * (d + 1) // 2
    assert float((Ga[:Q] - Gb[:Q]).abs().max()) <= 1e-12 * float(ref[:Q].abs().max()), what
    assert float((Ga[Q:] - Gb[Q:]).abs().max()) <= 1e-11 * max(1.0, float(ref[Q:].abs().max())), what


# ---- a. strides of the d <= 28 kernel ----------------------------------------------------------------------------------
# N = B T is two or more 64-sample chunks with a ragged last one (T = 64: N is a multiple of 64 whatever B is -- there every
# chunk starts on a trajectory boundary)
SMALL_BT = {1: 131, 3: 43, 64: 3, 65: 3}


@pytest.mark.parametrize('add_reward', [False, True])
@pytest.mark.parametrize('T', [1, 3, 64, 65])
@pytest.mark.parametrize('d', [21, 15, 1, 2, 16, 17, 28])
def test_small_d_strides(dev, d, T, add_reward):
    """k_grad_mfma_small<21>, <15> and the run-time-d form: element e of a chunk sits at base + e + q extra, q the trajectory
    boundaries in front of its sample, for skipped parts extra = stride_b - T d of 0, 1, 3, d and 4097 floats."""
    B = SMALL_BT[T]
    data = inputs(dev, d, B, T, 1000 * d + T)
    for extra in sorted({0, 1, 3, d, 4097}):
        run_case(dev, d, B, T, T * d + extra, add_reward, data=data)


def test_small_d_wide_strides(dev):
    """The last stride of the 32-bit offset form (extra = 2^23 - 1) and the first of the wide form, k_grad_mfma_small<0, true>
    (extra = 2^23 and 2^23 + 5), at d = 21, T = 3, B = 24: 72 samples, a full chunk and a ragged one, 0.84 GB of sentinel.
    The same values in all three: the sums agree across the address forms."""
    d, T, B = 21, 3, 24
    data = inputs(dev, d, B, T, 77)
    Gs = []
    for extra in ((1 << 23) - 1, 1 << 23, (1 << 23) + 5):
        G, ref = run_case(dev, d, B, T, T * d + extra, add_reward=False, data=data)
        Gs.append(G)
        torch.cuda.empty_cache()
    agree(Gs[0], Gs[1], ref, d, 'extra 2^23 - 1 / 2^23')
    agree(Gs[0], Gs[2], ref, d, 'extra 2^23 - 1 / 2^23 + 5')
    run_case(dev, d, B, T, T * d + (1 << 23) + 5, add_reward=True, data=data)
    # the wide form counts the boundaries of T >= 64 with a compare: T = 65, three trajectories in four chunks
    run_case(dev, 2, 3, 65, 65 * 2 + (1 << 23), add_reward=True)


# ---- b. every tile layout of the matrix-core kernels, d >= 64 --------------------------------------------------------------
@pytest.mark.parametrize('add_reward', [False, True])
@pytest.mark.parametrize('d', list(range(64, 513, 16)))
def test_tile_sweep(dev, d, add_reward):
    """k_grad_mfma (k_grad_mfma2 at d = 128 / 256) at every multiple of 16: each d is another (grid rows, tiles per wave,
    ragged last run) of the upper-triangle tile list.  B = 67, T = 3: six 32-sample chunks and 9 samples; at d = 64 a block
    takes several chunks, at d = 512 about half the blocks have no sample and leave zero rows."""
    run_case(dev, d, 67, 3, 4 * d, add_reward)


@pytest.mark.parametrize('add_reward', [False, True])
@pytest.mark.parametrize('B,T', [(1, 1), (11, 3)])
@pytest.mark.parametrize('d', [64, 80, 512])
def test_tile_sweep_one_chunk(dev, d, B, T, add_reward):
    """One sample, and 33 (one chunk and one sample), through the pipelined (d = 64, 512) and the scalar-staged (d = 80) body."""
    run_case(dev, d, B, T, (T + 1) * d, add_reward)


# ---- c. staging fall-backs -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('d', [64, 128, 256, 512])
def test_staging_fallbacks(dev, d):
    """float4 staging needs a 16-byte aligned `pi` and stride_b % 4 == 0.  Otherwise d = 128 / 256 run k_grad_mfma<0> in place
    of k_grad_mfma2 and d = 64 / 512 the unpipelined scalar body in place of NPF = 2 / 16: the same sums as the aligned call
    on the same values (another kernel or another staging order: the tolerance, not equality).
    What this proves: the fall-back kernels give the right sums for misaligned input.  What it cannot prove: that the host
    TAKES them -- the pipelined bodies load float4 from global memory whatever the alignment, the hardware serves a misaligned
    16-byte global load, and a host that kept NPF = d / 32 for a misaligned `pi` changes no result here (tried, docs/HISTORY.md)."""
    B, T = 67, 3
    data = inputs(dev, d, B, T, 5 * d)
    G0, ref = run_case(dev, d, B, T, (T + 1) * d, False, data=data)
    for offset, stride_b in ((1, (T + 1) * d), (2, (T + 1) * d), (0, (T + 1) * d + 1), (0, (T + 1) * d + 2), (3, (T + 1) * d + 3)):
        for add_reward in (False, True):
            G1, _ = run_case(dev, d, B, T, stride_b, add_reward, offset=offset, data=data)
            if not add_reward:
                agree(G0, G1, ref, d, (d, offset, stride_b))


def test_staging_fallback_control_d80(dev):
    """d = 80 is on the scalar staging path whatever the alignment (256 is no multiple of 80 / 4): the control."""
    d, B, T = 80, 67, 3
    data = inputs(dev, d, B, T, 401)
    G0, ref = run_case(dev, d, B, T, (T + 1) * d, False, data=data)
    for offset, stride_b in ((0, (T + 1) * d + 1), (0, (T + 1) * d + 2), (1, (T + 1) * d)):
        G1, _ = run_case(dev, d, B, T, stride_b, False, offset=offset, data=data)
        assert torch.equal(G0, G1)                                    # the same kernel, the same order


# ---- d. the generic kernel ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('add_reward', [False, True])
@pytest.mark.parametrize('d', [29, 63, 65, 127, 129, 255, 257, 511])
def test_generic_kernel_chunk_sizes(dev, d, add_reward):
    """k_grad_partial stages min(64, 8192 // d) samples per block: 64, 64, 64, 64, 63, 32, 31, 16 here.  N = 3 B is two such
    chunks and a ragged third; the pi_traj stride and an odd one."""
    chunk = min(64, 8192 // d)
    B, T = (2 * chunk) // 3 + 2, 3
    assert 2 * chunk < B * T < 3 * chunk
    data = inputs(dev, d, B, T, 7 * d)
    run_case(dev, d, B, T, (T + 1) * d, add_reward, data=data)
    run_case(dev, d, B, T, T * d + 5, add_reward, data=data)


# ---- e. long trajectories ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('T', [4194000, 6556022, 8388610])
def test_long_trajectories(dev, T):
    """d = 2, B = 2, stride (T + 1) d.  The fp32 reciprocal multiply that counts trajectory boundaries puts step T - 1 behind the
    boundary from T = 6 556 022 on (tests/test_grad_index_host.py): until the host sent T >= 2^22 to the wide form, which
    compares, the kernel read the spare state row T, here the sentinel, for the last sample of each trajectory.  T = 4 194 000
    is the control: below 2^22, the multiply, exact.  delta is non-zero only in the first and the last 64 steps of each
    trajectory, so one misplaced row is an O(1/256) error of the delta-weighted sums even without the sentinel; the reward is
    dense.
    Tolerances a priori: n u sum |terms| with n = 256 non-zero terms for the delta-weighted entries (zero terms and all-zero
    partial rows add exactly), N u sum |r| for the reward sum, u = 2^-53; the count is exact.
    Measured error / bound (MI355X): at most 0.0025 for the delta-weighted entries, 1e-7 for the reward sum.  The library of
    the commit before failed T = 6 556 022 and 8 388 610 with ratios of 1e72 (the sentinel) and passed the control."""
    o_ = ops()
    d, B = 2, 2
    N, stride_b = B * T, (T + 1) * d
    gen = torch.Generator(device=dev)
    gen.manual_seed(T)
    u = torch.rand(B, T, device=dev, generator=gen)
    x = torch.stack([u, 1.0 - u], -1)                                  # Dirichlet(1, 1) rows
    flat, pi = lay_out(x, stride_b)
    nz = torch.cat([torch.arange(64, device=dev), torch.arange(T - 64, T, device=dev)])
    delta = torch.zeros(B, T, dtype=torch.float64, device=dev)
    delta[:, nz] = torch.randn(B, 128, dtype=torch.float64, device=dev, generator=gen)
    g = torch.randn(B, T, dtype=torch.float64, device=dev, generator=gen)
    r = torch.rand(B, T, device=dev, generator=gen)
    G = torch.full((o_.num_features(d) + 3,), 7.0, dtype=torch.float64, device=dev)
    ws = o_.workspace(N, d, dev)
    dl = delta.clone()
    o_.grad_accumulate(pi, dl, g, r, G, ws, T=T, stride_b=stride_b)
    assert torch.equal(dl, delta)
    n = B * 128
    ref, mag = reference(x[:, nz].reshape(n, d), delta[:, nz].reshape(n), g[:, nz].reshape(n), r[:, nz].reshape(n))
    F = o_.num_features(d)
    ratio = float(((G[:F + 1] - ref[:F + 1]).abs() / (n * U * mag[:F + 1])).max())
    r_sum = float(r.double().sum())
    ratio_r = abs(float(G[F + 1]) - r_sum) / (N * U * r_sum)
    print('long T = %d: error / bound %.3g (delta-weighted sums, n = %d), %.3g (reward sum, N = %d)' % (T, ratio, n, ratio_r, N))
    assert ratio <= 1.0, ratio
    assert ratio_r <= 1.0, ratio_r
    assert float(G[F + 2]) == N


def test_small_d_refuses_T_beyond_its_index_range(dev):
    """d <= 28 serves T <= 2^31 - 65 (include/mfg_hip.h); one more is refused with MFG_EUNSUPPORTED before anything is launched.
    The buffers hold 64 elements: the call is safe only BECAUSE it is refused, which is why the check is the first statement of
    launch_grad, in front of the workspace check, and must stay there.  Never point this test at a library without the check
    (the commit before this test, for one): it would launch the kernel over 2^31 samples of these buffers."""
    from discrete_mean_field_game_amd import _lib as L
    o_ = ops()
    d, T = 2, 2 ** 31 - 64
    buf = torch.zeros(64, dtype=torch.float32, device=dev)
    dd = torch.zeros(64, dtype=torch.float64, device=dev)
    G = torch.zeros(o_.num_features(d) + 3, dtype=torch.float64, device=dev)
    ws = o_.workspace(1 << 20, d, dev)
    rc = L.lib().mfg_grad_accumulate(buf.data_ptr(), T * d, dd.data_ptr(), None, None, 1, T, d, 0, G.data_ptr(), 0, ws.data_ptr(),
                                     ws.numel() * 8, None)
    assert rc == -3 and b'2^31 - 65' in L.lib().mfg_last_error()
    assert float(G.abs().max()) == 0.0
