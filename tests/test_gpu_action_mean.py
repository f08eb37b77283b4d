"""-m gpu: mfg_action_mean_pop (ops.action_mean_pop) against np.mean of the fp64 copy (np.mean(np.asarray(actions), axis=0),
ac_irl.py:1276-1289): stacked and shared inputs, N around the chunk length of 32 and past the cap of 1024 chunks, learner k of
K the same bits as alone, and the refusals."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
U = 2.0 ** -52


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.fail('-m gpu tests need a GPU')
    return torch.device('cuda:0')


@functools.lru_cache(maxsize=None)
def _actions(K, N, d):
    """Row-stochastic matrices in [0, 1] as fp32 [K, N, d, d] (computed once per shape; never changed)."""
    rs = np.random.RandomState(K * 100003 + N * 101 + d)
    a = rs.dirichlet(np.ones(d), size=(K, N, d)).astype(np.float32)
    a.setflags(write=False)
    return a


# N = 1 | just below, at and past two chunks of 32 matrices | 32 chunks
@pytest.mark.parametrize('N', (1, 63, 64, 65, 1000))
@pytest.mark.parametrize('d', (15, 21, 64))
def test_mean_is_numpys_and_learner_k_is_the_k1_call(dev, d, N):
    from discrete_mean_field_game_amd import ops
    a = _actions(5, N, d)
    t = torch.tensor(a, device=dev)
    got5 = ops.action_mean_pop(t).cpu().numpy()
    assert got5.shape == (5, d, d) and got5.dtype == np.float64
    want = np.mean(a.astype(np.float64), axis=1)
    assert np.abs(got5 - want).max() <= N * U
    for k in range(5):
        alone = ops.action_mean_pop(t[k:k + 1].contiguous()).cpu().numpy()       # K = 1, stacked
        assert np.array_equal(alone[0], got5[k]), k
    shared1 = ops.action_mean_pop(t[2].contiguous()).cpu().numpy()               # K = 1, shared input (s_action = 0)
    assert np.array_equal(shared1[0], got5[2])
    shared5 = ops.action_mean_pop(t[2].contiguous(), K=5).cpu().numpy()          # K = 5 learners read one input
    assert shared5.shape == (5, d, d)
    for k in range(5):
        assert np.array_equal(shared5[k], got5[2]), k


def test_past_the_chunk_cap(dev):
    from discrete_mean_field_game_amd import ops
    d, N = 15, 32 * 1024 + 900                   # 1024 chunks of 33 matrices: the last chunks are empty
    a = _actions(1, N, d)
    got = ops.action_mean_pop(torch.tensor(a, device=dev)).cpu().numpy()
    want = np.mean(a.astype(np.float64), axis=1)
    assert np.abs(got - want).max() <= N * U


def test_refusals_write_nothing(dev):
    from discrete_mean_field_game_amd import _lib as L
    K, N, d = 3, 70, 15
    t = torch.from_numpy(_actions(5, 65, 15)[:K].copy()).to(dev)      # (any buffer of at least K N' d d floats)
    t = torch.cat([t, t], dim=1)[:, :N].contiguous()
    mean = torch.full((K, d, d), -7.0, dtype=torch.float64, device=dev)
    need = int(L.lib().mfg_action_mean_pop_workspace_bytes(K, N, d))
    assert need == K * 3 * d * d * 8
    ws = torch.full((need // 8,), -7.0, dtype=torch.float64, device=dev)
    st = torch.cuda.current_stream().cuda_stream

    def call(K_=K, N_=N, d_=d, s=N * d * d, nbytes=need):
        L.check(L.lib().mfg_action_mean_pop(t.data_ptr(), s, K_, N_, d_, mean.data_ptr(), ws.data_ptr(), nbytes, st),
                'mfg_action_mean_pop')
    for kw, code in ((dict(nbytes=need - 1), -4), (dict(nbytes=0), -4), (dict(K_=0), -1), (dict(N_=0), -1), (dict(d_=0), -1),
                     (dict(s=N * d * d - 1), -1), (dict(d_=65, s=N * 65 * 65), -3)):
        with pytest.raises(L.MfgError) as e:
            call(**kw)
        assert e.value.code == code, kw
    torch.cuda.synchronize()
    assert bool((mean == -7.0).all()) and bool((ws == -7.0).all())
    call()
    torch.cuda.synchronize()
    want = np.mean(t.cpu().numpy().astype(np.float64), axis=1)
    assert np.abs(mean.cpu().numpy() - want).max() <= N * U
