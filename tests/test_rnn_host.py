"""CPU: the RNN population call without a GPU -- the restatement itself (tests/rnn_ref.py) pinned against torch.autograd and
torch.optim.Adam in fp64, the cap on its own rounding error that the GPU tolerances are built from, the descriptor structs against
the C compiler, the two new symbols, the refusals of the library and of the Python layer, RnnFits and the trajectory file."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import rnn_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = [c for c in R.CASES if c[1] <= 32]


@pytest.fixture(scope='module')
def lib():
    from discrete_mean_field_game_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib


# ---------------------------------------------------------------------------------------------------- the restatement
def _torch_loss(torch, w, H, d, Y, wd):
    """The loss on an LSTMCell-form graph: torch.nn.functional's own cell arithmetic written with torch ops (gate order i, f, g,
    o as torch.nn.LSTMCell; its two biases are one here), so that autograd, not this file, forms the gradient."""
    G = 4 * H
    at = np.cumsum([0, G * d, G * H, G, d * H, d])
    Wx, Wh, b, Wo, bo = (w[at[q]:at[q + 1]] for q in range(5))
    Wx, Wh, Wo = Wx.reshape(G, d), Wh.reshape(G, H), Wo.reshape(d, H)
    N, Hd, _ = Y.shape
    h = c = torch.zeros(N, H, dtype=torch.float64)
    loss = 0.0
    for t in range(Hd - 1):
        i, f, g, o = (Y[:, t] @ Wx.T + h @ Wh.T + b).chunk(4, dim=1)
        c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
        h = torch.sigmoid(o) * torch.tanh(c)
        loss = loss - (Y[:, t + 1] * torch.log_softmax(h @ Wo.T + bo, dim=1)).sum()
    return loss / (N * (Hd - 1)) + 0.5 * wd * (w * w).sum()


def test_the_cell_is_torchs_lstmcell():
    torch = pytest.importorskip('torch')
    d, H = 5, 8
    w = R.init_weights(H, d, 3)
    Wx, Wh, b, _, _ = R.unpack(w, H, d)
    cellm = torch.nn.LSTMCell(d, H).double()
    with torch.no_grad():
        cellm.weight_ih.copy_(torch.as_tensor(Wx)), cellm.weight_hh.copy_(torch.as_tensor(Wh))
        cellm.bias_ih.copy_(torch.as_tensor(b)), cellm.bias_hh.zero_()
        rs = np.random.RandomState(0)
        x, h, c = rs.rand(4, d), rs.randn(4, H), rs.randn(4, H)
        h2, c2 = cellm(torch.as_tensor(x), (torch.as_tensor(h), torch.as_tensor(c)))
    got_h, got_c, _ = R.cell(w, H, d, x, h, c)
    assert np.abs(got_h - h2.numpy()).max() <= 1e-14 and np.abs(got_c - c2.numpy()).max() <= 1e-14


@pytest.mark.parametrize('case', R.CASES, ids=R.case_id)
@pytest.mark.parametrize('wd', [0.0, 1e-3])
def test_the_gradient_by_hand_is_autograds(case, wd):
    """1e-10 relative per element (relative to the larger of the element and 1e-3 of the gradient's largest entry: an entry that
    is zero up to rounding has no relative error)."""
    torch = pytest.importorskip('torch')
    d, H, n, Hd = case
    days, tr, _, _ = R.case_days(case)
    w0 = R.init_weights(H, d, 11)
    loss, g = R.loss_and_grad(w0, H, d, days[tr], wd)
    w = torch.tensor(w0, requires_grad=True)
    lt = _torch_loss(torch, w, H, d, torch.as_tensor(days[tr]), wd)
    lt.backward()
    gt = w.grad.numpy()
    rel = np.abs(g - gt) / np.maximum(np.abs(gt), 1e-3 * np.abs(gt).max())
    print('%s wd %g: loss %.3e vs %.3e, max rel %.2e' % (R.case_id(case), wd, loss, float(lt.detach()), rel.max()))
    assert abs(loss - float(lt.detach())) <= 1e-12 * abs(float(lt.detach())) and rel.max() <= 1e-10


@pytest.mark.parametrize('case', SMALL, ids=R.case_id)
def test_eight_adam_steps_are_torch_optim_adams(case):
    torch = pytest.importorskip('torch')
    d, H, n, Hd = case
    days, tr, _, _ = R.case_days(case)
    w0 = R.init_weights(H, d, 12)
    got = R.train(w0, H, d, days[tr], 8, 1e-2, wd=1e-3)
    w = torch.tensor(w0, requires_grad=True)
    opt = torch.optim.Adam([w], lr=1e-2)              # (the decay term is part of the loss, as in the restatement)
    Y = torch.as_tensor(days[tr])
    losses = []
    for _ in range(8):
        opt.zero_grad()
        lt = _torch_loss(torch, w, H, d, Y, 1e-3)
        lt.backward()
        opt.step()
        losses.append(float(lt.detach()))
    err = np.abs(got['last'] - w.detach().numpy()).max()
    print('%s: 8 Adam steps, max |dw| %.2e' % (R.case_id(case), err))
    assert err <= 1e-9 and np.abs(got['loss'] - np.array(losses)).max() <= 1e-12


def test_clipping_sgd_and_selection_of_the_restatement():
    d, H = 3, 4
    days, tr, va, _ = R.case_days((d, H, 2, 16))
    w0 = R.init_weights(H, d, 1)
    loss, g = R.loss_and_grad(w0, H, d, days[tr])
    gn = np.sqrt((g * g).sum())
    one = R.train(w0, H, d, days[tr], 1, 0.5, optimizer='sgd')
    assert np.allclose((w0 - one['last']) / 0.5, g, rtol=1e-12, atol=1e-15) and one['loss'][0] == loss and one['best_epoch'] == 1
    clipped = R.train(w0, H, d, days[tr], 1, 0.5, clip=gn / 4, optimizer='sgd')
    assert np.allclose((w0 - clipped['last']) / 0.5, g / 4, rtol=1e-12, atol=1e-15)
    sel = R.train(w0, H, d, days[tr], 6, 1e-2, Yval=days[va], eval_every=4)
    assert len(sel['val']) == 2 and sel['best_epoch'] in (4, 6) and sel['best_epoch'] == (4 if sel['val'][0] <= sel['val'][1] else 6)
    # the forecast starts from the observed row and stays on the simplex
    fut = R.forecast(w0, H, d, days[va])
    assert np.array_equal(fut[:, 0], days[va][:, 0]) and np.allclose(fut.sum(axis=2), 1.0)
    per_day, met = R.metrics(fut, days[va])
    assert per_day.shape == (2, 4) and met[6] == per_day[:, 3].mean()


@pytest.mark.parametrize('case', SMALL, ids=R.case_id)
def test_the_restatements_own_rounding_error_is_small(case):
    """The GPU tests allow 64 x this gap: it must not be able to grow large enough to hide an fp32 slip (5e-8 and more in the
    weights after 8 Adam steps)."""
    d, H, n, Hd = case
    days, tr, va, _ = R.case_days(case)
    w0 = R.init_weights(H, d, 12)
    a = R.train(w0, H, d, days[tr], 8, 1e-2)
    b = R.train(w0, H, d, days[tr], 8, 1e-2, dtype=np.longdouble)
    gap = float(np.abs(a['last'] - b['last']).max())
    print('%s: fp64 against longdouble after 8 Adam steps %.2e' % (R.case_id(case), gap))
    assert 64 * gap <= 1e-9


# ---------------------------------------------------------------------------------------------------- the C boundary
@pytest.mark.parametrize('ctype,name', [('mfg_rnn_model_t', 'RnnModelStruct'), ('mfg_rnn_fit_t', 'RnnFitStruct')])
def test_struct_layouts_match_the_header(lib, tmp_path, ctype, name):
    st = getattr(lib, name)
    fields = [n for n, _ in st._fields_]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "mfg_hip.h"\nint main(void){printf("%%zu", sizeof(%s));\n' % ctype
    for f in fields:
        src += 'printf(" %%zu", offsetof(%s, %s));\n' % (ctype, f)
    src += 'return 0;}\n'
    c = tmp_path / 'layout.c'
    c.write_text(src)
    exe = str(tmp_path / 'layout')
    subprocess.run(['gcc', '-std=c99', '-I', os.path.join(ROOT, 'include'), str(c), '-o', exe], check=True)
    out = [int(x) for x in subprocess.run([exe], check=True, stdout=subprocess.PIPE).stdout.decode().split()]
    assert out[0] == C.sizeof(st)
    assert out[1:] == [getattr(st, f).offset for f in fields]
    text = open(os.path.join(ROOT, 'include', 'mfg_hip.h')).read()
    body = re.search(r'typedef struct \w+ \{([^}]*)\} %s;' % ctype, text).group(1)
    assert len(re.findall(r'[\w\]]\s*[,;]', body)) == len(fields)          # (no member of the header is missing from the mirror)


def test_the_new_symbols_are_declared_bound_and_exported(lib):
    raw = open(os.path.join(ROOT, 'include', 'mfg_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', raw, flags=re.S)
    h = lib.lib()
    for name in ('mfg_rnn_fit_pop', 'mfg_rnn_fit_workspace_bytes'):
        assert re.search(r'\b%s\s*\(' % name, text) and name in lib.SIGNATURES and getattr(h, name) is not None
    assert not re.search(r'mfg_rnn_fit_pop\s*\([^)]*mfg_stream_t', text)          # the stream is a member of the descriptor
    assert int(re.search(r'#define MFG_RNN_MAX_EPOCHS (\d+)', text).group(1)) == lib.RNN_MAX_EPOCHS == 65535
    for cite in ('process.py:4-22', 'mfg_ac2.py:757-761', 'plots.py:29-30'):   # what the entry stands in for
        assert cite in raw and cite in open(os.path.join(ROOT, 'discrete_mean_field_game_amd', 'csrc', 'mfg_rnn_pop.h')).read()
    assert h.mfg_abi_version() == 18


def _table(lib, rows):
    t = (lib.RnnModelStruct * len(rows))()
    for x, (H, E, ntr, nva, nte, lr, wd, clip) in zip(t, rows):
        x.hidden, x.epochs, x.n_train, x.n_val, x.n_test, x.lr, x.wd, x.clip = H, E, ntr, nva, nte, lr, wd, clip
    return t


GOOD = (8, 10, 3, 1, 1, 1e-2, 0.0, 0.0)


def test_workspace_layout(lib):
    h = lib.lib()
    t = _table(lib, [GOOD, (64, 5, 13, 0, 5, 1e-3, 0.0, 1.0), GOOD])
    total = h.mfg_rnn_fit_workspace_bytes(3, t, 15, 16)
    assert t[0].ws_offset == 0 and 0 < t[1].ws_offset < t[2].ws_offset < total
    assert t[1].ws_offset % 256 == 0 and t[2].ws_offset % 256 == 0 and total % 256 == 0
    assert total - t[2].ws_offset == t[1].ws_offset                 # the same record, the same slice
    # the saved activations of the H = 64 model: six [15 hours][64][16 days] planes and the logits, at least
    assert t[2].ws_offset - t[1].ws_offset >= 8 * 15 * 16 * (9 * 64 + 15)
    for K, tab, d, Hd in ((0, t, 15, 16), (3, None, 15, 16), (3, t, 1, 16), (3, t, 65, 16), (3, t, 15, 1), (3, t, 15, 65)):
        assert h.mfg_rnn_fit_workspace_bytes(K, tab, d, Hd) == 0
    t[1].hidden = 6
    assert h.mfg_rnn_fit_workspace_bytes(3, t, 15, 16) == 0


def _fit(lib, rows, d=3, Hd=16, D=8, W_max=None, E_max=None, C_max=None, strides=(4, 4, 4), ws_bytes=None, optimizer=0, eval_every=1,
         **nulls):
    """A descriptor whose device pointers are dummies: every refusal below happens before anything is launched or read."""
    from discrete_mean_field_game_amd import ops
    h = lib.lib()
    t = _table(lib, rows)
    total = h.mfg_rnn_fit_workspace_bytes(len(rows), t, d, Hd)
    f = lib.RnnFitStruct()
    for name in ('days', 'models', 'train_idx', 'val_idx', 'test_idx', 'w0', 'weights', 'loss', 'val', 'best_epoch', 'future',
                 'per_day', 'metrics', 'status', 'workspace'):
        setattr(f, name, None if nulls.get(name) else 4096)
    f.models_host = C.addressof(t)
    f.workspace_bytes = total if ws_bytes is None else ws_bytes
    f.D, f.Hd, f.d, f.K = D, Hd, d, len(rows)
    f.train_stride, f.val_stride, f.test_stride = strides
    f.W_max = max([ops.rnn_weight_count(max(r[0], 0), max(d, 0)) for r in rows] + [1]) if W_max is None else W_max
    f.E_max = max([r[1] for r in rows] + [1]) if E_max is None else E_max
    f.C_max = max([r[1] for r in rows] + [1]) if C_max is None else C_max
    f.optimizer, f.eval_every = optimizer, eval_every
    return f, t


def _row(**kw):
    names = ('hidden', 'epochs', 'n_train', 'n_val', 'n_test', 'lr', 'wd', 'clip')
    return [tuple(kw.get(n, v) for n, v in zip(names, GOOD))]


@pytest.mark.parametrize('why,kw', [
    ('d = 1', dict(d=1)), ('d = 65', dict(d=65)), ('Hd = 1', dict(Hd=1)), ('Hd = 65', dict(Hd=65)), ('D = 0', dict(D=0)),
    ('H = 0', dict(rows=_row(hidden=0))), ('H = 6', dict(rows=_row(hidden=6))), ('H = 68', dict(rows=_row(hidden=68))),
    ('no epoch', dict(rows=_row(epochs=0))), ('65536 epochs', dict(rows=_row(epochs=65536), E_max=70000, C_max=70000)),
    ('no training day', dict(rows=_row(n_train=0))), ('65 training days', dict(rows=_row(n_train=65), strides=(65, 4, 4))),
    ('more training days than the table', dict(rows=_row(n_train=5))), ('65 validation days', dict(rows=_row(n_val=65), strides=(4, 65, 4))),
    ('validation days < 0', dict(rows=_row(n_val=-1))), ('more validation days than the table', dict(rows=_row(n_val=5))),
    ('65 test days', dict(rows=_row(n_test=65), strides=(4, 4, 65))), ('test days < 0', dict(rows=_row(n_test=-1))),
    ('lr 0', dict(rows=_row(lr=0.0))), ('lr < 0', dict(rows=_row(lr=-1.0))), ('lr inf', dict(rows=_row(lr=float('inf')))),
    ('lr nan', dict(rows=_row(lr=float('nan')))), ('wd < 0', dict(rows=_row(wd=-1e-3))), ('wd nan', dict(rows=_row(wd=float('nan')))),
    ('clip < 0', dict(rows=_row(clip=-1.0))), ('clip inf', dict(rows=_row(clip=float('inf')))),
    ('W_max too small', dict(W_max=10)), ('E_max too small', dict(E_max=9)), ('C_max too small', dict(C_max=9)),
    ('optimizer 2', dict(optimizer=2)), ('eval_every 0', dict(eval_every=0)),
    ('null days', dict(days=True)), ('null w0', dict(w0=True)), ('null weights', dict(weights=True)), ('null loss', dict(loss=True)),
    ('null val', dict(val=True)), ('null future', dict(future=True)), ('null status', dict(status=True)),
    ('null device table', dict(models=True)), ('null workspace', dict(workspace=True)), ('null val_idx', dict(val_idx=True)),
    ('second model bad', dict(rows=[GOOD] + _row(lr=0.0)))])
def test_the_library_refuses_with_einval_before_it_launches(lib, why, kw):
    kw = dict(kw)
    f, t = _fit(lib, kw.pop('rows', [GOOD]), **kw)
    assert lib.lib().mfg_rnn_fit_pop(C.byref(f)) == -1, why          # MFG_EINVAL


def test_the_library_checks_the_layout_and_the_workspace_size(lib):
    h = lib.lib()
    assert h.mfg_rnn_fit_pop(None) == -1
    f, t = _fit(lib, [GOOD, GOOD], ws_bytes=512)
    assert h.mfg_rnn_fit_pop(C.byref(f)) == -4                       # MFG_EWORKSPACE
    f, t = _fit(lib, [GOOD, GOOD])
    t[1].ws_offset += 256
    assert h.mfg_rnn_fit_pop(C.byref(f)) == -1 and b'ws_offset' in h.mfg_last_error()
    f, t = _fit(lib, [GOOD])
    f.workspace = 4100
    assert h.mfg_rnn_fit_pop(C.byref(f)) == -1 and b'aligned' in h.mfg_last_error()


# ---------------------------------------------------------------------------------------------------- the Python layer
def test_ops_argument_rules():
    from discrete_mean_field_game_amd import ops
    ok = dict(hidden=[8], epochs=[10], lrs=[1e-2], wds=[0.0], clips=[0.0], train_n=[3], val_n=[1], test_n=[1])
    assert ops.rnn_weight_count(8, 3) == 4 * 8 * 12 + 3 * 9 == R.weight_count(8, 3)
    assert ops.check_rnn_fit_args((8, 16, 3), **ok) == (1, 8, 16, 3, 411, 10, 10)
    assert ops.check_rnn_fit_args((8, 16, 3), eval_every=4, **ok)[6] == 3          # epochs 4, 8 and the last
    two = ops.check_rnn_fit_args((8, 16, 3), [4, 64], [7, 300], [1.0, 2.0], [0, 0], [0, 1], [1, 64], [0, 2], [0, 64], 'sgd', 100)
    assert two == (2, 8, 16, 3, ops.rnn_weight_count(64, 3), 300, 3)
    assert ops.check_rnn_fit_args((8, 16, 3), **dict(ok, val_n=[0]))[6] == 0
    for shape, bad in (((8, 16), {}), ((8, 16, 65), {}), ((8, 16, 1), {}), ((8, 1, 3), {}), ((8, 65, 3), {}), ((0, 16, 3), {}),
                       ((8, 16, 3), dict(hidden=[0])), ((8, 16, 3), dict(hidden=[6])), ((8, 16, 3), dict(hidden=[68])),
                       ((8, 16, 3), dict(epochs=[0])), ((8, 16, 3), dict(epochs=[65536])), ((8, 16, 3), dict(train_n=[0])),
                       ((8, 16, 3), dict(train_n=[65])), ((8, 16, 3), dict(val_n=[65])), ((8, 16, 3), dict(val_n=[-1])),
                       ((8, 16, 3), dict(test_n=[65])), ((8, 16, 3), dict(test_n=[-1])), ((8, 16, 3), dict(lrs=[0.0])),
                       ((8, 16, 3), dict(lrs=[float('nan')])), ((8, 16, 3), dict(lrs=[float('inf')])), ((8, 16, 3), dict(wds=[-1.0])),
                       ((8, 16, 3), dict(wds=[float('inf')])), ((8, 16, 3), dict(clips=[-1.0])), ((8, 16, 3), dict(clips=[float('nan')])),
                       ((8, 16, 3), dict(optimizer='rmsprop')), ((8, 16, 3), dict(eval_every=0)), ((8, 16, 3), dict(eval_every=1.5)),
                       ((8, 16, 3), dict(hidden=[])), ((8, 16, 3), dict(hidden=[8, 8]))):
        a = dict(ok)
        a.update(bad)
        with pytest.raises(ValueError):
            ops.check_rnn_fit_args(shape, **a)
    for stride in (dict(train_stride=2), dict(val_stride=0), dict(test_stride=0)):
        with pytest.raises(ValueError):
            ops.check_rnn_fit_args((8, 16, 3), **dict(ok, **stride))


def test_the_model_table_and_the_shapes(lib):
    from discrete_mean_field_game_amd import ops
    table, nbytes = ops.rnn_models([8, 16], [10, 20], [1e-2, 1e-3], [0, 1e-4], [0, 1.0], [3, 4], [1, 0], [1, 2], 3, 16)
    assert nbytes % 256 == 0 and table[0].ws_offset == 0 and 0 < table[1].ws_offset < nbytes
    assert (table[1].hidden, table[1].epochs, table[1].n_train, table[1].n_val, table[1].n_test) == (16, 20, 4, 0, 2)
    assert (table[1].lr, table[1].wd, table[1].clip) == (1e-3, 1e-4, 1.0)
    with pytest.raises(ValueError):
        ops.rnn_models([6], [10], [1e-2], [0], [0], [3], [1], [1], 3, 16)
    torch = pytest.importorskip('torch')
    shapes = ops.rnn_fit_shapes(2, 16, 3, 100, 20, 5, 2)
    assert shapes['future'] == ((2, 2, 16, 3), torch.float64) and shapes['val'][0] == (2, 5) and shapes['best_epoch'] == ((2,), torch.int32)
    assert set(shapes) == set(ops.RNN_OUTPUTS)


def test_fit_population_argument_rules():
    from discrete_mean_field_game_amd import rnn
    days = R.dirichlet_days(6, 16, 3, 1)
    out = rnn.check_population_args(days, [4, 8], 1e-2, 10, [0, 1, 2], [[3], [4]], [[5], [4, 5]], 0, 0, 'adam', 1)
    assert out[9] == (2, 6, 16, 3, R.weight_count(8, 3), 10, 10) and out[2].tolist() == [1e-2, 1e-2] and out[3].tolist() == [10, 10]
    assert [t.tolist() for t in out[6]] == [[0, 1, 2]] * 2 and [t.tolist() for t in out[8]] == [[5], [4, 5]]
    for args in ((days[0], [4], 1e-2, 10, [0], None, None, 0, 0, 'adam', 1), (days, [], 1e-2, 10, [0], None, None, 0, 0, 'adam', 1),
                 (days, [4], 1e-2, 10, [6], None, None, 0, 0, 'adam', 1), (days, [4], 1e-2, 10, [], None, None, 0, 0, 'adam', 1),
                 (days, [4], 1e-2, 10, [0], [7], None, 0, 0, 'adam', 1), (days, [4], 1e-2, 10, [0], None, [-1], 0, 0, 'adam', 1),
                 (days, [4, 4], [1e-2] * 3, 10, [0], None, None, 0, 0, 'adam', 1), (days, [5], 1e-2, 10, [0], None, None, 0, 0, 'adam', 1),
                 (days, [4], 0.0, 10, [0], None, None, 0, 0, 'adam', 1), (days, [4], 1e-2, 0, [0], None, None, 0, 0, 'adam', 1),
                 (days, [4], 1e-2, 10, [0], None, None, -1.0, 0, 'adam', 1), (days, [4], 1e-2, 10, [0], None, None, 0, -1.0, 'adam', 1),
                 (days, [4], 1e-2, 10, [0], None, None, 0, 0, 'lbfgs', 1), (days, [4], 1e-2, 10, [0], None, None, 0, 0, 'adam', 0)):
        with pytest.raises(ValueError):
            rnn.check_population_args(*args)


def test_init_weights_and_unpack():
    from discrete_mean_field_game_amd import rnn
    w = rnn.init_weights(8, 3, 5)
    assert w.shape == (R.weight_count(8, 3),) and w.dtype == np.float64 and np.abs(w).max() <= 1 / np.sqrt(8)
    assert np.array_equal(w, rnn.init_weights(8, 3, 5)) and not np.array_equal(w, rnn.init_weights(8, 3, 6))
    assert np.array_equal(w, R.init_weights(8, 3, 5))
    parts = rnn.unpack(w, 8, 3)
    assert [parts[n].shape for n in ('Wx', 'Wh', 'b', 'Wo', 'bo')] == [(32, 3), (32, 8), (32,), (3, 8), (3,)]
    assert all(np.array_equal(parts[n], a) for n, a in zip(('Wx', 'Wh', 'b', 'Wo', 'bo'), R.unpack(w, 8, 3)))
    assert parts['Wh'][1, 2] == w[32 * 3 + 8 + 2] and parts['bo'][2] == w[-1]


def _fits(K=2, N=3, Hd=16, d=3):
    from discrete_mean_field_game_amd import rnn
    rs = np.random.RandomState(0)
    Wm = R.weight_count(8, d)
    out = {'weights': rs.rand(K, Wm), 'loss': rs.rand(K, 10), 'val': rs.rand(K, 5), 'best_epoch': np.array([4, 10], np.int32),
           'future': rs.dirichlet(np.ones(d), size=(K, N, Hd)), 'per_day': rs.rand(K, N, 4), 'metrics': rs.rand(K, 8),
           'status': np.zeros(K, np.int32)}
    return rnn.RnnFits(out, np.array([4, 8]), np.array([1e-2, 1e-3]), np.array([6, 10]), np.zeros(K), np.zeros(K), np.array([2, 0]),
                       np.array([2, 3]), Hd, d, 'adam', 2), out


def test_rnnfits_crops_and_traj_is_the_scorers_member_layout():
    fits, out = _fits()
    assert len(fits) == 2
    m = fits.model(0)
    assert m['Wx'].shape == (16, 3) and m['Wo'].shape == (3, 4) and m['loss'].shape == (6,) and m['val'].shape == (3,)
    assert m['future'].shape == (2, 16, 3) and m['per_day'].shape == (2, 4) and m['best_epoch'] == 4 and m['hidden'] == 4
    assert np.array_equal(m['bo'], out['weights'][0, R.weight_count(4, 3) - 3:R.weight_count(4, 3)])
    assert fits.model(1)['val'].shape == (0,) and fits.model(1)['Wh'].shape == (32, 8)
    t = fits.traj(0)
    assert t.shape == (2, 16, 3) and t.dtype == np.float32 and np.array_equal(t, out['future'][0, :2].astype(np.float32))
    assert fits.traj(1).shape == (3, 16, 3)


def test_the_trajectory_file_round_trips_and_read_rnn_reads_it(tmp_path):
    from discrete_mean_field_game_amd import rnn
    fits, out = _fits()
    path = str(tmp_path / 'trajectories_rnn.txt')
    assert rnn.write_trajectories(fits, 1, path) == 3 * 16
    back = rnn.read_trajectories(path)
    assert back.shape == (3, 16, 3) and back.dtype == np.float32 and np.array_equal(back, fits.traj(1))
    lines = open(path).read().splitlines()
    assert len(lines) == 48 and all(len(l.split(' ')) == 3 for l in lines)
    with pytest.raises(ValueError):
        rnn.read_trajectories(path, hours=7)
    pd = pytest.importorskip('pandas')
    df = pd.read_csv(path, sep=' ', header=None, names=range(3), usecols=range(3), dtype=np.float32)     # mfg_ac2.py:758
    assert df.shape == (48, 3) and np.array_equal(df.values.reshape(3, 16, 3), fits.traj(1))


def test_cross_validation_argument_rules_and_model_order(monkeypatch):
    from discrete_mean_field_game_amd import rnn
    days = R.dirichlet_days(6, 16, 3, 1)
    for args in ((days[0], [4], [1e-2]), (days, [], [1e-2]), (days, [4], []), (days, [4], [1e-2], 6), (days, [4], [1e-2], 0)):
        with pytest.raises(ValueError):
            rnn.cross_validation(*args)
    seen = {}

    def fake(days, hidden, lrs, epochs, train_days, val_days, test_days, **kw):
        seen.update(hidden=list(hidden), lrs=list(lrs), train=train_days, test=test_days)

        class F:
            metrics = np.arange(len(hidden) * 8, dtype=np.float64).reshape(-1, 8)
        return F()
    monkeypatch.setattr(rnn, 'fit_population', fake)
    cv = rnn.cross_validation(days, [4, 8], [1e-2, 1e-3, 1e-4], 2, 2, split_seed=5)
    assert seen['hidden'] == [4] * 6 + [8] * 6 and seen['lrs'] == [1e-2, 1e-2, 1e-3, 1e-3, 1e-4, 1e-4] * 2
    from discrete_mean_field_game_amd.var import var
    want = var.splits(6, 2, 12, np.random.RandomState(5))
    assert [list(s) for s in seen['train']] == [list(s) for s, _ in want] and seen['test'] == [r for _, r in want]
    assert cv['mean'].shape == (2, 3) and cv['mean'][0, 0] == (6 + 14) / 2 and cv['best'] == (4, 1e-2) and cv['std'][1, 2] == 4.0
