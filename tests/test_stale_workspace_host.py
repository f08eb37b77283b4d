"""CPU: what the stale-workspace procedures (tests/stale_workspace.py) can see, and that the table's workspace contracts are
those of include/mfg_hip.h.

Detection power.  Procedures P and R run on CPU tensors against toy "entry points" written in torch: a writer leaves one partial
per four samples behind a 64-byte control block, a reader combines them.  The correct one passes everything; one that sums
`rows + 1` partials is reported by each of P's three fills and by R; one that takes fmax over an unwritten slot is MISSED by
0xFF (fmax drops a NaN) and by 0xFE and caught by 0x7F, its fmin mirror is caught by 0xFE alone: why there are three bytes.

Table against header.  Every entry point of the header with a `workspace` or `*scratch` parameter has a row that owns that work
buffer; a row declares no zero range exactly when the entry point's comment calls the contents scratch, the control block (of
every slice, for the population forms) otherwise; the row count of procedure P is the count derived here."""
import os
import re

import pytest

torch = pytest.importorskip('torch')

import stale_workspace as W
import stream_order as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = torch.device('cpu')


# ---------------------------------------------------------------------------------------------------- the toy entry points
def toy_bytes(N):
    """Control block + one fp64 partial per four samples, rounded up to 256 bytes (as the library rounds its slices)."""
    return (S.CONTROL_BYTES + 8 * -(-N // 4) + 255) // 256 * 256


def toy(kind, N):
    def build(a):
        x = a.randn64((N,), 1).abs_() + 0.1
        x = a.inp('x', -x if kind == 'fmin' else x)
        out = a.out('out', (1,), S.F64)
        ws = a.ws(toy_bytes(N), S.F64, zero=S.CONTROL)
        rows = -(-N // 4)

        def issue():
            part = ws[S.CONTROL_BYTES // 8:]
            padded = torch.zeros(4 * rows, dtype=S.F64)
            padded[:N] = x
            part[:rows] = padded.view(rows, 4).sum(1)                    # the writer: `rows` partials
            if kind == 'correct':
                out[0] = part[:rows].sum()
            elif kind == 'one_row_more':
                out[0] = part[:rows + 1].sum()                           # the reader: one more than was written
            else:
                m = part[0]
                for v in part[1:rows + 1]:                               # (an unwritten slot under a maximum / minimum)
                    m = torch.fmax(m, v) if kind == 'fmax' else torch.fmin(m, v)
                out[0] = m
        return issue
    return S.Row('toy-%s-N%d' % (kind, N), ('toy',), build, work=(('toy', 'workspace', S.CTL),))


def _caught(kind, fill):
    r = toy(kind, 10)
    return bool(W.poisoned(r, W.fresh(r, CPU), CPU, fill))


def _caught_by_leftovers(kind, small_first=False):
    big, small = toy(kind, 40), toy(kind, 10)                            # 10 partials, then 3: the small reader's 4th slot is stale
    if small_first:
        return bool(W.leftovers_small_first(big, small, W.fresh(big, CPU), W.fresh(small, CPU), CPU))
    return bool(W.leftovers([big, small, big], [W.fresh(big, CPU), W.fresh(small, CPU), W.fresh(big, CPU)], CPU))


def test_the_correct_toy_passes_everything():
    assert not any(_caught('correct', f) for f in W.FILLS)
    assert not _caught_by_leftovers('correct') and not _caught_by_leftovers('correct', small_first=True)


def test_a_reader_of_one_row_more_is_reported_by_every_fill_and_by_leftovers():
    assert all(_caught('one_row_more', f) for f in W.FILLS)
    assert _caught_by_leftovers('one_row_more')
    # (small -> big on a workspace zeroed once: the stale slot is still 0.0 -- the order that finds it is big -> small)
    assert not _caught_by_leftovers('one_row_more', small_first=True)


def test_why_three_bytes():
    assert [_caught('fmax', f) for f in (0xFF, 0x7F, 0xFE)] == [False, True, False]
    assert [_caught('fmin', f) for f in (0xFF, 0x7F, 0xFE)] == [False, False, True]


def test_the_fill_bytes_are_what_the_docstring_says():
    def as_(dtype, byte):
        return torch.full((8,), byte, dtype=torch.uint8).view(dtype)[0].item()
    assert as_(torch.float32, 0xFF) != as_(torch.float32, 0xFF) and as_(torch.float64, 0xFF) != as_(torch.float64, 0xFF)    # NaN
    assert as_(torch.int32, 0xFF) == -1
    assert 3.3e38 < as_(torch.float32, 0x7F) < 3.5e38 and 1.3e306 < as_(torch.float64, 0x7F) < 1.5e306 and as_(torch.int32, 0x7F) > 2 ** 30
    assert -1.8e38 < as_(torch.float32, 0xFE) < -1.6e38 and -6e303 < as_(torch.float64, 0xFE) < -4e303 and as_(torch.int32, 0xFE) < 0


def test_a_declared_range_left_dirty_and_a_store_into_a_band_are_reported():
    def dirty(a):
        ws = a.ws(256, S.F64, zero=S.CONTROL)
        out = a.out('out', (1,), S.F64)

        def issue():
            out[0] = 1.0
            ws[2] = 8.86                                                 # byte 16 of the control block
        return issue
    r = S.Row('toy-dirty', ('toy',), dirty, work=(('toy', 'workspace', S.CTL),))
    found = W.poisoned(r, {'out': torch.ones(1, dtype=S.F64)}, CPU, 0xFF)
    assert found and all('work[0] bytes [0, 64) not zero again' in f for f in found)

    def stray(a):
        ws = a.ws(256, S.F64, zero=S.CONTROL)
        out = a.out('out', (1,), S.F64)
        g = a.guarded[0] if a.guarded else None

        def issue():
            out[0] = 1.0
            if g is not None:
                g.raw[g.end + 3] = 0                                     # the 4th byte behind the workspace
        return issue
    r = S.Row('toy-stray', ('toy',), stray, work=(('toy', 'workspace', S.CTL),))
    found = W.poisoned(r, {'out': torch.ones(1, dtype=S.F64)}, CPU, 0x7F)
    assert found and all('back band changed, bytes +3 .. +3' in f for f in found)


def test_the_modes_of_bufs():
    a = S.Bufs(CPU, 0)
    assert not a.ws(256, S.F64, zero=S.CONTROL).any() and not a.guarded                    # plain: zeroed, as before
    b = S.Bufs(CPU, 0, fill=0x7F)
    t = b.ws(512, S.U8, zero=S.slices(2, 256))
    assert not t[:64].any() and not t[256:320].any() and (t[64:256] == 0x7F).all() and (t[320:] == 0x7F).all()
    assert b.guarded[0].nbytes == 512 and S.kind_of(b.zero[0], 512) == S.SLICES
    t[64:] = 3
    c = S.Bufs(CPU, 0, donor=b)
    u = c.ws(256, S.U8, zero=S.slices(2, 128))
    assert u.data_ptr() == t.data_ptr() and u.numel() == 256
    assert not u[:64].any() and (u[64:] == 3).all()                                        # donor mode touches nothing
    c.zero_new_ranges(b.zero)                                                              # the caller's side, and only that:
    assert not u[:64].any() and (u[64:128] == 3).all() and not u[128:192].any() and (u[192:] == 3).all()     # the new range
    with pytest.raises(AssertionError):
        S.Bufs(CPU, 0, donor=b).ws(1024)                                                   # the donor must be the larger one


# ---------------------------------------------------------------------------------------------------- the table against the header
NO_BYTES = ('mfg_row_distribution',)       # its workspace query returns 0 at present (the header says so): no buffer to own
BY_NAME = re.compile(r'^\w*scratch$')      # pi_scratch, scratch: scratch by their name


def _header():
    return open(os.path.join(ROOT, 'include', 'mfg_hip.h')).read()


def work_parameters(text):
    """(entry point, parameter) for every `workspace` / `*scratch` parameter of a function with an mfg_stream_t."""
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    found = []
    for name, params in re.findall(r'\b(mfg_[a-zA-Z0-9_]+)\s*\(([^;{}]*?)\)\s*;', text, flags=re.S):
        if re.search(r'\bmfg_stream_t\b', params):
            found += [(name, q) for q in re.findall(r'\*\s*(workspace|\w*scratch)\s*[,)]', params + ')')]
    return sorted(found)


def _comment_before(text, name):
    at = re.search(r'^int\s+%s\s*\(' % re.escape(name), text, flags=re.M).start()
    blocks = [m for m in re.finditer(r'/\*.*?\*/', text[:at], flags=re.S)]
    return re.sub(r'\s*\n\s*\*\s*', ' ', blocks[-1].group(0))


def block_scratch_members(text):
    """Work buffers that reach the library through a STRUCT bound to a context, not through a parameter: 'block.member' for every
    member that the comment in front of `typedef struct mfg_pop_<block>` lists as scratch (a line `member [shape type]  scratch`)."""
    found = []
    for m in re.finditer(r'typedef struct mfg_pop_(\w+)\s*\{', text):
        doc = [c for c in re.finditer(r'/\*.*?\*/', text[:m.start()], flags=re.S)][-1].group(0)
        found += ['%s.%s' % (m.group(1), q) for q in re.findall(r'^\s*\*\s+(\w+)(?:\s+\[[^\]]*\]\s+\w+)?\s+scratch\b', doc, flags=re.M)]
    return sorted(found)


def header_kind(text, entry, param, depth=0):
    """What the header's words say about a work buffer: scratch, the control block, or the control block of every slice."""
    if '.' in param:
        assert param in block_scratch_members(text), '%s: the header does not list it as scratch' % param
        return S.SCRATCH_KIND
    if BY_NAME.match(param):
        return S.SCRATCH_KIND
    doc = _comment_before(text, entry)
    if re.search(r'contents are scratch|and the workspace are scratch', doc):
        return S.SCRATCH_KIND
    if 'control block' in doc:
        return S.SLICES if re.search(r'\bslices\b', doc) else S.CTL
    ref = re.search(r'[Ww]orkspace as for (mfg_\w+)', doc)
    assert ref and depth < 3, '%s: the header says nothing about the contents of its workspace' % entry
    return header_kind(text, ref.group(1), param, depth + 1)


def test_the_header_is_read():
    params = work_parameters(_header())
    assert len(params) >= 39, params                              # (39 when this test was written)
    assert ('mfg_train_episode', 'pi_scratch') in params and ('mfg_train_episode', 'workspace') in params
    assert ('mfg_traj_log_z_pop', 'scratch') in params and not [q for q in params if q[0] == 'mfg_step_given_P']
    text = _header()
    assert header_kind(text, 'mfg_td_pg_accumulate', 'workspace') == S.CTL
    assert header_kind(text, 'mfg_grad_apply', 'workspace') == S.CTL                        # (through two "as for")
    assert header_kind(text, 'mfg_train_rollouts_irl_pop', 'workspace') == S.SLICES
    assert header_kind(text, 'mfg_train_episodes_pop_resident', 'workspace') == S.SCRATCH_KIND
    assert header_kind(text, 'mfg_evaluate_pop', 'workspace') == S.SCRATCH_KIND
    assert 'at present 0' in _comment_before(text, 'mfg_row_distribution')


def test_every_work_parameter_of_the_header_has_a_row_that_owns_it():
    params = [q for q in work_parameters(_header()) if q[0] not in S.NEEDS_COMM and q[0] not in NO_BYTES]
    owned = {(e, q) for r in S.ROWS for e, q, _ in r.work if '.' not in q}
    assert sorted(set(params) - owned) == []
    # (what a row owns beyond them: the device copy of the plan, a void* the header describes beside the workspace)
    assert sorted(owned - set(params)) == [('mfg_reward_net_train_steps_pop', 'plan_dev'), ('mfg_reward_net_train_steps_pop_z', 'plan_dev')]


def test_every_scratch_member_of_a_bound_block_has_a_row_that_owns_it():
    """The validation workspace and the evolve block's order / active arrays are handed over in a struct (mfg_ctx_set_pop_validate,
    mfg_ctx_set_pop_evolve): no parameter list shows them.  A new block with a scratch member and no row fails here."""
    members = block_scratch_members(_header())
    assert members == ['evolve.active', 'evolve.order', 'validate.workspace']
    owned = sorted({q for r in S.ROWS for _, q, _ in r.work if '.' in q})
    assert owned == members
    more = _header().replace('typedef struct mfg_pop_validate {', '/* Another block.\n *   tmp [K] fp64   scratch: a buffer\n */\n'
                             'typedef struct mfg_pop_other { double* tmp; } mfg_pop_other_t;\n'
                             '/* x */\ntypedef struct mfg_pop_validate_moved {')
    assert 'other.tmp' in block_scratch_members(more)


def test_a_row_declares_what_the_header_says():
    text = _header()
    for r in S.ROWS:
        for entry, param, kind in r.work:
            want = S.SCRATCH_KIND if param == 'plan_dev' else header_kind(text, entry, param)
            assert kind == want, '%s: %s of %s is declared %s, the header says %s' % (r.name, param, entry, kind, want)


def test_the_row_count_of_procedure_P():
    with_work = {e for e, _ in work_parameters(_header())} - set(NO_BYTES)
    rows = [r for r in S.ROWS if any(e in with_work for e in r.entries)]
    assert [r.name for r in rows] == [r.name for r in S.ROWS if r.work]
    assert len(rows) == W.N_WORK_ROWS


def test_a_new_entry_point_with_a_workspace_is_seen():
    more = _header().replace('#ifdef __cplusplus\n}', 'int mfg_new_thing(const float* x, void* workspace, size_t workspace_bytes,\n'
                             '    mfg_stream_t stream);\n#ifdef __cplusplus\n}')
    assert ('mfg_new_thing', 'workspace') in work_parameters(more)
