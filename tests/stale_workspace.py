"""Stale workspaces: the two procedures of tests/test_gpu_stale_workspace.py, on any device (tests/test_stale_workspace_host.py
runs them on CPU tensors against toy entry points to show what each one can and cannot see).

include/mfg_hip.h promises that a workspace is zeroed ONCE, that only its control block (the first 64 bytes; of every slice in
the population forms) has to be zero, that every call leaves it zero again, and that everything else -- the rest of such a
workspace, and every workspace or scratch buffer called scratch -- may hold anything.  tests/stream_order.py declares these
ranges row by row (Row.work, Bufs.ws(zero=)); here the rest of the buffer is made to hold something.

  poisoned(r, want, dev, fill)   procedure P: every byte outside the declared ranges is `fill`; the call runs twice in the same
                                 buffers (the second time only the outputs and the in/out buffers are put back).
  leftovers(seq, wants, dev)     procedure R: the rows of `seq` (big, small, big -- or small, big) run one after the other in ONE
                                 set of work buffers, the first one's, each with its own workspace_bytes; nothing is re-zeroed but
                                 a declared range that lay in the scratch part of the call before (a slice boundary).
Both return the list of findings (empty: passes): outputs that differ from the run on a fresh, fully zeroed workspace
(stream_order.reference), declared ranges that are not zero again, guard bands that changed.

The three fill bytes, each for a class of bug the other two miss:
  0xFF  NaN as fp32 and fp64, -1 as int32: an unwritten word that reaches a SUM.  fmin / fmax and comparisons hide it.
  0x7F  +3.4e38 / +1.4e306 / a large positive int: an unwritten word that reaches a MAXIMUM, a `<` test or a count.
  0xFE  -1.7e38 / -5e303 / a negative int: the same for a MINIMUM.
"""
import torch

import stream_order as S

FILLS = (0xFF, 0x7F, 0xFE)
N_WORK_ROWS = 47          # rows of stream_order.ROWS that own a work buffer: procedure P runs every one of them under every fill


def _sync(dev):
    if torch.device(dev).type == 'cuda':
        torch.cuda.synchronize()


def fresh(r, dev):
    """What the row leaves on a fresh, fully zeroed workspace: clones of every output and in/out buffer (the CPU counterpart of
    stream_order.reference(r, dev).want)."""
    a = S.Bufs(dev, 0)
    issue = r.build(a)
    _sync(dev)
    issue()
    _sync(dev)
    return {n: t.clone() for n, t in a.compared().items()}


def declared(a):
    """The kinds of the ranges a built Bufs declared, in the order of Row.work."""
    return [S.kind_of(z, t.numel() * t.element_size()) for t, z in zip(a.work, a.zero)]


def _after(a, want, what):
    found = ['%s: %s differs from the run on a fresh workspace' % (what, n) for n in S.differing(dict(a.compared()), want)]
    found += ['%s: %s not zero again' % (what, s) for s in a.stale_ranges()]
    try:
        a.check_bands()
    except AssertionError as e:
        found.append('%s: %s' % (what, e))
    return found


def _put_back(a, true):
    for n, t in a.inputs.items():
        t.copy_(true[n])
    a.refill()


def poisoned(r, want, dev, fill):
    """Procedure P."""
    a = S.Bufs(dev, 0, fill=fill)
    issue = r.build(a)
    true = {n: t.clone() for n, t in a.inputs.items()}
    found = []
    if declared(a) != [k for _, _, k in r.work]:
        found.append('the builder declares %s, Row.work %s' % (declared(a), [k for _, _, k in r.work]))
    for k in (1, 2):
        if k == 2:
            _put_back(a, true)
        _sync(dev)
        issue()
        _sync(dev)
        found += _after(a, want, 'fill 0x%02X, run %d' % (fill, k))
    return found


def leftovers(seq, wants, dev):
    """Procedure R.  seq: rows of one family; seq[0]'s builder sizes the buffers (it must be the largest).  wants[i]: what
    seq[i] leaves on a fresh workspace."""
    first = S.Bufs(dev, 0, fill=0)                   # guarded, fully zero: a workspace zeroed once
    built = {}
    found = []
    prev = None
    for i, r in enumerate(seq):
        if r.name in built:                          # (the big call once more, in its own buffers)
            a, issue, true = built[r.name]
            _put_back(a, true)
        else:
            a = first if i == 0 else S.Bufs(dev, 0, donor=first)
            issue = r.build(a)
            built[r.name] = (a, issue, {n: t.clone() for n, t in a.inputs.items()})
        if prev is not None:
            a.zero_new_ranges(prev.zero)
        _sync(dev)
        issue()
        _sync(dev)
        found += _after(a, wants[i], 'call %d (%s)' % (i, r.name))
        try:
            first.check_bands()
        except AssertionError as e:
            found.append('call %d (%s): %s' % (i, r.name, e))
        prev = a
    return found


def leftovers_small_first(big, small, want_big, want_small, dev):
    """Procedure R in the order small -> big: the buffers are the big call's (built first, not run)."""
    first = S.Bufs(dev, 0, fill=0)
    issue_big = big.build(first)
    b = S.Bufs(dev, 0, donor=first)
    issue_small = small.build(b)
    b.zero_new_ranges(first.zero)
    _sync(dev)
    issue_small()
    _sync(dev)
    found = _after(b, want_small, 'small first (%s)' % small.name)
    first.zero_new_ranges(b.zero)
    issue_big()
    _sync(dev)
    return found + _after(first, want_big, 'then big (%s)' % big.name)
