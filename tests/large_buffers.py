"""Operands past 2^31 elements and 8 GiB: a plain helper of tests/test_gpu_large_buffers.py, not a conftest.

Every other test of the suite stays below 2^29 floats (the signed 2 GiB byte offset).  The cases built on this helper hand
one entry point an operand of a little more than 2^31 fp32 elements, so that the 2 GiB, 4 GiB and 8 GiB byte offsets (float
offsets 2^29, 2^30, 2^31) all lie inside it, with many tiles and super tiles wholly past the last of them:

  SLAB_FLOATS            2^31 + 2^25 floats (8.72 GB): one allocation, made once per module and viewed per case.
  batch_for              the item count of a case: fills the slab, ragged against the kernel's tile.
  boundary_windows       five index ranges (first, last, and round the items that hold float offsets 2^29, 2^30, 2^31) that
                         are compared with the fp64 / NumPy reference of the operation.
  chunks                 unequal ranges of < 2^28 floats that tile the batch: the same entry point is called on each of them
                         (the address range the rest of the suite covers) and must give the bits of the whole-batch call.
  fill_rows_             deterministic row-stochastic contents, written chunk by chunk on the device.
  require_free           fails (never skips) when the device cannot hold a case.

Memory budget.  Groups A-C of the test module hold the slab (8.72 GB) and small outputs.  Group D holds two slabs, or one
slab and one fp64 output of about 17.2 GB.  No test keeps more than 18 GiB live beyond the slab; every test frees its second
buffer and empties torch's cache before it returns.  One MI355X has 288 GB.
"""
SLAB_FLOATS = 2 ** 31 + 2 ** 25
MARGIN_FLOATS = 2 ** 31 + 2 ** 24            # a case's operand is larger than this: tiles / super tiles wholly past 2^31
BOUNDARIES = (2 ** 29, 2 ** 30, 2 ** 31)     # float offsets of the 2 GiB, 4 GiB and 8 GiB byte offsets
CHUNK_FLOATS = 2 ** 28                       # every chunk is smaller (1 GiB of fp32)
TAIL_FLOATS = 2 ** 22                        # the last chunk is no larger: it starts behind the window round 2^31
MIN_WINDOW_ELEMENTS = 250_000               # the five windows together: the floor of test_gpu_sampler_elementwise._batch


def batch_for(per_item_floats, tile=1):
    """The largest B with B * per_item_floats <= SLAB_FLOATS that is not a multiple of `tile` (the items the kernel under test
    takes together: 12 trajectories at d = 21, say), so the last tile is ragged.  tile = 1: no such constraint."""
    per_item_floats, tile = int(per_item_floats), int(tile)
    if per_item_floats < 1 or tile < 1:
        raise ValueError('per_item_floats and tile must be positive')
    B = SLAB_FLOATS // per_item_floats
    while tile > 1 and B % tile == 0:
        B -= 1
    if B * per_item_floats <= MARGIN_FLOATS:
        raise ValueError('items of %d floats leave no batch in (2^31 + 2^24, 2^31 + 2^25]' % per_item_floats)
    return B


def window_items(per_item_floats):
    """W: the smallest item count with 5 W per_item_floats >= MIN_WINDOW_ELEMENTS."""
    return max(1, -(-MIN_WINDOW_ELEMENTS // (5 * int(per_item_floats))))


def boundary_windows(B, per_item_floats, W):
    """Five ranges of W consecutive items, in increasing order: the first W, W centred on the item that contains float offset
    2^29, 2^30 and 2^31, and the last W."""
    B, per_item_floats, W = int(B), int(per_item_floats), int(W)
    out = [range(0, W)]
    for off in BOUNDARIES:
        item = off // per_item_floats
        lo = item - W // 2
        out.append(range(lo, lo + W))
    out.append(range(B - W, B))
    for a, b in zip(out[:-1], out[1:]):
        if not (0 <= a.start and a.stop <= b.start and b.stop <= B):
            raise ValueError('windows of %d items overlap or leave [0, %d)' % (W, B))
    return out


def window_index(windows):
    """The items of all windows as one int64 array (NumPy)."""
    import numpy as np
    return np.concatenate([np.arange(w.start, w.stop, dtype=np.int64) for w in windows])


_FRACTIONS = (0.97, 0.53, 0.81, 0.37, 0.68)  # of the largest chunk: sizes are unequal on purpose


def chunks(B, per_item_floats, align=4):
    """Consecutive (lo, hi) ranges that tile [0, B) once.  Every chunk holds fewer than 2^28 floats; every lo is a multiple of
    `align` items (align = 4: lo * per_item_floats * 4 bytes is a multiple of 16, so a chunk call takes the kernels of an
    aligned operand); the sizes cycle through unequal fractions of the largest one, and the last chunk holds at most
    TAIL_FLOATS: a chunk boundary lies behind the window round 2^31 and in front of the last window."""
    B, per_item_floats, align = int(B), int(per_item_floats), int(align)
    most = (CHUNK_FLOATS - 1) // per_item_floats // align * align
    if most < align:
        raise ValueError('an item of %d floats does not fit a chunk' % per_item_floats)
    out, lo, k = [], 0, 0
    while lo < B:
        n = max(align, int(most * _FRACTIONS[k % len(_FRACTIONS)]) // align * align)
        hi = min(B, lo + n)
        out.append((lo, hi))
        lo, k = hi, k + 1
    lo, hi = out[-1]
    cut = (B - TAIL_FLOATS // per_item_floats) // align * align
    if lo < cut < hi:
        out[-1:] = [(lo, cut), (cut, hi)]
    return out


def fill_rows_(slab_view, d, seed, chunk_floats=2 ** 26):
    """Row-stochastic rows of d floats over the whole flat fp32 view, on its device: (uniform + 1e-3) / row sum, from a
    generator seeded with `seed` -- deterministic, so any part can be produced again.  Written `chunk_floats` at a time: the
    temporaries stay far below 1 GiB."""
    import torch
    n = slab_view.numel()
    if slab_view.dim() != 1 or n % d != 0:
        raise ValueError('fill_rows_ takes a flat view of whole rows')
    g = torch.Generator(device=slab_view.device)
    g.manual_seed(int(seed))
    step = max(1, int(chunk_floats) // d) * d
    for lo in range(0, n, step):
        part = slab_view[lo:min(n, lo + step)].view(-1, d)
        part.uniform_(0.0, 1.0, generator=g)
        part.add_(1e-3)
        part.div_(part.sum(1, keepdim=True))
    return slab_view


def require_free(nbytes):
    """pytest.fail (not skip: a skip would hide what the module is for) unless the device has `nbytes` free."""
    import pytest
    import torch
    free, total = torch.cuda.mem_get_info()
    free += torch.cuda.memory_reserved() - torch.cuda.memory_allocated()     # torch's own cache can be reused
    if free < nbytes:
        pytest.fail('the case needs %d bytes of device memory, %d are free (of %d)' % (nbytes, free, total))
