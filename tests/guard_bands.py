"""Guard bands round a tensor: a plain helper of the write-bounds tests (tests/test_gpu_write_bounds.py), not a conftest.

Guarded(shape, dtype, device) is ONE uint8 allocation of pad + offset + nbytes + pad bytes, every byte 0xA5, and `.t`, a view
of its interior with the requested shape and dtype.  A kernel that is handed `.t` and stores before its first or past its
last byte changes a band, and `.check(name)` says where.  The bands belong to the allocation of the interior, so such a store
(up to `pad` bytes away: 1 MiB, more than any tile or super-tile burst of this library) is recorded and cannot fault.

0xA5 repeated is finite and unmistakable in every type the library reads: -2.87e-16 as fp32, -1.2e-130 as fp64, -1515870811
as int32.  A masked lane that legally LOADS bytes next to an input is not disturbed by it.
"""
import numpy as np
import torch

PAD = 1 << 20
BYTE = 0xA5


class Guarded:
    """`.t`: the interior, `pad + offset` bytes into the allocation.  `pad` is a multiple of 256, so offset = 0 gives a
    16-byte-aligned interior and offset = 4 / 8 the misaligned forms.  The back band starts at the very byte where the interior
    ends (no rounding): a 16-byte store that straddles the end is seen.  fill: a number (NaN for outputs, 0 for a workspace
    that is zeroed once) or the data of an input (array or tensor of the interior's shape); None leaves the interior 0xA5."""

    def __init__(self, shape, dtype, device, pad=PAD, offset=0, fill=None):
        shape = (int(shape),) if isinstance(shape, (int, np.integer)) else tuple(int(s) for s in shape)
        item = torch.empty(0, dtype=dtype).element_size()
        if pad <= 0 or pad % 256 != 0:
            raise ValueError('pad must be a positive multiple of 256')
        if offset < 0 or offset % item != 0:
            raise ValueError('offset must be a non-negative multiple of the element size')
        self.shape, self.dtype, self.pad, self.offset = shape, dtype, int(pad), int(offset)
        self.nbytes = int(np.prod(shape, dtype=np.int64)) * item
        self.start = self.pad + self.offset                     # first byte of the interior
        self.end = self.start + self.nbytes                     # first byte of the back band
        self.raw = torch.full((self.end + self.pad,), BYTE, dtype=torch.uint8, device=device)
        assert self.raw.data_ptr() % 16 == 0, 'allocation is not 16-byte aligned'
        self.t = self.raw[self.start:self.end].view(dtype).view(shape)
        if fill is not None:
            if isinstance(fill, (int, float)):
                self.t.fill_(fill)
            else:
                src = fill if isinstance(fill, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(fill))
                if tuple(src.shape) != shape or src.dtype != dtype:
                    raise ValueError('fill: expected %s %s, got %s %s' % (shape, dtype, tuple(src.shape), src.dtype))
                self.t.copy_(src)

    def ptr(self):
        return self.t.data_ptr()

    def _changed(self, band):
        """(first, last) changed byte index of a band, or None."""
        bad = band != BYTE
        if not bool(bad.any()):
            return None
        idx = bad.nonzero()
        return int(idx[0]), int(idx[-1])

    def check(self, name):
        """Both bands are still all 0xA5; else AssertionError with the buffer's name, the band, and the first and last changed
        byte: in the front band as (negative) offsets from the interior's first byte, in the back band as offsets from the
        interior's end (0 = the byte right behind the last element)."""
        front = self._changed(self.raw[:self.start])
        if front is not None:
            raise AssertionError('%s: front band changed, bytes %d .. %d relative to the start of the interior (%d bytes, %s %s)'
                                 % (name, front[0] - self.start, front[1] - self.start, self.nbytes, self.dtype, self.shape))
        back = self._changed(self.raw[self.end:])
        if back is not None:
            raise AssertionError('%s: back band changed, bytes +%d .. +%d relative to the end of the interior (%d bytes, %s %s)'
                                 % (name, back[0], back[1], self.nbytes, self.dtype, self.shape))


def check_all(*guarded):
    """.check on several buffers: Guarded objects (named by position) or (name, Guarded) pairs; None entries are skipped."""
    for k, g in enumerate(guarded):
        if g is None:
            continue
        name, g = g if isinstance(g, tuple) else ('buffer %d' % k, g)
        if g is not None:
            g.check(name)
