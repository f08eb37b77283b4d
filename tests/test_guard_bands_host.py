"""No GPU: tests/guard_bands.py on CPU tensors.  This is where the helper of the write-bounds tests is shown to be able to
fail: a byte changed just before the interior, just behind it, or at the far end of the back band is found and named."""
import re

import pytest

torch = pytest.importorskip('torch')

from guard_bands import BYTE, PAD, Guarded, check_all

CPU = torch.device('cpu')


@pytest.mark.parametrize('offset', [0, 4, 8])
@pytest.mark.parametrize('dtype,shape', [(torch.float32, (5, 21)), (torch.float32, (3,)), (torch.int32, (7,)),
                                          (torch.float64, (1,)), (torch.int64, (2, 3))])
def test_interior_view(dtype, shape, offset):
    item = torch.empty(0, dtype=dtype).element_size()
    if offset % item != 0:
        with pytest.raises(ValueError):
            Guarded(shape, dtype, CPU, offset=offset)
        return
    g = Guarded(shape, dtype, CPU, offset=offset)
    n = item
    for s in shape:
        n *= s
    assert tuple(g.t.shape) == shape and g.t.dtype == dtype and g.t.is_contiguous()
    assert g.raw.dtype == torch.uint8 and g.raw.numel() == PAD + offset + n + PAD
    assert bool((g.raw == BYTE).all())
    assert g.t.data_ptr() == g.raw.data_ptr() + PAD + offset
    assert g.t.data_ptr() % 16 == offset % 16
    # the back band starts at the very byte where the interior ends
    assert g.end == PAD + offset + n and g.raw.numel() - g.end == PAD
    g.check('untouched')


def test_the_pattern_is_finite_in_every_type():
    for dtype in (torch.float32, torch.float64):
        g = Guarded((4,), dtype, CPU)
        assert bool(torch.isfinite(g.t).all()) and bool((g.t != 0).all())
    assert int(Guarded((1,), torch.int32, CPU).t[0]) == -1515870811


def test_fill_and_interior_writes_pass():
    g = Guarded((3, 5), torch.float32, CPU, offset=4, fill=float('nan'))
    assert bool(torch.isnan(g.t).all())
    g.t.copy_(torch.arange(15, dtype=torch.float32).view(3, 5))
    g.t[2, 4] = -1.0
    g.check('written inside')
    data = torch.arange(6, dtype=torch.float64).view(2, 3)
    h = Guarded((2, 3), torch.float64, CPU, fill=data)
    assert torch.equal(h.t, data)
    z = Guarded((8,), torch.uint8, CPU, fill=0)
    assert int(z.t.sum()) == 0
    check_all(g, ('h', h), None, ('z', z), ('absent', None))
    with pytest.raises(ValueError):
        Guarded((2, 3), torch.float64, CPU, fill=data.float())


def _fails(g, name):
    with pytest.raises(AssertionError) as e:
        g.check(name)
    return str(e.value)


@pytest.mark.parametrize('offset', [0, 4])
def test_a_byte_just_before_the_interior_is_found(offset):
    g = Guarded((5,), torch.float32, CPU, offset=offset, fill=0.0)
    g.raw[PAD + offset - 1] = 0
    msg = _fails(g, 'pi_next')
    assert 'pi_next' in msg and 'front band' in msg
    assert re.search(r'bytes -1 \.\. -1 ', msg), msg


def test_a_byte_just_after_the_interior_is_found():
    g = Guarded((5,), torch.float32, CPU, offset=4, fill=0.0)
    g.raw[PAD + 4 + 20] = 0xA4
    msg = _fails(g, 'reward')
    assert 'reward' in msg and 'back band' in msg
    assert re.search(r'bytes \+0 \.\. \+0 ', msg), msg
    with pytest.raises(AssertionError):
        check_all(('reward', g))


def test_the_last_byte_of_the_back_band_is_found():
    g = Guarded((1,), torch.float64, CPU, fill=0.0)
    g.raw[-1] = 0
    msg = _fails(g, 'theta')
    assert 'theta' in msg and 'back band' in msg
    assert re.search(r'bytes \+%d \.\. \+%d ' % (PAD - 1, PAD - 1), msg), msg


def test_first_and_last_changed_byte_of_a_range():
    """A 16-byte store that straddles the end of a 5-float interior: 12 bytes land in the band."""
    g = Guarded((5,), torch.float32, CPU, fill=0.0)
    g.raw[g.end - 4:g.end + 12] = 0
    msg = _fails(g, 'out')
    assert re.search(r'bytes \+0 \.\. \+11 ', msg), msg
    f = Guarded((5,), torch.float32, CPU, fill=0.0)
    f.raw[0] = 1
    f.raw[f.start - 3] = 1
    msg = _fails(f, 'out')
    assert re.search(r'bytes -%d \.\. -3 ' % PAD, msg), msg
