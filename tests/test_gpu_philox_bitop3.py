"""-m gpu: the Philox4x32-10 rounds of the device (csrc/mfg_device.h, xor3: one three-input bit operation per `hi ^ counter word
^ round key`) against oracle/philox_ref on words chosen to exercise every operand of the fused xor, bit for bit.

k_philox_raw (ops.philox_raw) takes the first counter word as `first + e`, the other three counter words and the 64-bit key as
launch arguments: every case below is one small launch.  Words: zero, all ones and the 32 single-bit words in each of the four
counter positions and both key halves, over an all-zero, an all-ones and a mixed background; then a few thousand random
counters and keys.
"""
import numpy as np
import pytest

torch = pytest.importorskip('torch')

pytestmark = pytest.mark.gpu

SPECIAL = [0x00000000, 0xFFFFFFFF] + [1 << b for b in range(32)]
BACKGROUNDS = [(0, 0, 0, 0, 0, 0), (0xFFFFFFFF,) * 6,
               (0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344, 0xA4093822, 0x299F31D0)]
PER_LAUNCH = 3   # consecutive first-counter words per case: a case at 0xFFFFFFFF also wraps to 0 and 1


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.fail('-m gpu tests need a GPU: the HIP path has no CPU fallback')
    return torch.device('cuda:0')


def run_cases(cases, n, dev):
    """cases: (c0, c1, c2, c3, k0, k1) words.  Device words and oracle words of n consecutive c0 per case, (len(cases) * n, 4)."""
    from discrete_mean_field_game_amd import ops
    from oracle.philox_ref import philox4x32_10
    outs, refs = [], []
    for c0, c1, c2, c3, k0, k1 in cases:
        outs.append(ops.philox_raw(k0 | (k1 << 32), c0, c1, c2, c3, n, dev))
        ctr = (c0 + np.arange(n, dtype=np.uint64)) & np.uint64(0xFFFFFFFF)
        refs.append(np.stack(philox4x32_10(ctr, c1, c2, c3, k0, k1), axis=1))
    torch.cuda.synchronize()
    return torch.cat(outs).cpu().numpy().view(np.uint32), np.concatenate(refs)


@pytest.mark.parametrize('position', range(6), ids=['c0', 'c1', 'c2', 'c3', 'k0', 'k1'])
def test_special_words_in_every_operand(dev, position):
    cases = []
    for bg in BACKGROUNDS:
        for word in SPECIAL:
            c = list(bg)
            c[position] = word
            cases.append(tuple(c))
    out, ref = run_cases(cases, PER_LAUNCH, dev)
    assert out.shape == ref.shape == (len(cases) * PER_LAUNCH, 4)
    assert np.array_equal(out, ref)


def test_random_counters_and_keys(dev):
    rs = np.random.RandomState(20240607)
    words = rs.randint(0, 2 ** 32, size=(1024, 6), dtype=np.uint64)
    out, ref = run_cases([tuple(int(w) for w in row) for row in words], 4, dev)
    assert out.shape == ref.shape == (4096, 4)
    assert np.array_equal(out, ref)


def test_long_run_of_one_launch(dev):
    """One launch over 2^16 consecutive first-counter words crossing the 32-bit wrap (grid-stride path of the kernel)."""
    out, ref = run_cases([(0xFFFF8000, 0xFFFFFFFF, 0, 0x80000000, 0x00000001, 0xFFFFFFFE)], 1 << 16, dev)
    assert np.array_equal(out, ref)
