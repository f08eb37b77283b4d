"""Host checks (no GPU) of the index arithmetic of the d <= 28 batch-sum kernel, restated in oracle/grad_index_ref.py, against
integer division.  `W` is the window s0 + j in [max(0, T - 64), T + 64) around the first trajectory boundary of a chunk; the
rules are monotone in s0 + j and a chunk holds 64 samples, so for T >= 64 nothing outside W can differ from inside it."""
import os

import numpy as np

from oracle import grad_index_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIRST_BAD_T = 6556022


def exact(sj, T):
    return np.asarray(sj, dtype=np.int64) // T


def wrong_on_window(T, rule):
    w = R.window(T)
    q = R.boundaries(w, T, rule)
    bad = np.nonzero(q != exact(w, T))[0]
    return [(T, int(w[i]), int(q[i])) for i in bad]


def test_parent_rule_is_exact_for_short_trajectories():
    """Every T in 1..4096 with every s0 < T, j < 64: s0 + j runs over [0, T + 63)."""
    for T in range(1, 4097):
        sj = np.arange(0, T + R.GS_CH - 1, dtype=np.int64)
        assert np.array_equal(R.boundaries(sj, T, 'parent'), exact(sj, T)), T
        for wide in (False, True):
            assert np.array_equal(R.boundaries(sj, T, 'fixed', wide), exact(sj, T)), (T, wide)


def test_parent_rule_is_exact_just_below_its_documented_limit():
    for k in range(32):
        T = 2 ** 22 - 64 - k
        assert wrong_on_window(T, 'parent') == [], T


def test_parent_rule_fails_first_at_6556022():
    """The finding: the parent rule puts the LAST step of a trajectory behind the boundary, (T, s0 + j, q) =
    (6 556 022, 6 556 021, 1) where integer division gives 0.  It is the first such T: for every smaller T >= 64 the values of
    s0 + j that decide a monotone rule, T - 1 (q = 0), T and the last of a chunk, T + 62 (q = 1), come out right -- so the
    multiply, which the 32-bit address form keeps, is exact for every T below LONG_T = 2^22 that the host gives it."""
    assert wrong_on_window(FIRST_BAD_T, 'parent') == [(FIRST_BAD_T, FIRST_BAD_T - 1, 1)]
    for lo in range(64, FIRST_BAD_T, 1 << 20):
        Ts = np.arange(lo, min(lo + (1 << 20), FIRST_BAD_T), dtype=np.int64)
        invT = np.float32(1.0) / Ts.astype(np.float32)
        q_last = (((Ts - 1).astype(np.float32) + np.float32(0.5)) * invT).astype(np.int64)
        q_first = ((Ts.astype(np.float32) + np.float32(0.5)) * invT).astype(np.int64)
        q_end = (((Ts + 62).astype(np.float32) + np.float32(0.5)) * invT).astype(np.int64)
        assert not q_last.any() and (q_first == 1).all() and (q_end == 1).all(), lo
    assert R.LONG_T == 2 ** 22 < FIRST_BAD_T
    # it goes on failing: every second T just above 2^23, and on both sides of 2^24
    above = [T for T in range(2 ** 23 + 1, 2 ** 23 + 41) if wrong_on_window(T, 'parent')]
    assert len(above) == 20
    assert wrong_on_window(2 ** 24 - 2, 'parent') and wrong_on_window(2 ** 24 + 1, 'parent') and wrong_on_window(8388610, 'parent')


def fixed_rule_cases():
    Ts = [FIRST_BAD_T, 2 ** 31 - 65]
    Ts += list(range(2 ** 23 - 300, 2 ** 23 + 301))
    Ts += list(range(2 ** 24 - 2, 2 ** 24 + 3))
    Ts += list(range(12000000, 12000301))
    return Ts


def test_fixed_rule_is_exact_for_long_trajectories():
    for T in fixed_rule_cases():
        assert R.host_picks_wide(T, 0)
        assert wrong_on_window(T, 'fixed') == [], T
        assert R.window(T)[-1] < 2 ** 31          # s0 + j fits the kernel's int
    assert max(fixed_rule_cases()) == R.T_MAX


def test_sample_of_element_is_exact_for_every_small_d():
    """The other fp32 division of the loader: flat element e of a chunk's [64][d] block -> sample e // d, d <= 28."""
    for d in range(1, R.GRAD_SMALL_MAX_D + 1):
        e = np.arange(0, 64 * R.GRAD_SMALL_MAX_D + 64, dtype=np.int64)      # every load slot of a lane, live or not
        assert np.array_equal(R.sample_of_element(e, d), e // d), d


def test_row_offsets_of_both_address_forms():
    """The fixed rule addresses row (n // T, n % T) in the 32-bit and in the wide form, ragged chunks and T < 64 included; the
    parent rule at the first bad T reads exactly one row too far, for the last step of each trajectory."""
    for (N, T, d, extra) in [(129, 3, 21, 21), (131, 1, 2, 4097), (195, 65, 17, 3), (192, 64, 28, 0), (72, 3, 21, (1 << 23) - 1),
                             (72, 3, 21, (1 << 23) + 5)]:
        stride_b = T * d + extra
        n = np.arange(N, dtype=np.int64)
        want = (n // T) * stride_b + (n % T) * d
        for wide in (None, False, True):
            if wide is False and extra >= R.WIDE_EXTRA:
                continue                              # (the 32-bit form cannot hold these offsets)
            assert np.array_equal(R.row_offsets(N, T, d, stride_b, 'fixed', wide), want), (N, T, d, extra, wide)
    T, d, B = FIRST_BAD_T, 2, 2
    stride_b = (T + 1) * d
    n = np.arange(B * T, dtype=np.int64)
    want = (n // T) * stride_b + (n % T) * d
    assert np.array_equal(R.row_offsets(B * T, T, d, stride_b, 'fixed'), want)
    got = R.row_offsets(B * T, T, d, stride_b, 'parent')
    bad = np.nonzero(got != want)[0]
    assert bad.tolist() == [T - 1, 2 * T - 1]
    assert np.array_equal(got[bad] - want[bad], [d, d])
    assert got.max() + d <= B * stride_b           # the parent's overshoot is the spare row: inside the allocation


def test_long_T_cases_of_the_gpu_test_stay_in_bounds_under_the_parent_rule():
    """tests/test_gpu_batch_sums_layouts.py runs T = 6 556 022, 8 388 610 (parent rule wrong) and 4 194 000 (still exact) at
    d = 2, B = 2, stride (T + 1) d: whatever rule the library under test was built with, no read leaves the B strides."""
    for T, n_bad in ((4194000, 0), (FIRST_BAD_T, 2), (8388610, 2)):
        d, B = 2, 2
        stride_b = (T + 1) * d
        n = np.arange(B * T, dtype=np.int64)
        want = (n // T) * stride_b + (n % T) * d
        got = R.row_offsets(B * T, T, d, stride_b, 'parent')
        assert int((got != want).sum()) == n_bad, T
        assert got.min() >= 0 and got.max() + d <= B * stride_b, T


def test_documented_limit_and_build_flags():
    """include/mfg_hip.h documents T <= 2^31 - 65 and the wide form from T >= 2^22 for d <= 28 (the refusal itself and the long
    trajectories run in tests/test_gpu_batch_sums_layouts.py), and the library is built without
    fast-math: 1.0f / (float)T is the correctly rounded quotient the restatement assumes."""
    hdr = open(os.path.join(ROOT, 'include', 'mfg_hip.h')).read()
    assert 'T <= 2^31 - 65' in hdr and R.T_MAX == 2 ** 31 - 65
    assert 'T >= 2^22' in hdr and R.LONG_T == 2 ** 22
    mk = open(os.path.join(ROOT, 'discrete_mean_field_game_amd', 'csrc', 'Makefile')).read()
    for flag in ('-ffast-math', '-Ofast', '-freciprocal-math', '-funsafe-math-optimizations',
                 '-fno-hip-fp32-correctly-rounded-divide-sqrt'):
        assert flag not in mk, flag
