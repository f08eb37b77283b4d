"""NumPy float32 restatement of the sample -> (trajectory, step) index arithmetic of the d <= 28 batch-sum kernel
(grad_chunk_load, csrc/mfg_grad.h).

A wave of k_grad_mfma_small takes a chunk of GS_CH = 64 consecutive samples.  The chunk starts at sample n0 = 64 c, i.e. at
step s0 = n0 % T of trajectory b0 = n0 // T, and sample n0 + j (j < 64) lies q = (s0 + j) // T trajectory boundaries
further on.  The kernel does not divide:

* ``parent`` rule (every T, until this restatement found it wrong): ``q = (int)(((float)(s0 + j) + 0.5f) * (1.0f / (float)T))``.
  Exact for every T < 2^22; from T = 6 556 022 on the rounded reciprocal times T - 1/2 reaches 1.0f and the LAST step of a
  trajectory is placed behind the boundary (q = 1): the kernel then reads state row T of the trajectory, which in a
  pi_traj layout is the spare T+1-th state, instead of row T - 1.
* ``fixed`` rule: the 32-bit address form keeps the multiply and the host gives it only T < LONG_T = 2^22; longer trajectories
  (and skipped parts of 2^23 floats or more, as before) go to the wide form, which counts with an integer compare when
  T >= 64 -- a chunk then crosses at most one boundary, ``q = (s0 + j >= T)`` -- and with the multiply below (s0 + j < 127).
  The host accepts T <= T_MAX = 2^31 - 65, so that s0 + j fits a 32-bit int.

Every float32 operation here is one correctly rounded IEEE operation, as in the kernel (the library is built without fast-math,
and (x + 0.5f) * y is not a contractable pattern).
"""
import numpy as np

GS_CH = 64                      # samples per chunk (mfg_grad.h)
GRAD_SMALL_MAX_D = 28           # MFG_GRAD_SMALL_MAX_D
T_MAX = 2 ** 31 - 1 - GS_CH     # largest T mfg_grad_accumulate serves for d <= 28 (include/mfg_hip.h)
WIDE_EXTRA = 1 << 23            # skipped floats per trajectory from which the host picks the 64-bit (WIDE) address form
LONG_T = 1 << 22                # MFG_GRAD_LONG_T: trajectory length from which it picks that form as well

_f32 = np.float32


def _mul_rule(sj, T):
    sj = np.asarray(sj, dtype=np.int64)
    invT = _f32(1.0) / _f32(T)
    # (float)sj: int32 -> float32, round to nearest even, as v_cvt_f32_i32
    return ((sj.astype(np.float32) + _f32(0.5)) * invT).astype(np.int64)


def host_picks_wide(T, extra):
    return extra >= WIDE_EXTRA or T >= LONG_T


def boundaries(sj, T, rule='fixed', wide=None):
    """q for the steps-from-chunk-start `sj` = s0 + j (array), trajectory length T, by the kernel's arithmetic: the parent's
    rule, or the fixed one in the address form `wide` (None: the form the host picks for a skipped part below 2^23 floats)."""
    if rule == 'parent':
        return _mul_rule(sj, T)
    if rule != 'fixed':
        raise ValueError(rule)
    if wide is None:
        wide = host_picks_wide(T, 0)
    if not wide and T >= LONG_T:
        raise ValueError('the 32-bit form is never given T >= 2^22')
    if wide and T >= GS_CH:
        return (np.asarray(sj, dtype=np.int64) >= T).astype(np.int64)
    return _mul_rule(sj, T)


def sample_of_element(e, d):
    """Sample j of flat element e of a chunk's [64][d] block: (int)(((float)e + 0.5f) * (1.0f / (float)d))."""
    e = np.asarray(e, dtype=np.int64)
    return ((e.astype(np.float32) + _f32(0.5)) * (_f32(1.0) / _f32(d))).astype(np.int64)


def window(T):
    """The values of s0 + j around the first boundary: [max(0, T - 64), T + 64)."""
    return np.arange(max(0, T - GS_CH), T + GS_CH, dtype=np.int64)


def row_offsets(N, T, d, stride_b, rule='fixed', wide=None):
    """Float offset (from `pi`) of the state row the kernel reads for each sample n < N, by the address form the host picks
    (wide=None) or a given one.  The exact answer is (n // T) * stride_b + (n % T) * d."""
    n = np.arange(N, dtype=np.int64)
    n0 = (n // GS_CH) * GS_CH
    b0, s0 = n0 // T, n0 % T
    sj = s0 + (n - n0)
    extra = stride_b - T * d
    if wide is None:
        wide = host_picks_wide(T, extra) if rule == 'fixed' else extra >= WIDE_EXTRA
    q = boundaries(sj, T, rule, wide)
    if wide:
        return (b0 + q) * stride_b + (sj - q * T) * d
    return b0 * stride_b + s0 * d + (n - n0) * d + q * extra
