"""Networks, inputs and the shape / regime grid of the reward network's FORWARD kernels off the matrix-core path.  TEST
INFRASTRUCTURE shared by tests/test_reward_forward_cases.py (CPU: the admission rule of this table) and
tests/test_gpu_reward_net_forward_paths.py (GPU).  Everything here runs on CPU tensors too.

reward_net_forward_sums (csrc/mfg_reward_net.hip) picks one of four kernels; `kernel_of` restates its rule:
  mfma        the matrix-core kernel: d = 21 / 15, (k1, f2, k2) = (5, 2, 3), n3 <= 16, fc3.weight 8-byte aligned
  runs        k_reward_net_runs: d = 21 / 15 at (5, 2, 3), n3 > 16 or the matrix-core kernel refused
  generic-ct  k_reward_net<PP, 5, 3, 2, 0>: (5, 2, 3) at any other d, or a 4-byte aligned fc3.weight
  generic-rt  k_reward_net<PP, 0, 0, 0, 0>: any other (k1, f2, k2)
and `stages` its rule for copying the FC3 weights into LDS (runs / generic only): at least MFG_RN_LDS_MIN = 16 samples per
block -- the grid is capped at 256 MFG_RN_BPC = 512 blocks of MFG_RN_WAVES = 8 waves, so B >= 7 681 --, the weights no more
than 64 KB, 16-byte aligned, and the launch's whole LDS request within what one block may have (RN_LDS_LIMIT).

Families (the smallest shapes that reach each path):
  generic    run-time conv geometry at the PP boundaries d = 16 | 17, 21 | 22, at 8 | 9 (one pass | one lane into the second), at
             d = 1, 2 (the image smaller than every conv kernel) and at the widest / narrowest dense layers
  ref        the reference's geometry through the pixel-per-lane kernel at the same d; at d = 21 / 15 a 4-byte offset of
             fc3.weight (-> generic-ct) and an 8-byte one (-> mfma with its pieces on an address = 8 mod 16)
  runs       d = 21 / 15 at n3 = 17, 24, 32, n4 = 1, 8, 32 (nin = n3 + d = 53 lanes of FC4 input at the widest), and the
             8-byte offset (float2 reads from global memory on an address = 8 mod 16)
  staged     B = 7 681 / 8 197: the float4 copy loop, its scalar tail (17 x 450 and 75 floats are no multiples of 4), the LDS
             float2 reads; n3 = 18 is the last run-mapped n3 under 64 KB of weights, n3 = 19 the control that must not stage;
             the three d = 32 shapes are the family's largest LDS requests (149 600, 159 264 and -- refused by `stages` --
             163 968 B)
  regime     out.weight x gain in {1e-3, 1, 8, 30} and Dirichlet concentration in {1, 0.02} (near one-hot rows; the 0.02 cases
             carry exact zeros and exactly one-hot rows), one shape per kernel

A case is ADMITTED when a plain fp32 evaluation of the network stays within HALF of the GPU test's tolerance of the fp64 oracle
(cpu_ratio <= 0.5): a case whose reference alone leaves the bound proves nothing on the device.  The fp32 evaluation is
`f32_forward`: every sum term by term in index order in NumPy element-wise float32 arithmetic, the same bits on every machine.
networks.RewardNet in fp32 is measured next to it (`torch_ratio`, printed by the CPU test) and not asserted: its ratio depends on
the CPU's vector width and thread count through PyTorch's summation order -- one case gave 0.31 on one machine and 0.64 on
another --, and an admission rule must not.  A dropout network is two networks to the device -- dropout off, and under the
masks of dropout_key(case), which remove units and scale the others by 2.5 -- and is admitted on both: the tolerance's scale m
sees the cancellation in front of the output unit but not the one in front of FC4, and a mask can leave exactly such a sample
(seed 0 of regime-ct-d15-gain8-conc1: 0.06 with dropout off, 1.37 under its masks with networks.RewardNet, 4.33 on the device).
`python -m oracle.reward_forward_cases` walks the network seed upwards from 0 until both hold and prints the _SEEDS table below.
Staged cases are compared on their oracle subsample only (`oracle_indices`)."""
from collections import namedtuple

import numpy as np
import torch

from oracle import reward_net_oracle as RO
from oracle.reward_train_cases import _net

Case = namedtuple('Case', 'name family d k1 f2 k2 n3 n4 reg gain conc B seed w3_offset n_oracle')

RN_WAVES, RN_BPC, RN_LDS_MIN = 8, 2, 16                      # MFG_RN_WAVES, MFG_RN_BPC, MFG_RN_LDS_MIN
STAGE_B = 256 * RN_BPC * (RN_LDS_MIN - 1) + 1                # 7 681: the first batch with 16 samples in one of the 512 blocks
RN_LDS_LIMIT = 160 * 1024                                    # LDS of one CU of gfx950
GAINS = (1e-3, 1.0, 8.0, 30.0)
CONCS = (1.0, 0.02)
REF = (5, 2, 3)
TOL_REL = 1e-5                                               # x max(|r_ref|, m), m = |h4| . |out_w| + |out_b|
TOL_ABS = {False: 2e-6, True: 5e-6}                          # gain 1, conc 1: the existing forward tests' bounds (dropout off / on)

# (d, k1, f2, k2, n3, n4)
_GENERIC = [(1, 7, 2, 7, 3, 2), (2, 7, 1, 1, 3, 2), (8, 3, 1, 5, 5, 3), (9, 3, 1, 5, 5, 3), (16, 1, 2, 1, 6, 4), (17, 3, 2, 5, 8, 4),
            (21, 7, 2, 7, 8, 4), (22, 5, 1, 3, 4, 4), (32, 7, 2, 7, 32, 32), (15, 1, 1, 1, 32, 1), (12, 5, 2, 5, 1, 32)]
_REF_D = (1, 2, 8, 9, 16, 17, 22, 32)
_RUNS_N = [(17, 1), (24, 8), (32, 32), (17, 32), (32, 1)]
# (tag, d, (k1, f2, k2), n3, n4, batches)
_STAGED = [('runs15-tail', 15, REF, 17, 4, (7681, 8197)),
           ('runs21-last', 21, REF, 18, 32, (7681, 8197)),
           ('runs21-control', 21, REF, 19, 4, (7681, 8197)),
           ('rt5-tail', 5, (3, 1, 5), 3, 2, (7681, 8197)),
           ('ct4', 4, REF, 3, 2, (7681, 8197)),
           ('ct32', 32, REF, 8, 32, (7681,)),
           ('rt32', 32, (7, 2, 7), 8, 4, (7681,)),
           ('rt32-corner', 32, (7, 2, 7), 8, 32, (7681,))]
# (tag, d, (k1, f2, k2), n3, n4, fc3 byte offset)
_REGIME = [('runs', 21, REF, 24, 4, 0), ('ct', 15, REF, 8, 4, 4), ('rt', 9, (3, 1, 5), 5, 3, 0), ('mfma', 21, REF, 8, 4, 0)]

# network seeds, keyed by case name: (the first seed >= 0 whose f32_forward stays within half the tolerance, its ratio with dropout
# off, its ratio under the case's masks).  Fifteen cases left seed 0, among them regime-ct-d15-gain8-conc1-dropout_l1l2, where the
# device gave 4.33 under the masks at seed 0 and networks.RewardNet itself 1.37.
_SEEDS = {
    'generic-d1-k727-n3x2-none': (0, 0.014, None),
    'generic-d2-k711-n3x2-dropout_l1l2': (0, 0.075, 0.050),
    'generic-d8-k315-n5x3-none': (0, 0.021, None),
    'generic-d9-k315-n5x3-dropout_l1l2': (0, 0.038, 0.056),
    'generic-d16-k121-n6x4-none': (0, 0.031, None),
    'generic-d17-k325-n8x4-dropout_l1l2': (1, 0.069, 0.171),
    'generic-d21-k727-n8x4-none': (0, 0.072, None),
    'generic-d22-k513-n4x4-dropout_l1l2': (0, 0.010, 0.014),
    'generic-d32-k727-n32x32-none': (0, 0.009, None),
    'generic-d15-k111-n32x1-dropout_l1l2': (0, 0.032, 0.060),
    'generic-d12-k525-n1x32-none': (0, 0.016, None),
    'ref-d1-none': (0, 0.006, None),
    'ref-d2-dropout_l1l2': (0, 0.022, 0.022),
    'ref-d8-none': (0, 0.042, None),
    'ref-d9-dropout_l1l2': (0, 0.027, 0.029),
    'ref-d16-none': (0, 0.014, None),
    'ref-d17-dropout_l1l2': (0, 0.016, 0.025),
    'ref-d22-none': (0, 0.098, None),
    'ref-d32-dropout_l1l2': (0, 0.023, 0.452),
    'ref-d21-off4-none': (0, 0.029, None),
    'ref-d21-off8-dropout_l1l2': (0, 0.029, 0.128),
    'ref-d15-off4-dropout_l1l2': (0, 0.071, 0.221),
    'ref-d15-off8-none': (0, 0.071, None),
    'runs-d21-n17x1-none': (0, 0.168, None),
    'runs-d21-n24x8-dropout_l1l2': (0, 0.181, 0.481),
    'runs-d21-n32x32-none': (0, 0.040, None),
    'runs-d21-n17x32-dropout_l1l2': (0, 0.030, 0.019),
    'runs-d21-n32x1-none': (0, 0.023, None),
    'runs-d15-n17x1-dropout_l1l2': (1, 0.310, 0.143),
    'runs-d15-n24x8-none': (0, 0.075, None),
    'runs-d15-n32x32-dropout_l1l2': (0, 0.038, 0.060),
    'runs-d15-n17x32-none': (0, 0.022, None),
    'runs-d15-n32x1-dropout_l1l2': (0, 0.005, 0.008),
    'runs-d21-n24x8-off8-dropout_l1l2': (0, 0.181, 0.285),
    'runs-d15-n17x1-off8-none': (0, 0.095, None),
    'staged-runs15-tail-d15-n17x4-B7681': (1, 0.041, 0.040),
    'staged-runs15-tail-d15-n17x4-B8197': (1, 0.030, 0.035),
    'staged-runs21-last-d21-n18x32-B7681': (0, 0.016, 0.030),
    'staged-runs21-last-d21-n18x32-B8197': (0, 0.019, 0.026),
    'staged-runs21-control-d21-n19x4-B7681': (1, 0.051, 0.111),
    'staged-runs21-control-d21-n19x4-B8197': (1, 0.055, 0.172),
    'staged-rt5-tail-d5-n3x2-B7681': (0, 0.035, 0.045),
    'staged-rt5-tail-d5-n3x2-B8197': (0, 0.021, 0.054),
    'staged-ct4-d4-n3x2-B7681': (0, 0.015, 0.033),
    'staged-ct4-d4-n3x2-B8197': (0, 0.011, 0.035),
    'staged-ct32-d32-n8x32-B7681': (0, 0.041, 0.111),
    'staged-rt32-d32-n8x4-B7681': (1, 0.089, 0.157),
    'staged-rt32-corner-d32-n8x32-B7681': (0, 0.015, 0.044),
    'regime-runs-d21-gain0.001-conc1-none': (0, 0.006, None),
    'regime-runs-d21-gain0.001-conc0.02-dropout_l1l2': (0, 0.007, 0.008),
    'regime-runs-d21-gain1-conc1-dropout_l1l2': (0, 0.128, 0.178),
    'regime-runs-d21-gain1-conc0.02-none': (0, 0.135, None),
    'regime-runs-d21-gain8-conc1-none': (0, 0.445, None),
    'regime-runs-d21-gain8-conc0.02-dropout_l1l2': (1, 0.034, 0.139),
    'regime-runs-d21-gain30-conc1-dropout_l1l2': (1, 0.001, 0.089),
    'regime-runs-d21-gain30-conc0.02-none': (1, 0.058, None),
    'regime-ct-d15-gain0.001-conc1-dropout_l1l2': (0, 0.008, 0.021),
    'regime-ct-d15-gain0.001-conc0.02-none': (0, 0.010, None),
    'regime-ct-d15-gain1-conc1-none': (0, 0.071, None),
    'regime-ct-d15-gain1-conc0.02-dropout_l1l2': (1, 0.079, 0.157),
    'regime-ct-d15-gain8-conc1-dropout_l1l2': (1, 0.087, 0.151),
    'regime-ct-d15-gain8-conc0.02-none': (1, 0.360, None),
    'regime-ct-d15-gain30-conc1-none': (0, 0.034, None),
    'regime-ct-d15-gain30-conc0.02-dropout_l1l2': (3, 0.244, 0.018),
    'regime-rt-d9-gain0.001-conc1-none': (0, 0.007, None),
    'regime-rt-d9-gain0.001-conc0.02-dropout_l1l2': (0, 0.007, 0.005),
    'regime-rt-d9-gain1-conc1-dropout_l1l2': (0, 0.038, 0.118),
    'regime-rt-d9-gain1-conc0.02-none': (0, 0.025, None),
    'regime-rt-d9-gain8-conc1-none': (0, 0.064, None),
    'regime-rt-d9-gain8-conc0.02-dropout_l1l2': (0, 0.030, 0.195),
    'regime-rt-d9-gain30-conc1-dropout_l1l2': (1, 0.052, 0.062),
    'regime-rt-d9-gain30-conc0.02-none': (0, 0.020, None),
    'regime-mfma-d21-gain0.001-conc1-dropout_l1l2': (0, 0.010, 0.008),
    'regime-mfma-d21-gain0.001-conc0.02-none': (0, 0.009, None),
    'regime-mfma-d21-gain1-conc1-none': (0, 0.029, None),
    'regime-mfma-d21-gain1-conc0.02-dropout_l1l2': (0, 0.036, 0.227),
    'regime-mfma-d21-gain8-conc1-dropout_l1l2': (0, 0.183, 0.230),
    'regime-mfma-d21-gain8-conc0.02-none': (0, 0.097, None),
    'regime-mfma-d21-gain30-conc1-none': (0, 0.415, None),
    'regime-mfma-d21-gain30-conc0.02-dropout_l1l2': (0, 0.081, 0.275),
}


def _cases():
    out = []

    def add(name, fam, d, geom, n3, n4, reg, gain=1.0, conc=1.0, B=100, off=0, n_oracle=512):
        out.append(Case(name, fam, d, geom[0], geom[1], geom[2], n3, n4, reg, gain, conc, B, _SEEDS.get(name, (0,))[0], off, n_oracle))

    alt = ('none', 'dropout_l1l2')
    for i, (d, k1, f2, k2, n3, n4) in enumerate(_GENERIC):
        add('generic-d%d-k%d%d%d-n%dx%d-%s' % (d, k1, f2, k2, n3, n4, alt[i % 2]), 'generic', d, (k1, f2, k2), n3, n4, alt[i % 2])
    for i, d in enumerate(_REF_D):
        add('ref-d%d-%s' % (d, alt[i % 2]), 'ref', d, REF, 8, 4, alt[i % 2])
    for i, (d, off) in enumerate([(21, 4), (21, 8), (15, 4), (15, 8)]):
        add('ref-d%d-off%d-%s' % (d, off, alt[(i // 2 + i) % 2]), 'ref', d, REF, 8, 4, alt[(i // 2 + i) % 2], off=off)
    for j, d in enumerate((21, 15)):
        for i, (n3, n4) in enumerate(_RUNS_N):
            add('runs-d%d-n%dx%d-%s' % (d, n3, n4, alt[(i + j) % 2]), 'runs', d, REF, n3, n4, alt[(i + j) % 2])
    add('runs-d21-n24x8-off8-dropout_l1l2', 'runs', 21, REF, 24, 8, 'dropout_l1l2', off=8)
    add('runs-d15-n17x1-off8-none', 'runs', 15, REF, 17, 1, 'none', off=8)
    for i, (tag, d, geom, n3, n4, batches) in enumerate(_STAGED):
        for B in batches:
            add('staged-%s-d%d-n%dx%d-B%d' % (tag, d, n3, n4, B), 'staged', d, geom, n3, n4, 'dropout_l1l2', B=B)
    for j, (tag, d, geom, n3, n4, off) in enumerate(_REGIME):
        for gi, gain in enumerate(GAINS):
            for ci, conc in enumerate(CONCS):
                reg = alt[(j + gi + ci) % 2]
                add('regime-%s-d%d-gain%g-conc%g-%s' % (tag, d, gain, conc, reg), 'regime', d, geom, n3, n4, reg, gain, conc, off=off)
    return out


CASES = _cases()
FAMILIES = ('generic', 'ref', 'runs', 'staged', 'regime')
_INDEX = {c.name: i for i, c in enumerate(CASES)}


def by_family(family):
    return [c for c in CASES if c.family == family]


def kernel_of(case):
    """The kernel reward_net_forward_sums picks for a case (fc3.weight at a 16-byte boundary + w3_offset)."""
    ref = (case.k1, case.f2, case.k2) == REF
    if ref and case.d in (21, 15):
        if case.n3 <= 16 and case.w3_offset % 8 == 0:
            return 'mfma'
        if case.w3_offset % 8 == 0:
            return 'runs'
    return 'generic-ct' if ref else 'generic-rt'


def lds_bytes(case, staged=True):
    """Dynamic LDS of the launch of a case's kernel (the host formulas of reward_net_forward_sums; runs / generic only)."""
    d, n3, n4 = case.d, case.n3, case.n4
    small = n4 * (n3 + d) + 2 * n4 + 1 + n3
    w3 = n3 * case.f2 * d * d if staged else 0
    if kernel_of(case) == 'runs':
        p = 25 if d == 21 else 19
        tiles = (d + 4) * p + (d + 2) * p
        fl = ((small + 3) & ~3) + w3
    else:
        small += case.k1 * case.k1 + 1 + case.f2 * case.k2 * case.k2 + case.f2
        W1, W2 = d + 2 * (case.k1 // 2), d + 2 * (case.k2 // 2)
        tiles = W1 * W1 + W2 * W2
        fl = ((small + 3) & ~3) + w3
    return 4 * (((fl + 3) & ~3) + RN_WAVES * tiles)


def stages(case, B=None):
    """Whether a launch of B samples of this case copies the FC3 weights into LDS."""
    B = case.B if B is None else B
    if kernel_of(case) == 'mfma' or case.w3_offset % 16:
        return False
    grid = min(-(-B // RN_WAVES), 256 * RN_BPC)
    return (-(-B // grid) >= RN_LDS_MIN and case.n3 * case.f2 * case.d * case.d * 4 <= 64 * 1024
            and lds_bytes(case, True) <= RN_LDS_LIMIT)


def dropout_key(case):
    """(seed, sample_offset) of a case's dropout run: both above 2^32 (the high words of the Philox key and counter) except in
    the regime family."""
    i = _INDEX[case.name]
    if case.family == 'regime':
        return 77 + i, 1000 * i
    return (0x9E3779B97F4A7C15 ^ (i * 0x100000001)) & 0xFFFFFFFFFFFFFFFF, (1 << 33) + 12345 * (i + 1)


def build(case, dev):
    """(net, state [B,d], action [B,d,d]) of a case: the network on `dev` ('cpu' works) with out.weight scaled by the gain and
    fc3.weight re-homed w3_offset bytes past a 16-byte boundary; the inputs as fp32 NumPy arrays."""
    net = _net(case.d, case.reg, case.n3, case.n4, dev, k1=case.k1, f2=case.f2, k2=case.k2, seed=case.seed).eval()
    with torch.no_grad():
        net.out.weight.mul_(case.gain)
    if case.w3_offset:
        w = net.fc3.weight.data
        k = case.w3_offset // 4
        buf = torch.empty(w.numel() + 4, dtype=w.dtype, device=w.device)
        assert buf.data_ptr() % 16 == 0
        buf[k:k + w.numel()].copy_(w.reshape(-1))
        net.fc3.weight.data = buf[k:k + w.numel()].view_as(w)
    assert net.fc3.weight.data_ptr() % 16 == case.w3_offset and net.fc3.weight.is_contiguous()
    d, B = case.d, case.B
    rs = np.random.RandomState(7919 * d + 31 * case.n3 + B + int(1000 * case.conc))
    state = rs.dirichlet(np.full(d, case.conc), size=B).astype(np.float32)
    action = rs.dirichlet(np.full(d, case.conc), size=(B, d)).astype(np.float32)
    if case.conc < 1.0:
        # the policy's actions: exact zeros, and a few rows / samples exactly one-hot
        state[state < 1e-6] = 0.0
        action[action < 1e-6] = 0.0
        for n in range(0, B, 17):
            state[n] = 0.0
            state[n, n % d] = 1.0
            action[n] = np.eye(d, dtype=np.float32)[rs.permutation(d)]
        action[1::17, 0] = 0.0
        action[1::17, 0, d - 1] = 1.0
    assert np.isfinite(state).all() and np.isfinite(action).all()
    return net, state, action


def oracle_indices(case):
    """The samples compared with the oracle: all of them up to n_oracle, else the first and last 16 and every k-th between."""
    B, n = case.B, case.n_oracle
    if B <= n:
        return np.arange(B)
    k = -(-(B - 32) // (n - 32))
    return np.concatenate([np.arange(16), np.arange(16, B - 16, k), np.arange(B - 16, B)])


def oracle(case, net, state, action, idx, dropout):
    """(r_ref [n], tolerance [n]) of the samples idx in fp64: RO.forward_cache, with the kernel's dropout masks of
    dropout_key(case) where `dropout`; tolerance = TOL_REL max(|r_ref|, m), and no more than the absolute bound at gain 1, conc 1."""
    prm = RO.params_from_torch(net)
    masks = None
    if dropout:
        seed, off = dropout_key(case)
        m3, m4 = RO.dropout_masks(net.keep_prob, seed, off, case.B, case.n3, case.n4)
        masks = (m3[idx], m4[idx])
    r, cache = RO.forward_cache(prm, state[idx].astype(np.float64), action[idx].astype(np.float64), masks)
    m = np.abs(cache['h4']).dot(np.abs(prm['out_w'])) + np.abs(prm['out_b'])
    tol = TOL_REL * np.maximum(np.abs(r), m)[:, 0]
    if case.gain == 1.0 and case.conc == 1.0:
        tol = np.minimum(tol, TOL_ABS[bool(dropout)])
    return r[:, 0], tol


def ratio(dev_, tol):
    return float(np.max(np.abs(dev_) / tol)) if np.size(dev_) else 0.0


def f32_forward(prm, state, action, masks=None):
    """The network in fp32 with every sum formed term by term in index order, a rounded product added to a rounded sum: NumPy
    element-wise float32 operations only (IEEE, no BLAS, no FMA, no library reduction), so the result is the same bits on every
    machine.  prm: RO.params_from_torch (TF layouts); masks = (m3, m4) of 0 / (1/keep) or None.  Returns [N] float64."""
    f = lambda a: np.asarray(a, dtype=np.float32)
    N, d = state.shape

    def conv(x, w, b):                        # x [N,H,W], w [kh,kw,Cout], b [Cout] -> [N,H,W,Cout], bias first, taps row by row
        kh, kw, co = w.shape
        xp = np.zeros((N, d + kh - 1, d + kw - 1), dtype=np.float32)
        xp[:, kh // 2:kh // 2 + d, kw // 2:kw // 2 + d] = x
        out = np.empty((N, d, d, co), dtype=np.float32)
        for c in range(co):
            acc = np.full((N, d, d), b[c], dtype=np.float32)
            for u in range(kh):
                for v in range(kw):
                    acc = acc + xp[:, u:u + d, v:v + d] * w[u, v, c]
            out[..., c] = acc
        return np.maximum(out, np.float32(0))

    def dense(x, w, b):                       # x [N,K], w [K,M]: sum over k in order, then the bias
        acc = np.zeros((N, w.shape[1]), dtype=np.float32)
        for k in range(w.shape[0]):
            acc = acc + x[:, k:k + 1] * w[k]
        return acc + b

    a1 = conv(f(action), f(prm['conv1_w'])[:, :, 0, :], f(prm['conv1_b']))[..., 0]
    a2 = conv(a1, f(prm['conv2_w'])[:, :, 0, :], f(prm['conv2_b']))
    h3 = np.maximum(dense(a2.reshape(N, -1), f(prm['fc3_w']), f(prm['fc3_b'])), np.float32(0))
    if masks is not None:
        h3 = h3 * f(masks[0])
    h4 = np.maximum(dense(np.concatenate([h3, f(state)], axis=1), f(prm['fc4_w']), f(prm['fc4_b'])), np.float32(0))
    if masks is not None:
        h4 = h4 * f(masks[1])
    z = dense(h4, f(prm['out_w']), f(prm['out_b']))[:, 0]
    assert z.dtype == np.float32
    return np.tanh(z.astype(np.float64)).astype(np.float32).astype(np.float64)


def _case_masks(case, net, idx):
    seed, off = dropout_key(case)
    m3, m4 = RO.dropout_masks(net.keep_prob, seed, off, case.B, case.n3, case.n4)
    return m3[idx], m4[idx]


def cpu_ratio(case, dropout=False):
    """Worst |f32_forward - oracle| / tolerance over the case's oracle samples; dropout: under the masks of dropout_key(case),
    the network the device's dropout run evaluates."""
    net, state, action = build(case, 'cpu')
    idx = oracle_indices(case)
    ref, tol = oracle(case, net, state, action, idx, dropout)
    got = f32_forward(RO.params_from_torch(net), state[idx], action[idx], _case_masks(case, net, idx) if dropout else None)
    return ratio(got - ref, tol)


def cpu_ratios(case):
    """(dropout off, under the case's masks or None)."""
    return cpu_ratio(case), (cpu_ratio(case, True) if 'dropout' in case.reg else None)


def torch_ratio(case):
    """The same figure for networks.RewardNet itself (dropout off).  A MEASUREMENT: PyTorch's fp32 convolutions and matrix
    products sum in an order that depends on the CPU and the thread count (0.31 on one machine, 0.64 on another for one case)."""
    net, state, action = build(case, 'cpu')
    idx = oracle_indices(case)
    ref, tol = oracle(case, net, state, action, idx, False)
    net.dropout_always = False
    with torch.no_grad():
        got = net(torch.as_tensor(state[idx]), torch.as_tensor(action[idx])).reshape(-1).double().numpy()
    return ratio(got - ref, tol)


if __name__ == '__main__':                    # the seed search: prints the _SEEDS table
    for c in CASES:
        best = (np.inf, 0, None)
        for seed in range(50):
            plain, masked = cpu_ratios(c._replace(seed=seed))
            best = min(best, (max(plain, masked or 0.0), seed, (plain, masked)), key=lambda t: t[:2])
            if best[1] == seed and best[0] <= 0.5:
                break
        print('    %r: (%d, %.3f, %s),' % (c.name, best[1], best[2][0], 'None' if best[2][1] is None else '%.3f' % best[2][1]), flush=True)
