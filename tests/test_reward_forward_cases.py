"""The admission rule of oracle/reward_forward_cases.py, on the CPU: for every case a plain fp32 evaluation of the network
(FC.f32_forward: sums term by term in NumPy float32, bit-reproducible; dropout off, and under the masks of the case's dropout
run) stays within HALF of the tolerance that tests/test_gpu_reward_net_forward_paths.py allows the HIP kernels against the fp64
oracle -- 1e-5 max(|r_ref|, m), m = |h4| . |out_w| + |out_b|, and at gain 1 / concentration 1 no more than the 2e-6 (5e-6 with
dropout) of the existing forward tests.  A case whose reference alone leaves the bound would prove nothing on the device.  (A
worst-case bound through the absolute-value network is ~1 000 times looser -- c u A ~ 9e-3 at d = 21 -- and would catch nothing.)
networks.RewardNet in fp32 is printed next to it, not asserted: PyTorch's summation order, and with it that ratio, changes with
the CPU (see the table's docstring); f32_forward is tied to the module by test_f32_forward_is_the_module.  Staged cases are
evaluated on their oracle subsample (at most 512 samples).  Also pins what the table promises the GPU tests: the kernels, the
staging rule and the LDS figures its cases are there for."""
import numpy as np
import pytest

from oracle import reward_forward_cases as FC


@pytest.mark.parametrize('case', FC.CASES, ids=[c.name for c in FC.CASES])
def test_cpu_fp32_reference_stays_within_half_the_tolerance(case):
    """Dropout off, and for a dropout network also under the masks of its device run (FC.dropout_key): to the device those are
    two networks, and the case is admitted on both.  f32_forward is deterministic: the ratios ARE the recorded ones."""
    plain, masked = FC.cpu_ratios(case)
    fmt = lambda q: 'None' if q is None else '%.3f' % q
    print('\n%-52s %-10s seed %d  fp32 ratio %s / %s  (networks.RewardNet on this CPU: %.3f)'
          % (case.name, FC.kernel_of(case), case.seed, fmt(plain), fmt(masked), FC.torch_ratio(case)))
    assert plain <= 0.5 and (masked is None or masked <= 0.5), 'choose another network seed (python -m oracle.reward_forward_cases)'
    for q, rec in zip((plain, masked), FC._SEEDS[case.name][1:]):
        assert (q is None and rec is None) or abs(q - rec) <= 2e-3, 'the table records another ratio'


def test_f32_forward_is_the_module():
    """f32_forward against networks.RewardNet in fp32 (layouts, NHWC flatten, concat order): they differ by summation order only,
    a few ulp of the pre-activation scale -- 100 times below the 1e-5 the admission rule works at."""
    import torch
    from oracle import reward_net_oracle as RO
    for name in ('generic-d17-k325-n8x4-dropout_l1l2', 'runs-d21-n32x32-none', 'ref-d32-dropout_l1l2'):
        case = next(c for c in FC.CASES if c.name == name)
        net, state, action = FC.build(case, 'cpu')
        net.dropout_always = False
        with torch.no_grad():
            want = net(torch.as_tensor(state), torch.as_tensor(action)).reshape(-1).double().numpy()
        got = FC.f32_forward(RO.params_from_torch(net), state, action)
        assert np.abs(got - want).max() <= 1e-6, name


def test_every_case_has_a_recorded_seed_and_a_unique_name():
    names = [c.name for c in FC.CASES]
    assert len(set(names)) == len(names) and set(names) == set(FC._SEEDS)
    assert all(plain <= 0.5 and (masked is None or masked <= 0.5) for _, plain, masked in FC._SEEDS.values())
    assert all((FC._SEEDS[c.name][2] is None) == ('dropout' not in c.reg) and c.seed == FC._SEEDS[c.name][0] for c in FC.CASES)


def test_table_reaches_the_paths_it_names():
    K = FC.kernel_of
    fam = {f: FC.by_family(f) for f in FC.FAMILIES}
    assert all(K(c) == 'generic-rt' for c in fam['generic']) and len(fam['generic']) == 11
    assert {c.d for c in fam['generic']} >= {1, 2, 8, 9, 16, 17, 21, 22, 32}
    assert all(K(c) == 'generic-ct' for c in fam['ref'] if c.w3_offset != 8) and {K(c) for c in fam['ref'] if c.w3_offset == 8} == {'mfma'}
    assert {(c.d, c.w3_offset) for c in fam['ref'] if c.w3_offset} == {(21, 4), (21, 8), (15, 4), (15, 8)}
    assert all(K(c) == 'runs' for c in fam['runs']) and {(c.d, c.w3_offset) for c in fam['runs']} >= {(21, 8), (15, 8), (21, 0), (15, 0)}
    assert any((c.d, c.n3, c.n4) == (21, 32, 32) for c in fam['runs'])
    assert not any(FC.stages(c) for f in ('generic', 'ref', 'runs', 'regime') for c in fam[f])
    # the staged family: B >= 7 681 stages, any slice of at most 7 680 does not; the figures of the LDS corner
    assert FC.STAGE_B == 7681
    st = {c.name.split('-d')[0][7:]: c for c in fam['staged'] if c.B == 7681}
    for tag, c in st.items():
        assert not FC.stages(c, 7680) and not FC.stages(c, 4099)
        assert FC.stages(c) == (tag not in ('runs21-control', 'rt32-corner')), tag
    assert (17 * 450) % 4 == 2 and st['runs15-tail'].n3 * 2 * 15 * 15 == 17 * 450 and 3 * 1 * 5 * 5 == 75
    assert 18 * 882 * 4 == 63504 and 19 * 882 * 4 == 67032
    assert [FC.lds_bytes(st[t]) for t in ('runs21-last', 'ct32', 'rt32', 'rt32-corner')] == [107232, 149600, 159264, 163968]
    assert 159264 <= FC.RN_LDS_LIMIT < 163968
    assert all(len(FC.oracle_indices(c)) <= 512 and FC.oracle_indices(c)[-1] == c.B - 1 for c in fam['staged'])
    # regimes: every gain x concentration for one shape per kernel
    assert {K(c) for c in fam['regime']} == {'runs', 'generic-ct', 'generic-rt', 'mfma'}
    for k in ('runs', 'generic-ct', 'generic-rt', 'mfma'):
        assert {(c.gain, c.conc) for c in fam['regime'] if K(c) == k} == {(g, a) for g in FC.GAINS for a in FC.CONCS}
    # a dropout run with seed and sample offset above 2^32 for every kernel
    for k in ('runs', 'generic-ct', 'generic-rt', 'mfma'):
        assert any(c.reg == 'dropout_l1l2' and min(FC.dropout_key(c)) > 1 << 32 for c in FC.CASES if K(c) == k), k


def test_low_concentration_inputs_carry_exact_zeros_and_one_hot_rows():
    case = next(c for c in FC.by_family('regime') if c.conc == 0.02 and FC.kernel_of(c) == 'runs')
    _, state, action = FC.build(case, 'cpu')
    assert (action == 0).mean() > 0.3 and (state == 0).any()
    onehot = ((action == 1).sum(-1) == 1) & ((action != 0).sum(-1) == 1)
    assert onehot[0].all() and onehot.sum() >= case.d + 5
    assert (state[0] == 1).sum() == 1 and (state[0] != 0).sum() == 1
    assert abs(action.sum(-1) - 1).max() < 1e-4
