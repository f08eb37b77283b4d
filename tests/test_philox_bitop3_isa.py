"""CPU check of the compiled code: the headline kernel keeps its Philox rounds in three-input bit operations.

csrc/mfg_device.h (xor3) asks for v_bitop3_b32 on the device side; a later compiler or a later edit that gives the two v_xor_b32
per round word back would cost ~15 instructions per quad without failing any result test.  The listing of
k_core_small<true, true, true, 21, false, 0> is taken from the built library with the ROCm LLVM tools; where they are missing
the test skips.  The library read is the one the package loads (MFG_HIP_LIB selects another build: with a build of an older
commit selected, as in an A/B run, this test fails by design).  Bounds: at least 400 v_bitop3_b32 and at most 100 v_xor_b32 (502 / 0 with the fused form, 4 / 905 without)."""
import collections
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = os.path.join(os.environ.get('ROCM_PATH', '/opt/rocm'), 'llvm', 'bin')
KERNEL = '_ZN3mfg12k_core_smallILb1ELb1ELb1ELi21ELb0ELi0EEEvNS_8CoreArgsE'
MAGIC = b'__CLANG_OFFLOAD_BUNDLE__'
TARGET = 'hipv4-amdgcn-amd-amdhsa--gfx950'


def _tool(name):
    path = os.path.join(LLVM, name)
    if not os.path.exists(path):
        pytest.skip('%s not found under the ROCm tree' % name)
    return path


def _kernel_listing(lib, tmp):
    """Instruction mnemonics of KERNEL in the gfx950 code object of the bundle of lib's .hip_fatbin that defines it."""
    objcopy, bundler, objdump = _tool('llvm-objcopy'), _tool('clang-offload-bundler'), _tool('llvm-objdump')
    fat = os.path.join(tmp, 'fatbin')
    subprocess.run([objcopy, '--dump-section=.hip_fatbin=' + fat, lib, os.path.join(tmp, 'stripped')], check=True)
    data = open(fat, 'rb').read()
    starts = [m.start() for m in re.finditer(re.escape(MAGIC), data)]
    for n, s in enumerate(starts):
        e = starts[n + 1] if n + 1 < len(starts) else len(data)
        bundle, co = os.path.join(tmp, '%d.bundle' % n), os.path.join(tmp, '%d.co' % n)
        with open(bundle, 'wb') as f:
            f.write(data[s:e])
        r = subprocess.run([bundler, '--unbundle', '--type=o', '--input=' + bundle, '--output=' + co, '--targets=' + TARGET],
                           capture_output=True)
        if r.returncode != 0 or not os.path.exists(co) or os.path.getsize(co) == 0:
            continue
        txt = subprocess.run([objdump, '-d', '--no-show-raw-insn', '--no-leading-addr', '--disassemble-symbols=' + KERNEL, co],
                             check=True, capture_output=True, text=True).stdout
        ops = [m.group(1) for m in (re.match(r'^\s+([a-z][a-z_0-9]+)\s', ln + ' ') for ln in txt.splitlines()) if m]
        if ops:
            return ops
    return None


def test_headline_kernel_keeps_the_fused_xor(tmp_path):
    from discrete_mean_field_game_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip('the library is not built')
    ops = _kernel_listing(_lib.LIB_PATH, str(tmp_path))
    assert ops is not None, 'no gfx950 code object of the library defines %s' % KERNEL
    hist = collections.Counter(re.sub(r'_e32$|_e64$', '', op) for op in ops)
    print('v_bitop3_b32 %d, v_xor_b32 %d, %d instructions' % (hist['v_bitop3_b32'], hist['v_xor_b32'], len(ops)))
    assert len(ops) > 3000                      # the whole kernel was listed, not a fragment
    assert hist['v_bitop3_b32'] >= 400
    assert hist['v_xor_b32'] <= 100
