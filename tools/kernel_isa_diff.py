#!/usr/bin/env python3
"""Compare the gfx950 kernels of two builds of libmfg_hip.so, kernel by kernel (CPU only).

For every kernel symbol of build A: its instruction listing (addresses, encodings and trailing padding stripped) and its
.vgpr_count / .sgpr_count / .private_segment_fixed_size against the kernel of the same name in build B.

    python tools/kernel_isa_diff.py A/libmfg_hip.so B/libmfg_hip.so [--verbose]

Steps: llvm-objcopy --dump-section=.hip_fatbin (the section holds one offload bundle per translation unit),
clang-offload-bundler --unbundle of each bundle's gfx950 code object, llvm-objdump -d and llvm-readelf --notes on it.
Exit status 0 when every kernel of A is identical in B (kernels only in B are listed, not counted as differences).
"""
import argparse
import collections
import os
import re
import subprocess
import sys
import tempfile

ROCM = os.environ.get('ROCM_PATH', '/opt/rocm')
LLVM = os.path.join(ROCM, 'llvm', 'bin')
MAGIC = b'__CLANG_OFFLOAD_BUNDLE__'
TARGET = 'hipv4-amdgcn-amd-amdhsa--gfx950'


def tool(name):
    return os.path.join(LLVM, name)


def code_objects(lib, tmp, tag):
    """The gfx950 code objects of every offload bundle in lib's .hip_fatbin section."""
    fat = os.path.join(tmp, tag + '.fatbin')
    subprocess.run([tool('llvm-objcopy'), '--dump-section=.hip_fatbin=' + fat, lib, os.path.join(tmp, tag + '.stripped')],
                   check=True)
    data = open(fat, 'rb').read()
    starts = [m.start() for m in re.finditer(re.escape(MAGIC), data)]
    out = []
    for n, s in enumerate(starts):
        e = starts[n + 1] if n + 1 < len(starts) else len(data)
        bundle = os.path.join(tmp, '%s.%d.bundle' % (tag, n))
        with open(bundle, 'wb') as f:
            f.write(data[s:e])
        co = os.path.join(tmp, '%s.%d.co' % (tag, n))
        r = subprocess.run([tool('clang-offload-bundler'), '--unbundle', '--type=o', '--input=' + bundle, '--output=' + co,
                            '--targets=' + TARGET], capture_output=True, text=True)
        if r.returncode == 0 and os.path.getsize(co) > 0:
            out.append(co)
    if not out:
        raise SystemExit('%s: no %s code object in .hip_fatbin' % (lib, TARGET))
    return out


def listing(co):
    """{kernel symbol: [instruction lines]} of one code object, addresses / encodings / branch targets stripped."""
    txt = subprocess.run([tool('llvm-objdump'), '-d', '--no-show-raw-insn', '--no-leading-addr', co], check=True,
                         capture_output=True, text=True).stdout
    funcs, cur = {}, None
    for line in txt.splitlines():
        m = re.match(r'^(?:[0-9a-f]+ )?<(.+)>:$', line.strip())
        if m:
            cur = m.group(1)
            funcs[cur] = []
            continue
        if cur is None or not line.strip() or line.startswith('Disassembly'):
            continue
        ins = line.split('//')[0].strip()
        ins = re.sub(r'<[^>]*>', '<>', ins)  # branch targets name labels / offsets of this build
        if ins:
            funcs[cur].append(ins)
    # What follows a function's last instruction is layout, not the kernel: the s_nop padding up to the next function (or,
    # behind the last function of a code object, the section's closing run of them) and objdump's '...' for skipped zeros.
    # Which kernel comes last depends on the translation unit it is compiled in.
    for ins in funcs.values():
        while ins and ins[-1] in ('s_nop 0', '...'):
            ins.pop()
    return funcs


def metadata(co):
    """{kernel symbol: {field: value}} of the registers / scratch fields of the code object's metadata note (one entry of
    amdhsa.kernels per kernel: its fields are gathered up to the next entry, wherever .symbol falls among them)."""
    txt = subprocess.run([tool('llvm-readelf'), '--notes', co], check=True, capture_output=True, text=True).stdout
    fields = ('.vgpr_count', '.sgpr_count', '.private_segment_fixed_size', '.agpr_count')
    entries, cur, indent = [], None, None
    for line in txt.splitlines():
        m = re.match(r'^(\s*)- (\.[a-z_]+):', line)
        if m and (indent is None or len(m.group(1)) == indent) and m.group(2) == '.agpr_count':
            indent = len(m.group(1))
            cur = {}
            entries.append(cur)
        if cur is None:
            continue
        s = line.strip().lstrip('- ').strip()
        for f in fields + ('.symbol',):
            if s.startswith(f + ':'):
                cur.setdefault(f, s.split(':', 1)[1].strip())
    meta = {}
    for e in entries:
        sym = e.pop('.symbol', '')
        meta[sym[:-3] if sym.endswith('.kd') else sym] = e
    return meta


def kernels(lib, tmp, tag):
    isa, meta = {}, {}
    for co in code_objects(lib, tmp, tag):
        m = metadata(co)
        meta.update(m)
        for name, ins in listing(co).items():
            if name in m:
                isa[name] = ins
    return isa, meta


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('a', help='build A: libmfg_hip.so (e.g. the parent commit)')
    ap.add_argument('b', help='build B: libmfg_hip.so')
    ap.add_argument('--verbose', action='store_true', help='list identical kernels too')
    ap.add_argument('--histogram', action='append', default=[], metavar='SYMBOL',
                    help='also print the opcode histogram (A, B) of this mangled kernel symbol; may be repeated')
    ap.add_argument('--resources', metavar='SUBSTRING', default=None,
                    help='also print registers / scratch (A -> B) of every kernel whose symbol contains SUBSTRING')
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        isa_a, meta_a = kernels(args.a, tmp, 'a')
        isa_b, meta_b = kernels(args.b, tmp, 'b')
    same, diff = 0, []
    for name in sorted(isa_a):
        if name not in isa_b:
            diff.append((name, 'missing in B'))
            continue
        why = []
        if isa_a[name] != isa_b[name]:
            n = sum(1 for x, y in zip(isa_a[name], isa_b[name]) if x != y) + abs(len(isa_a[name]) - len(isa_b[name]))
            why.append('instructions: %d vs %d, %d differ' % (len(isa_a[name]), len(isa_b[name]), n))
        for f in sorted(set(meta_a.get(name, {})) | set(meta_b.get(name, {}))):
            va, vb = meta_a.get(name, {}).get(f), meta_b.get(name, {}).get(f)
            if va != vb:
                why.append('%s %s -> %s' % (f, va, vb))
        if why:
            diff.append((name, '; '.join(why)))
        else:
            same += 1
            if args.verbose:
                print('same  %s (%d instructions)' % (name, len(isa_a[name])))
    for name, why in diff:
        print('DIFF  %s: %s' % (name, why))
    only_b = sorted(set(isa_b) - set(isa_a))
    for name in only_b:
        m = meta_b.get(name, {})
        print('new   %s (%d instructions, .vgpr_count %s, .sgpr_count %s, .private_segment_fixed_size %s)' % (
            name, len(isa_b[name]), m.get('.vgpr_count'), m.get('.sgpr_count'), m.get('.private_segment_fixed_size')))
    for sym in args.histogram:
        ha, hb = (collections.Counter(i.split()[0] for i in isa.get(sym, [])) for isa in (isa_a, isa_b))
        print('\nopcode histogram of %s: %d -> %d instructions, .vgpr_count %s -> %s, .private_segment_fixed_size %s -> %s' % (
            sym, sum(ha.values()), sum(hb.values()), meta_a.get(sym, {}).get('.vgpr_count'), meta_b.get(sym, {}).get('.vgpr_count'),
            meta_a.get(sym, {}).get('.private_segment_fixed_size'), meta_b.get(sym, {}).get('.private_segment_fixed_size')))
        for op in sorted(set(ha) | set(hb), key=lambda o: -max(ha[o], hb[o])):
            if ha[op] != hb[op] or max(ha[op], hb[op]) >= 40:
                print('  %-28s %6d %6d  %+d' % (op, ha[op], hb[op], hb[op] - ha[op]))
    if args.resources:
        print('\nregisters / scratch of the kernels matching %r (A -> B; * = rises)' % args.resources)
        for name in sorted(n for n in isa_a if args.resources in n and n in isa_b):
            va, vb = (int(m.get(name, {}).get('.vgpr_count', 0)) for m in (meta_a, meta_b))
            sa, sb = (int(m.get(name, {}).get('.private_segment_fixed_size', 0)) for m in (meta_a, meta_b))
            print('  %-78s vgpr %3d -> %3d%s  scratch %4d -> %4d%s' % (name, va, vb, ' *' if vb > va else '  ', sa, sb, ' *' if sb > sa else ''))
    print('%d kernels of A: %d identical, %d differ; %d kernels only in B' % (len(isa_a), same, len(diff), len(only_b)))
    return 1 if diff else 0


if __name__ == '__main__':
    sys.exit(main())
