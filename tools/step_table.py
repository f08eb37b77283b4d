"""Static instruction table of ONE ENV STEP of the training call's rollout kernel OUTSIDE the quad loop, by piece (developer
tool; no GPU).  The sibling of tools/loop_table.py, which covers the quad loop itself.

A wave issues the code of the step loop once per env step (a lane is a matrix row), so the hot path of that loop without the
quad loop is what a wave spends per step besides its floor(d/4) quads per row.  The script compiles the shipped sources twice
-- with and without line tables (-gline-tables-only) -- and checks that both give the SAME opcode sequence for the kernel.  The
listing with line tables is assembled and linked, and llvm-symbolizer gives every instruction its stack of inlined frames; the
frame of core_small_body is the line of the body the instruction was compiled for, whatever helper it went through, and the
ranges of the body between the anchors below (found in the source by their text, not by line number) are the pieces.  Basic
blocks of the rare continuations (exact acceptance, small shapes, denormal variates: a frame of gamma_fix and what goes with it,
their rejection loops) are set apart as cold.  The pieces partition the region, so their opcode histograms add up to the region's
(checked), and [whole kernel = outside the step loop + step loop outside the quad loop + quad loop] is checked against the listing.
What the scheduler hoists or merges keeps the line of its origin; address arithmetic shared by two pieces is booked where the
compiler left it.  The column pass is a loop of 3 (d = 21) or 2 (d = 15) trips inside the step loop: its body counts that often.
usage: python tools/step_table.py [21 | 15] > profiles/lean_step_table_d21.txt"""
import collections, os, re, subprocess, sys, tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'discrete_mean_field_game_amd', 'csrc')
COST = {'mad64': 6.4, 'trans': 8.0, 'f64': 4.6, 'plain': 2.2}          # cycles per wave64 instruction (profiles/r03_valu_rates.txt)
PIECES = ['step set-up', 'E/F staging', 'quad loop: code left outside the loop', 'trailing element', 'row epilogue', 'column pass',
          'value terms', 'per-trajectory sums', 'TD error and stores']
COLD = 'cold continuations (not on the hot path)'

# core_small_body: (text that starts a range, piece), in source order from the head of the step loop to its end
BODY_ANCHORS = [
    ('for (int s = 0; s < T; ++s) {', 'step set-up'),
    ('float Fi = 0.0f;', 'E/F staging'),
    ('MFG_STAMP(1)', 'step set-up'),
    ('using TT = typename PolicyTerms<FAST>::T;', 'quad loop: code left outside the loop'),
    ('if (dq < d) {  // 1..3 trailing elements', 'trailing element'),
    ('MFG_STAMP(2)', 'row epilogue'),
    ('MFG_STAMP(3)', 'column pass'),
    ('MFG_STAMP(4)', 'per-trajectory sums'),
    ('if (want_v) {', 'value terms'),
    ('const bool par = d >= 8;', 'per-trajectory sums'),
    ('const int gl = d > 1 ? 1 : 0;', 'TD error and stores'),
    ('MFG_STAMP(5)', 'step set-up'),
    ('if (valid && a.pi_next_out)', None),
]
# frames that mark an instruction as part of a rare continuation (function, or (function, text of the line))
COLD_FUNCS = ('gamma_fix', 'gamma_try<', 'gamma_exact_path', 'log2_pos', 'policy_term_denormal')
TAIL_COLD = ['bool sure = true;', '(void)gamma_try<16>(pe.gs, xn, kf, sure);', 'if (!sure || pe.gs.small) y = gamma_fix(',
             'if (__builtin_expect(cm != 0, 0) && y < FLT_MIN_NORMAL)']
LLVM = os.path.join(os.environ.get('ROCM_PATH', '/opt/rocm'), 'llvm', 'bin')


def klass(op):
    if op.startswith('v_mad_u64') or op.startswith('v_lshl_add_u64'):
        return 'mad64'
    if re.match(r'v_(log|exp|rcp|rsq|sqrt|sin|cos)_f32', op):
        return 'trans'
    if 'f64' in op:
        return 'f64'
    return 'plain'


def compile_asm(out, extra):
    cmd = ['/opt/rocm/bin/hipcc'] + subprocess.check_output(['make', '-s', '-C', CSRC, 'flags', 'U=mfg_core_small'], text=True).split() + [  # (csrc/Makefile owns the flags)
           '-S', '--cuda-device-only'] + extra + [
           '-o', out, os.path.join(CSRC, 'mfg_core_small.hip')]
    subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return open(out).read().split('\n')


def kernel_body(text, kernel):
    start = next(i for i, l in enumerate(text) if l.startswith(kernel + ':'))
    end = next(i for i in range(start, len(text)) if text[i].startswith('.Lfunc_end'))
    return text[start:end]


def opcode(line):
    if line.lstrip().startswith((';', '.')) or not re.match(r'^\s+[a-z]', line):
        return None
    return re.sub(r'_e32$|_e64$|_sdwa$|_dpp$', '', line.split()[0])


def body_lines(path):
    """line of core_small_body -> piece; the cold lines of sample_tail1"""
    src = open(path).read().split('\n')
    def find(text, after=0):
        return next(i for i in range(after, len(src)) if text in src[i]) + 1
    body = find('__device__ __forceinline__ void core_small_body(')
    pos, marks, piece = body, [], {}
    for text, p in BODY_ANCHORS:
        pos = find(text, pos)
        marks.append((pos, p))
    for (s, p), (e, _) in zip(marks, marks[1:]):
        for n in range(s, e):
            piece[n] = p
    for n in range(body, marks[0][0]):
        piece[n] = 'step set-up'      # (what the compiler re-derives inside the loop from the body's prologue: lane ids, pointers)
    tail = find('__device__ __forceinline__ void sample_tail1(')
    return piece, {find(t, tail) for t in TAIL_COLD}


def frames_of(gs, kernel, tmp):
    """[(opcode, [(function, file, line), ...innermost first])] of the kernel, from the assembled and linked listing"""
    obj, so = os.path.join(tmp, 'g.o'), os.path.join(tmp, 'g.so')
    subprocess.run([os.path.join(LLVM, 'clang'), '-x', 'assembler', '-target', 'amdgcn-amd-amdhsa', '-mcpu=gfx950', '-c', gs, '-o', obj],
                   check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    subprocess.run([os.path.join(LLVM, 'ld.lld'), '-shared', obj, '-o', so], check=True)
    dis = subprocess.run([os.path.join(LLVM, 'llvm-objdump'), '-d', '--no-show-raw-insn', '--disassemble-symbols=' + kernel, so],
                         check=True, capture_output=True, text=True).stdout
    ops = []
    for l in dis.split('\n'):
        m = re.match(r'^\s+([a-z][a-z_0-9]+)\b.*//\s*([0-9A-Fa-f]+):', l)
        if m:
            ops.append((re.sub(r'_e32$|_e64$|_sdwa$|_dpp$', '', m.group(1)), m.group(2)))
    sym = subprocess.run([os.path.join(LLVM, 'llvm-symbolizer'), '--obj=' + so, '--inlines'], input='\n'.join('0x' + a for _, a in ops) + '\n',
                         check=True, capture_output=True, text=True).stdout
    out = []
    for (op, _), blk in zip(ops, sym.strip('\n').split('\n\n')):
        ls = blk.split('\n')
        fr = []
        for f, pos in zip(ls[0::2], ls[1::2]):
            m = re.match(r'^(.*):(\d+):(\d+)$', pos)
            fr.append((f, os.path.basename(m.group(1)) if m else '?', int(m.group(2)) if m else 0))
        out.append((op, fr))
    return out


def main():
    d = int(sys.argv[1]) if len(sys.argv) > 1 else 21
    kernel = '_ZN3mfg17k_core_small_leanILi%dEEEvNS_8CoreArgsE' % d
    tmp = tempfile.mkdtemp()
    if len(sys.argv) > 2:   # developer shortcut: a directory that already holds both listings (g.s with line tables, p.s without)
        gs = os.path.join(sys.argv[2], 'g.s')
        tg, tp = (open(os.path.join(sys.argv[2], n)).read().split('\n') for n in ('g.s', 'p.s'))
    else:
        gs = os.path.join(tmp, 'g.s')
        with ThreadPoolExecutor(2) as ex:
            fg = ex.submit(compile_asm, gs, ['-gline-tables-only'])
            fp = ex.submit(compile_asm, os.path.join(tmp, 'p.s'), [])
            tg, tp = fg.result(), fp.result()
    body = kernel_body(tg, kernel)
    plain_ops = [o for o in map(opcode, kernel_body(tp, kernel)) if o]
    frames = frames_of(gs, kernel, tmp)
    piece_of, tail_cold = body_lines(os.path.join(CSRC, 'mfg_core.h'))

    # basic blocks with their loop membership (the assembler's loop comments)
    parent, has_child, blocks, cur_block = {}, set(), [], None
    i = 0
    while i < len(body):
        l = body[i]
        m = re.match(r'^(?:\.L(BB\d+_\d+):|; %bb\.\d+:)(.*)$', l)
        if m:
            label, hdr, chain, j, comment = m.group(1), None, [], i, m.group(2)
            while True:
                mm = re.search(r'in Loop: Header=(BB\d+_\d+) Depth=(\d+)', comment)
                if mm:
                    hdr = mm.group(1)
                mm = re.search(r'Parent Loop (BB\d+_\d+) Depth=(\d+)', comment)
                if mm:
                    chain.append(mm.group(1))
                if re.search(r'This (?:Inner )?Loop Header: Depth=(\d+)', comment):
                    hdr = label
                    parent[label] = chain[-1] if chain else None
                if 'Child Loop' in comment:
                    has_child.add(label)
                if j + 1 < len(body) and body[j + 1].lstrip().startswith(';') and 'Loop' in body[j + 1]:
                    j += 1
                    comment = body[j]
                else:
                    break
            cur_block = {'loop': hdr, 'ins': []}
            blocks.append(cur_block)
            i = j + 1
            continue
        op = opcode(l)
        if op:
            if cur_block is None:
                cur_block = {'loop': None, 'ins': []}
                blocks.append(cur_block)
            cur_block['ins'].append(op)
        i += 1
    g_ops = [op for b in blocks for op in b['ins']]
    if g_ops != plain_ops:
        sys.exit('the build with line tables is not the shipped code: %d vs %d instructions' % (len(g_ops), len(plain_ops)))
    if g_ops != [op for op, _ in frames]:
        sys.exit('the disassembly of the assembled listing does not follow the listing (%d vs %d instructions)' % (len(frames), len(g_ops)))

    def chain_of(loop):
        out = []
        while loop:
            out.append(loop)
            loop = parent.get(loop)
        return out
    depth_of = {lp: len(chain_of(lp)) for lp in parent}
    step_loop = [lp for lp, n in depth_of.items() if n == 2]
    quad_loop = [lp for lp, n in depth_of.items() if n == 3 and lp in has_child]
    if len(step_loop) != 1 or len(quad_loop) != 1:
        sys.exit('expected one step loop and one quad loop with inner loops: %r %r' % (step_loop, quad_loop))
    step_loop, quad_loop = step_loop[0], quad_loop[0]

    def is_cold(fr):
        return any(f.startswith(COLD_FUNCS) or (f.startswith('sample_tail1') and n in tail_cold) for f, _, n in fr)

    hist = {p: collections.Counter() for p in PIECES + [COLD]}
    n_outside = n_quad = static_sum = 0
    col_trips, k = None, 0
    region = collections.Counter()
    last = 'step set-up'
    for b in blocks:
        fr_b = frames[k:k + len(b['ins'])]
        k += len(b['ins'])
        ch = chain_of(b['loop'])
        if step_loop not in ch:
            n_outside += len(b['ins'])
            continue
        if quad_loop in ch:
            n_quad += len(b['ins'])
            continue
        inner = [lp for lp in ch if depth_of[lp] == 3]
        tags = []
        for op, fr in fr_b:
            core = [n for f, fl, n in fr if f.startswith('core_small_body') and fl == 'mfg_core.h']
            if core and piece_of.get(core[0]):
                last = piece_of[core[0]]
            tags.append(last)   # (no line: the piece of the instruction before)
        n_cold = sum(1 for _, fr in fr_b if is_cold(fr))
        is_col_loop = bool(inner) and collections.Counter(tags).most_common(1)[0][0] == 'column pass'
        cold_block = (bool(inner) and not is_col_loop) or 2 * n_cold > len(tags)
        trips = 1
        if is_col_loop:
            trips = col_trips = {21: 3, 15: 2}[d]
        for (op, _), t in zip(fr_b, tags):
            region[op] += 1
            hist[COLD if cold_block else t][op] += trips
        static_sum += len(tags)
    if n_outside + n_quad + static_sum != len(plain_ops):
        sys.exit('the split of the kernel does not add up')
    if col_trips is None:
        col_trips = 1
    def row(name, h):
        valu = sum(v for k_, v in h.items() if k_.startswith('v_'))
        cyc = sum(COST[klass(k_)] * v for k_, v in h.items() if k_.startswith('v_'))
        return (name, valu, sum(v for k_, v in h.items() if k_.startswith('s_')), sum(v for k_, v in h.items() if k_.startswith('ds_')),
                sum(v for k_, v in h.items() if k_.startswith(('global_', 'flat_', 'scratch_', 'buffer_'))), cyc,
                sum(v for k_, v in h.items() if k_ in ('v_readlane_b32', 'v_writelane_b32')))
    print('k_core_small_lean<%d>: one env step of a wave OUTSIDE the quad loop, by piece (hot path; static count from the listing of the shipped' % d)
    print('sources, attributed by the line of core_small_body each instruction was inlined for; the column-pass loop body counted %d times).' % col_trips)
    print('Checked: the build with line tables has the opcode sequence of the shipped build; the pieces partition the region; kernel = %d outside' % n_outside)
    print('the step loop + %d step loop outside the quad loop (static) + %d quad loop with its continuations = %d instructions.' % (
        static_sum, n_quad, len(plain_ops)))
    print('%-44s %6s %6s %5s %5s %8s %9s' % ('piece', 'VALU', 'scalar', 'LDS', 'VMEM', 'cycles', 'lane r/w'))
    hot = collections.Counter()
    for p in PIECES:
        hot.update(hist[p])
        print('%-44s %6d %6d %5d %5d %8.0f %9d' % row(p, hist[p]))
    print('%-44s %6d %6d %5d %5d %8.0f %9d' % row('TOTAL hot path per wave and step', hot))
    print('%-44s %6d %6d %5d %5d %8.0f %9d' % row(COLD, hist[COLD]))
    print('(cycles: VALU issue cycles per wave at the rates of profiles/r03_valu_rates.txt; lane r/w: v_readlane_b32 / v_writelane_b32, the reloads of spilled scalars)')
    for p in PIECES:
        print('%-44s %s' % (p, ', '.join('%s %d' % (k_, v) for k_, v in hist[p].most_common() if k_.startswith('v_') and v >= 2)))
    print('The trailing element: both parities of the env step are in its count (the even step draws the Philox block and the Box-Muller pair,')
    print('the odd step takes the carried partner: sample_tail1); a wave runs one of the two paths per step.')


if __name__ == '__main__':
    main()
