"""
The memory waits of the listed frame loop, read off the compiler's assembly of kernels.hip:
    hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 --offload-device-only -S bild_amd/csrc/kernels.hip -o kernels.s
    python tools/wait_audit.py kernels.s
For logl_one_kernel<10, 1, 16, 4, 2, 3, 2> (the headline's kernel) and geometry 23's logl_kernel: VGPRs, spilled VGPRs, scratch
bytes and scratch accesses by loop depth; and for the two-row (PAIR) body of the first, every `s_waitcnt vmcnt` at loop depth >= 2
with the loads issued since the last vmcnt(0) in program order (an upper bound of what the wait can be for: a wait behind a
branch lists the loads of the path in front of it in the file).  Loads are named by width and immediate offset.
"""
import re
import sys

ONE = '_ZN4bild12_GLOBAL__N_115logl_one_kernelILi10ELi1ELi16ELi4ELi2ELi3ELi2EEEvNS_7KParamsENS_10WalkParamsE'
G23 = '_ZN4bild12_GLOBAL__N_111logl_kernelILi10ELi1ELi16ELi4ELi2ELi3ELi1ELi2ELb0ELb1ELb0EEEvNS_7KParamsE'


def body(lines, sym):
    a = next(i for i, l in enumerate(lines) if l.startswith(sym + ':'))
    b = next(i for i in range(a, len(lines)) if lines[i].strip().startswith('.amdhsa_kernel ' + sym))
    return lines[a:b]


def with_depth(fn):
    """ (line, loop depth) from the block comments of the assembly printer """
    depth = 0
    for l in fn:
        m = re.search(r'Depth=(\d)', l)
        if m and (l.startswith('.LBB') or l.startswith('; %bb') or 'Loop Header' in l):
            depth = int(m.group(1))
        elif re.match(r'^\.LBB\d+_\d+:\s*$', l):
            depth = 0
        yield l, depth


def figures(text, lines, name, sym):
    acc = {}
    for l, depth in with_depth(body(lines, sym)):
        if l.strip().startswith(('scratch_load', 'scratch_store')):
            acc[depth] = acc.get(depth, 0) + 1
    i0 = text.index('.name:           ' + sym)
    meta = text[text.rfind('\n  - .a', 0, i0): text.find('\n  - .a', i0)]
    val = lambda key: re.search(r'\.' + key + r':\s*(\d+)', meta).group(1)  # noqa: E731
    print(f"{name}: VGPRs {val('vgpr_count')}, spilled VGPRs {val('vgpr_spill_count')}, scratch {val('private_segment_fixed_size')} B, "
          f"scratch accesses by loop depth 0 / 1 / 2 / 3: " + ' / '.join(str(acc.get(d, 0)) for d in range(4)))


def waits(lines):
    fn = body(lines, ONE)
    # the PAIR body begins at the first block whose S sum and rank-1 update are five DPP FMAs each
    starts = [i for i, l in enumerate(fn) if re.match(r'^(\.LBB\d+_\d+:|; %bb\.\d+:)', l)] + [len(fn)]
    first = next(a for a, b in zip(starts, starts[1:]) if sum('v_fmac_f64_dpp' in l for l in fn[a:b]) == 10)
    pending, rows = [], []
    for i, (l, depth) in enumerate(with_depth(fn)):
        if i < first:
            continue
        t = l.strip()
        if t.startswith(('global_load', 'scratch_load')):
            pending.append(t.split()[0].replace('global_load_', 'g.').replace('scratch_load_', 'scratch.') +
                           ('@' + t.split('offset:')[1] if 'offset:' in t else ''))
        m = re.search(r's_waitcnt.*vmcnt\((\d+)\)', t)
        if m:
            if depth >= 2:
                rows.append((i + 1, depth, int(m.group(1)), list(pending)))
            if int(m.group(1)) == 0:
                pending = []
    for line, depth, cnt, loads in rows:
        print(f"  line {line:6d} depth {depth} vmcnt({cnt})  {' '.join(loads) or '-'}")
    print(f"  {len(rows)} waits at depth >= 2, {sum(1 for r in rows if r[1] == 3)} of them at depth 3")


if __name__ == '__main__':
    text = open(sys.argv[1]).read()
    lines = text.split('\n')
    figures(text, lines, 'logl_one_kernel<10, 1, 16, 4, 2, 3, 2>', ONE)
    figures(text, lines, "geometry 23's logl_kernel", G23)
    print('PAIR body of logl_one_kernel<10, 1, 16, 4, 2, 3, 2>, waits for vector memory at loop depth >= 2 (line of the function):')
    waits(lines)
