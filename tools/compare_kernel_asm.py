#!/usr/bin/env python3
"""Kernel-for-kernel comparison of two builds' device assembly (no GPU needed):

    tools/compare_kernel_asm.py BASE_DIR NEW_DIR

Each directory holds the `hipcc -S --cuda-device-only` output (*.s) of every translation unit of one build.  The two builds
are equal when they define the same kernels, each exactly once, with the same instruction text (local labels renumbered by
order of first appearance within the kernel) and the same .amdhsa_* descriptor values.  Prints one line per kernel and a
verdict; exits 1 when anything differs."""
import glob
import os
import re
import sys

LOCAL = re.compile(r'\.L[A-Za-z_]*\d+(?:_\d+)?|\bBB\d+_\d+')


def kernels_of(path):
    """{name: (instruction lines, descriptor lines)} of one assembly file"""
    lines = open(path).read().split('\n')
    bodies, descs, cur, desc = {}, {}, None, None
    for line in lines:
        m = re.match(r'^([_A-Za-z0-9$.]+):\s*; @', line)
        if m:
            cur = m.group(1)
            bodies[cur] = []
            continue
        if line.startswith('.Lfunc_end'):
            cur = None
            continue
        m = re.match(r'^\s*\.amdhsa_kernel\s+(\S+)', line)
        if m:
            desc = m.group(1)
            descs[desc] = []
            continue
        if line.strip() == '.end_amdhsa_kernel':
            desc = None
            continue
        if desc is not None:
            descs[desc].append(line.strip())
        elif cur is not None:
            bodies[cur].append(line.rstrip())
    out = {}
    for name, d in descs.items():          # (only kernels have a descriptor: device functions that were not inlined are skipped)
        seen = {}
        body = [LOCAL.sub(lambda m: seen.setdefault(m.group(0).lstrip('.L'), 'L%d' % len(seen)), l) for l in bodies[name]]
        body = [re.sub(r'\s+;', ' ;', l) for l in body]          # (the comment column moves with the width of a label's number)
        out[name] = (body, d)
    return out


def build_of(directory):
    table, twice = {}, []
    for path in sorted(glob.glob(os.path.join(directory, '*.s'))):
        for name, k in kernels_of(path).items():
            if name in table:
                twice.append((name, table[name][0], os.path.basename(path)))
            table[name] = (os.path.basename(path), k)
    return table, twice


def main():
    base, twice_base = build_of(sys.argv[1])
    new, twice_new = build_of(sys.argv[2])
    bad = 0
    for name, a, b in twice_base + twice_new:
        print('TWICE      %s (%s, %s)' % (name, a, b))
        bad += 1
    for name in sorted(set(base) | set(new)):
        if name not in new or name not in base:
            print('%-10s %s' % ('ONLY BASE' if name in base else 'ONLY NEW', name))
            bad += 1
            continue
        (_, (ia, da)), (unit, (ib, db)) = base[name], new[name]
        verdict = 'same' if ia == ib and da == db else 'TEXT' if ia != ib else 'DESCRIPTOR'
        bad += verdict != 'same'
        print('%-10s %-18s %6d lines  %s' % (verdict, unit, len(ib), name))
    print('# %d kernels in the base, %d in the new build, %d differences' % (len(base), len(new), bad))
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
