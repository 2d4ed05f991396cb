#!/usr/bin/env python
"""The loop bodies of k_raycast_quad<false> as compiled for gfx950, cut into phases, with their instructions counted by class
(no GPU needed: hipcc cross-compiles):

    tools/quad_isa_phases.py > profiles/rNN/isa_quad_after.txt        # compiles chroma_amd/csrc/chroma_hip.hip (a minute)
    tools/quad_isa_phases.py --asm chroma_hip.s                        # or reads an assembly file made with the Makefile's flags
    tools/quad_isa_phases.py --counts                                  # the counts alone, one JSON object

The phases are cut at instructions the kernel's source puts there on purpose, so the cut does not depend on block numbers:

    pop          s_setprio 3 (a node-loop iteration begins) .. the block that fetches the node (it ends in s_setprio 0)
    node_visit   that block .. the wave barrier behind the node loop: the slab tests, the decision word, the ring write, the
                 choice of the nearest child, BOTH arms of the push (the arm through the spill area runs for a few rays in 1e8)
                 and the loop control
    round        the wave barrier .. the first global store behind it (the retirement): the triangle round and its loop control

The counts are static: every instruction of the region once, whatever the branches do.  tests/test_isa_quad_slots.py holds them
against the committed listing."""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (the device flags of chroma_amd/csrc/Makefile, as tools/isa_report.sh has them)
FLAGS = ['--offload-arch=gfx950', '-O3', '-fPIC', '-std=c++17', '-ffp-contract=off', '-fno-fast-math',
         '-fhip-fp32-correctly-rounded-divide-sqrt', '-fno-gpu-flush-denormals-to-zero', '-Wno-unused-value', '-Wno-unused-result']
KERNEL = re.compile(r'^(_Z14k_raycast_quadILb0E\w*):')
PHASES = ('pop', 'node_visit', 'round')
CLASSES = ('total', 'valu', 'dpp', 'dpp_mov', 'v_mov', 's_nop', 'wait_states', 'lds', 'vmem', 'salu', 'branch', 'waitcnt')


def compile_asm(extra=()):
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, 'chroma_hip.s')
        subprocess.run(['/opt/rocm/bin/hipcc'] + FLAGS + list(extra) + ['-S', '--cuda-device-only', '-o', out,
                        os.path.join(ROOT, 'chroma_amd', 'csrc', 'chroma_hip.hip')], check=True, stderr=subprocess.DEVNULL)
        return open(out).read()


def kernel_lines(asm):
    lines = asm.splitlines()
    start = next(k for k, line in enumerate(lines) if KERNEL.match(line))
    end = next(k for k in range(start, len(lines)) if lines[k].strip() == 's_endpgm')
    return lines[start:end + 1]


def is_instruction(line):
    s = line.strip()
    return line.startswith('\t') and s and s[0] not in '.;'


def cut(lines):
    """{phase: its lines}.  Every anchor must be there exactly as often as the source puts it."""
    def find(text, begin=0):
        return next(k for k in range(begin, len(lines)) if lines[k].strip() == text)
    prio3 = find('s_setprio 3')
    prio0 = find('s_setprio 0', prio3)
    assert sum(line.strip() == 's_setprio 3' for line in lines) == 1 and sum(line.strip() == 's_setprio 0' for line in lines) == 1
    fetch = max(k for k in range(prio3, prio0) if lines[k].startswith('.LBB'))         # the label of the block that fetches
    barrier = find('; wave barrier', prio0)
    retire = next(k for k in range(barrier, len(lines)) if lines[k].strip().startswith('global_store_dword'))
    return {'pop': lines[prio3:fetch], 'node_visit': lines[fetch:barrier], 'round': lines[barrier + 1:retire]}


def count(lines):
    c = dict.fromkeys(CLASSES, 0)
    for line in lines:
        if not is_instruction(line):
            continue
        text = line.split(';')[0].strip()
        op = text.split()[0]
        c['total'] += 1
        if op == 's_nop':
            c['s_nop'] += 1
            c['wait_states'] += int(text.split()[1]) + 1
        elif op.startswith('v_'):
            c['valu'] += 1
            c['dpp'] += 'dpp' in op or 'quad_perm' in text or 'row_' in text.replace('row_mask', '')
            c['dpp_mov'] += op == 'v_mov_b32_dpp'
            c['v_mov'] += op.startswith('v_mov_b32_e')
        elif op.startswith('ds_'):
            c['lds'] += 1
        elif op.split('_')[0] in ('global', 'buffer', 'flat', 'scratch'):
            c['vmem'] += 1
        elif op in ('s_branch',) or op.startswith('s_cbranch'):
            c['branch'] += 1
        elif op == 's_waitcnt':
            c['waitcnt'] += 1
        else:
            c['salu'] += 1
    return c


def phase_counts(asm):
    phases = cut(kernel_lines(asm))
    return phases, {name: count(phases[name]) for name in PHASES}


def parse_header(text):
    """The counts back out of a listing this tool wrote: {phase: {class: n}}."""
    found = {}
    for line in text.splitlines():
        m = re.match(r'^# (\w+): (.*)$', line)
        if m and m.group(1) in PHASES:
            found[m.group(1)] = {k: int(v) for k, v in (kv.split('=') for kv in m.group(2).split())}
    return found


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--asm', default=None, help='an assembly file of chroma_hip.hip (default: compile it)')
    ap.add_argument('--counts', action='store_true', help='print the counts as JSON, no listing')
    args, extra = ap.parse_known_args()
    asm = open(args.asm).read() if args.asm else compile_asm(extra)
    phases, counts = phase_counts(asm)
    if args.counts:
        print(json.dumps(counts))
        return
    print('# k_raycast_quad<false>, gfx950, hipcc -O3 (flags of chroma_amd/csrc/Makefile), cut by tools/quad_isa_phases.py: static')
    print('# instruction counts per phase (dpp, dpp_mov -- a DPP step left as a move -- and v_mov are among valu; wait_states: the cycles the s_nop ask for)')
    for name in PHASES:
        print('# %s: %s' % (name, ' '.join('%s=%d' % (k, counts[name][k]) for k in CLASSES)))
    for name in PHASES:
        print('\n# ---- %s' % name)
        print('\n'.join(phases[name]))


if __name__ == '__main__':
    sys.exit(main())
