"""The triangle round of the default ray cast as compiled for gfx950 (no GPU needed): the Moeller-Trumbore over the
48-byte intersection record (intersect_triangle_edges, csrc/propagate_device.h) fetches its record with three vector
loads at the record's three 16-byte offsets, and the round stays near the instruction count it was built for.

The round is the innermost loop of k_raycast_quad<false> that holds the division's v_div_fixup_f32: every basic block
the compiler annotates as part of that loop.  It issued 114 VALU with the 48-byte vertex record (26 of them register
copies, 5 loads per test) and 85 with the edge form; the bound below leaves room for compiler drift, not for the operand
shuffles of the vertex form to come back."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

ROUND_VALU_MAX = 92
ROUND_COPIES_MAX = 12


@pytest.fixture(scope='module')
def quad_round(tmp_path_factory):
    hipcc = '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc) or shutil.which('c++filt') is None:
        pytest.skip('hipcc / c++filt not available')
    out = str(tmp_path_factory.mktemp('isa') / 'k.s')
    # the flags of chroma_amd/csrc/Makefile (and tools/isa_report.sh)
    subprocess.run([hipcc, '--offload-arch=gfx950', '-O3', '-fPIC', '-std=c++17', '-ffp-contract=off', '-fno-fast-math',
                    '-fhip-fp32-correctly-rounded-divide-sqrt', '-fno-gpu-flush-denormals-to-zero', '-Wno-unused-value',
                    '-Wno-unused-result', '-S', '--cuda-device-only', '-o', out,
                    os.path.join(ROOT, 'chroma_amd', 'csrc', 'chroma_hip.hip')], check=True, capture_output=True, timeout=900)
    lines = open(out).read().split('\n')
    begin = end = None
    for i, line in enumerate(lines):
        m = re.match(r'^([_A-Za-z0-9]+):\s*; @', line)
        if not m:
            continue
        if begin is not None:
            end = i
            break
        name = subprocess.run(['c++filt', m.group(1)], capture_output=True, text=True).stdout.strip()
        if name.startswith('void k_raycast_quad<false>('):
            begin = i
    assert begin is not None, 'k_raycast_quad<false> not found'
    blocks, cur = [], None
    for line in lines[begin:end]:
        m = re.match(r'^(\.LBB\d+_\d+):(.*)$', line) or re.match(r'^; %(bb\.\d+):(.*)$', line)
        if m:
            cur = dict(name=m.group(1), note=m.group(2), ins=[])
            blocks.append(cur)
        elif cur is not None and line.startswith('\t') and not line.strip().startswith(('.', ';')):
            cur['ins'].append(line.split(';')[0].strip())
    div = [b for b in blocks if any(i.startswith('v_div_fixup_f32') for i in b['ins'])]
    assert len(div) == 1, 'one division in the kernel: the triangle test'
    m = re.search(r'Header=BB(\d+_\d+) Depth=\d+', div[0]['note'])
    header = m.group(1) if m else div[0]['name'][len('.LBB'):]
    loop = [b for b in blocks if b['name'] == '.LBB' + header or re.search(r'Header=BB%s\b' % header, b['note'])]
    return [i for b in loop for i in b['ins']]


@pytest.mark.timeout(1000)
def test_round_fetches_the_record_with_three_loads(quad_round):
    loads = [i for i in quad_round if re.match(r'(global|buffer|flat)_load_', i)]
    offsets = sorted(int(re.search(r'offset:(\d+)', i).group(1)) if 'offset:' in i else 0 for i in loads)
    assert offsets == [0, 16, 32], loads
    assert all(i.startswith(('global_load_dwordx4', 'global_load_dwordx2')) for i in loads), loads
    assert sum(i.startswith('global_load_dwordx4') for i in loads) >= 2, loads


@pytest.mark.timeout(1000)
def test_round_valu_count(quad_round):
    valu = [i for i in quad_round if i.startswith('v_')]
    copies = [i for i in valu if i.split()[0] in ('v_mov_b32_e32', 'v_mov_b32_e64', 'v_pk_mov_b32')]
    packed = [i for i in valu if i.startswith(('v_pk_mul_f32', 'v_pk_add_f32'))]
    assert len(valu) <= ROUND_VALU_MAX, (len(valu), len(copies))
    assert len(copies) <= ROUND_COPIES_MAX, copies
    # the two cross products and the four dot products run as pairs: 12 packed multiplies, 7 packed adds (and u + v)
    assert len(packed) >= 18, packed
    # no contraction: the only fused operations are the correctly rounded division's own
    assert not any(i.startswith('v_pk_fma_f32') for i in valu), 'a packed fma in the triangle round'
