"""The track recorder's kernels (chroma_amd/csrc/kernels_tracks.h) as compiled for gfx950 (no GPU needed): streaming
kernels like k_load_working -- nothing in scratch, 8 waves per SIMD.  The family needs device_common.h only, so it is
compiled here on its own, with the flags of chroma_amd/csrc/Makefile, in seconds; tools/isa_report.sh lists the same
kernels as part of chroma_hip.hip."""
import os
import re
import subprocess

import pytest

from conftest import ROOT

HIPCC = '/opt/rocm/bin/hipcc'
KERNELS = ('k_track_row0', 'k_track_step', 'k_track_scatter_row0', 'k_track_scatter')


@pytest.fixture(scope='module')
def track_kernels(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip('hipcc not available')
    tmp = tmp_path_factory.mktemp('isa_tracks')
    src, asm = str(tmp / 'tracks.hip'), str(tmp / 'tracks.s')
    with open(src, 'w') as f:
        f.write('#include "device_common.h"\n#include "kernels_tracks.h"\n')
    subprocess.run([HIPCC, '--offload-arch=gfx950', '-O3', '-fPIC', '-std=c++17', '-ffp-contract=off', '-fno-fast-math',
                    '-fhip-fp32-correctly-rounded-divide-sqrt', '-fno-gpu-flush-denormals-to-zero', '-I', os.path.join(ROOT, 'chroma_amd', 'csrc'),
                    '-S', '--cuda-device-only', '-o', asm, src], check=True, capture_output=True, text=True, timeout=600)
    table, name = {}, None
    for line in open(asm):
        m = re.match(r'^(_Z[A-Za-z0-9_]+):', line)
        if m:
            name = next((k for k in sorted(KERNELS, key=len, reverse=True) if re.match(r'_Z\d+%s[A-Z0-9]' % k, m.group(1))), None)
        for key, field in (('; NumVgprs:', 'vgpr'), ('; ScratchSize:', 'scratch'), ('; LDSByteSize:', 'lds'), ('; Occupancy:', 'waves')):
            if name and line.strip().startswith(key):
                table.setdefault(name, {})[field] = int(line.split()[2])
    return table


def test_track_kernels_stream_at_full_occupancy(track_kernels):
    assert sorted(track_kernels) == sorted(KERNELS), sorted(track_kernels)
    for name in KERNELS:
        k = track_kernels[name]
        assert k['scratch'] == 0 and k['waves'] == 8 and k['vgpr'] <= 64, (name, k)
    # one 4 KB staging area per wave of a 256-thread block where rows leave through LDS, none in the scatter passes
    assert track_kernels['k_track_row0']['lds'] == track_kernels['k_track_step']['lds'] == 4 * 64 * 64
    assert track_kernels['k_track_scatter']['lds'] == track_kernels['k_track_scatter_row0']['lds'] == 0
