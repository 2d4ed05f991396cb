"""The hybrid render's kernels (chroma_amd/csrc/kernels_hybrid_render.h) as compiled for gfx950, and the promise that adding
them changes no other kernel: tools/isa_report.sh with and without the family (-DCHROMA_HYBRID_RENDER=0) must list every
other kernel with the same registers, scratch, LDS, occupancy and code size.  No GPU needed."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

HYBRID = ('k_hybrid_lookup<24>', 'k_hybrid_image<24>', 'k_hybrid_reduce', 'k_hybrid_pixels')


def _report(*flags):
    out = subprocess.run([os.path.join(ROOT, 'tools', 'isa_report.sh')] + list(flags), check=True, capture_output=True, text=True,
                         timeout=900).stdout
    table = {}
    for line in out.splitlines():
        if line.startswith('#') or not line.strip():
            continue
        name, vgpr, sgpr, scratch, lds, waves, code = [x.strip() for x in line.rsplit(',', 6)]
        table[name.replace('void ', '')] = dict(vgpr=int(vgpr), sgpr=int(sgpr), scratch=int(scratch), lds=int(lds), waves=int(waves),
                                                code=int(code))
    return table


@pytest.fixture(scope='module')
def tables():
    if not os.path.exists('/opt/rocm/bin/hipcc') or shutil.which('c++filt') is None:
        pytest.skip('hipcc / c++filt not available')
    return _report(), _report('-DCHROMA_HYBRID_RENDER=0')


@pytest.mark.timeout(2000)
def test_hybrid_kernel_resources(tables):
    with_hybrid, _ = tables
    for name in HYBRID:
        assert name in with_hybrid, name
    k = with_hybrid['k_hybrid_pixels']
    assert k['scratch'] == 0 and k['waves'] == 8, k
    assert with_hybrid['k_hybrid_reduce']['scratch'] == 0
    prop = with_hybrid['k_propagate<24, false>']
    for name in ('k_hybrid_lookup<24>', 'k_hybrid_image<24>'):
        k = with_hybrid[name]
        assert k['waves'] >= prop['waves'] and k['scratch'] <= prop['scratch'], (name, k, prop)


@pytest.mark.timeout(2000)
def test_no_other_kernel_changes(tables):
    with_hybrid, without = tables
    assert len(without) > 50
    assert set(with_hybrid) - set(without) == set(HYBRID)
    for name, row in without.items():
        assert with_hybrid[name] == row, (name, row, with_hybrid[name])
