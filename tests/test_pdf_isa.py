"""The PDF kernels (chroma_amd/csrc/kernels_pdf.h) as compiled for gfx950: no scratch, full occupancy (8 waves per SIMD).
tools/isa_report.sh is the table; no GPU needed."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

PDF_KERNELS = ('k_pdf_bin_hits', 'k_pdf_eval_hitcount', 'k_pdf_eval_accumulate', 'k_pdf_moments', 'k_pdf_kernel_eval')


@pytest.fixture(scope='module')
def isa_table():
    if not os.path.exists('/opt/rocm/bin/hipcc') or shutil.which('c++filt') is None:
        pytest.skip('hipcc / c++filt not available')
    out = subprocess.run([os.path.join(ROOT, 'tools', 'isa_report.sh')], check=True, capture_output=True, text=True,
                         timeout=900).stdout
    table = {}
    for line in out.splitlines():
        if line.startswith('#') or not line.strip():
            continue
        name, vgpr, sgpr, scratch, lds, waves, code = [x.strip() for x in line.rsplit(',', 6)]
        table[name.replace('void ', '')] = dict(vgpr=int(vgpr), scratch=int(scratch), lds=int(lds), waves=int(waves))
    return table


@pytest.mark.timeout(1000)
@pytest.mark.parametrize('name', PDF_KERNELS)
def test_pdf_kernel_has_no_scratch_and_full_occupancy(isa_table, name):
    assert name in isa_table, name
    k = isa_table[name]
    assert k['scratch'] == 0 and k['waves'] == 8 and k['lds'] == 0, (name, k)
