"""Compile-time properties of the direction seed's kernels (no GPU needed), from tools/isa_report.sh's table as
tests/test_isa_budget.py reads it: the three kernels of kernels_dirseed.h are in the product library, keep nothing in scratch and
stay within 64 vector registers, and a block's LDS of the two 512-thread kernels -- 512 records of 8 bytes, the profile's 256 bytes,
and in the refinement cos_hist's 256 words and the fold's few -- is what DESIGN 3.10 states at the most.  Metadata only."""
import pytest

from test_isa_budget import isa_table          # noqa: F401  (the module-scoped fixture: one run of the report for this file)

KERNELS = ('k_dir_prepare', 'k_dir_scores', 'k_dir_refine')
LDS_BYTES = 5456          # DESIGN 3.10, "Resources": 8 * 512 + 256 + 4 * 256 + 8 * 8 + 16


@pytest.mark.timeout(1000)
def test_the_direction_seed_kernels_are_in_the_library_without_scratch(isa_table):
    for name in KERNELS + ('k_dir_check',):
        assert name in isa_table, name
        assert isa_table[name]['scratch'] == 0, (name, isa_table[name])
    for name in KERNELS:
        assert isa_table[name]['vgpr'] <= 64, (name, isa_table[name])


def test_a_block_of_the_512_thread_kernels_stays_within_its_lds(isa_table):
    assert isa_table['k_dir_prepare']['lds'] == 0
    for name in ('k_dir_scores', 'k_dir_refine'):
        lds = isa_table[name]['lds']
        assert 0 < lds <= LDS_BYTES, (name, lds)
