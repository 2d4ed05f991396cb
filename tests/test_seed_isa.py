"""Compile-time properties of the vertex seed's kernels (no GPU needed), from tools/isa_report.sh's table as tests/test_isa_budget.py
reads it: both kernels of kernels_seed.h are in the product library, keep nothing in scratch, and a block's LDS -- eight histograms
of 1024 + 16 words, 512 staged hits of five words, the shape and the refinement's few words -- is what DESIGN 3.9 states at the
most, so that three blocks fit a CU's 160 KiB (two are asked for)."""
import pytest

from test_isa_budget import isa_table          # noqa: F401  (the module-scoped fixture: one run of the report for this file)

KERNELS = ('k_seed_scores', 'k_seed_refine')
LDS_BYTES = 43712          # DESIGN 3.9, "Resources": 4 * (8 * 1040 + 5 * 512 + 16 + 32)


@pytest.mark.timeout(1000)
def test_the_seed_kernels_are_in_the_library_without_scratch(isa_table):
    for name in KERNELS + ('k_seed_check',):
        assert name in isa_table, name
        assert isa_table[name]['scratch'] == 0, (name, isa_table[name])
    for name in KERNELS:
        assert isa_table[name]['waves'] >= 4 and isa_table[name]['vgpr'] <= 64, (name, isa_table[name])          # (512 threads a block: two waves per SIMD each, two blocks a CU)


def test_a_block_of_the_seed_kernels_fits_a_cu_three_times(isa_table):
    for name in KERNELS:
        lds = isa_table[name]['lds']
        assert 0 < lds <= LDS_BYTES <= 65536 and 3 * LDS_BYTES <= 160 * 1024, (name, lds)
