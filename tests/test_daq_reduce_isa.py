"""Compile-time properties of the trace reduction's kernels (no GPU needed), from tools/isa_report.sh's table as
tests/test_isa_budget.py reads it: both kernels of kernels_daq_reduce.h are in the library, keep nothing in scratch and fit the 8
waves per SIMD that blocks of 256 (their __launch_bounds__) can run at; they hold nothing in LDS, as DESIGN 3.6f states (the runs
are found in scalar registers from ballots, the sums go across the wave lane to lane)."""
import pytest

from test_isa_budget import isa_table          # noqa: F401  (the module-scoped fixture: one run of the report for this file)

KERNELS = ('k_daq_reduce_count', 'k_daq_reduce_fill')
LDS_BYTES = 0          # DESIGN 3.6f, "Resources"


@pytest.mark.timeout(1000)
def test_the_reduction_runs_at_full_occupancy_without_scratch(isa_table):
    for name in KERNELS:
        assert name in isa_table, name
        k = isa_table[name]
        assert k['scratch'] == 0 and k['waves'] == 8 and k['vgpr'] <= 64, (name, k)


def test_the_reduction_holds_nothing_in_lds(isa_table):
    for name in KERNELS:
        assert isa_table[name]['lds'] == LDS_BYTES, (name, isa_table[name])
