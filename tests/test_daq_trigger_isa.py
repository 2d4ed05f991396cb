"""Compile-time properties of the DAQ trigger's kernels (no GPU needed), from tools/isa_report.sh's table as
tests/test_isa_budget.py reads it: every kernel of kernels_daq_trigger.h is in the library, keeps nothing in scratch and fits the
8 waves per SIMD that blocks of 256 (its __launch_bounds__) can run at; the kernel that finds the pulses' rows holds in LDS the
two rows that bracket a block, the others nothing (the scans of a row's bins carry from one 64 bins to the next in registers)."""
import pytest

from test_isa_budget import isa_table          # noqa: F401  (the module-scoped fixture: one run of the report for this file)

KERNELS = ('k_daq_trigger_edges', 'k_daq_trigger_count', 'k_daq_trigger_fire', 'k_daq_trigger_gates', 'k_daq_trigger_compact',
           'k_daq_trigger_reduce')


@pytest.mark.timeout(1000)
def test_the_trigger_kernels_run_at_full_occupancy_without_scratch(isa_table):
    for name in KERNELS:
        assert name in isa_table, name
        k = isa_table[name]
        assert k['scratch'] == 0 and k['waves'] == 8, (name, k)


def test_the_edges_keep_two_rows_in_lds_and_the_others_nothing(isa_table):
    lds = {'k_daq_trigger_edges': 4 * 2}
    for name in KERNELS:
        assert isa_table[name]['lds'] == lds.get(name, 0), (name, isa_table[name])
