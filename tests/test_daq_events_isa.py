"""Compile-time properties of the batch DAQ's kernels (no GPU needed), from tools/isa_report.sh's table as
tests/test_isa_budget.py reads it: k_run_daq_events keeps no scratch and fits 8 waves per SIMD, like k_run_daq; the two
compaction kernels are in the library, without scratch."""
import pytest

from test_isa_budget import isa_table          # noqa: F401  (the module-scoped fixture: one run of the report for this file)


@pytest.mark.timeout(1000)
def test_the_batch_acquire_runs_at_full_occupancy_without_scratch(isa_table):
    k = isa_table['k_run_daq_events']
    assert k['scratch'] == 0 and k['waves'] == 8, k
    # the two rows a block brackets its photons with: two words of LDS, nothing else
    assert k['lds'] == 8, k
    assert isa_table['k_run_daq']['scratch'] == 0 and isa_table['k_run_daq']['waves'] == 8


def test_the_compaction_kernels_are_there_without_scratch(isa_table):
    for name in ('k_daq_events_flag', 'k_daq_events_scatter'):
        assert name in isa_table, name
        assert isa_table[name]['scratch'] == 0, (name, isa_table[name])
