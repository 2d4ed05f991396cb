"""Compile-time properties of the time-binned DAQ's kernels (no GPU needed), from tools/isa_report.sh's table as
tests/test_isa_budget.py reads it: every kernel of kernels_daq_pulses.h is in the library, keeps nothing in scratch and fits the
8 waves per SIMD that blocks of 256 (its __launch_bounds__) can run at; the two kernels that walk the photons hold in LDS the two
rows that bracket a block and a word per wave and kind of count (the emit: the block's place among the accepted photons too),
the others nothing."""
import pytest

from test_isa_budget import isa_table          # noqa: F401  (the module-scoped fixture: one run of the report for this file)

KERNELS = ('k_daq_pulses_count', 'k_daq_pulses_emit', 'k_daq_pulses_heads', 'k_daq_pulses_open', 'k_daq_pulses_reduce', 'k_daq_pulses_finish')


@pytest.mark.timeout(1000)
def test_the_pulse_kernels_run_at_full_occupancy_without_scratch(isa_table):
    for name in KERNELS:
        assert name in isa_table, name
        k = isa_table[name]
        assert k['scratch'] == 0 and k['waves'] == 8, (name, k)


def test_the_photon_kernels_keep_rows_and_counts_in_lds_and_the_others_nothing(isa_table):
    lds = {'k_daq_pulses_count': 4 * (2 + 4), 'k_daq_pulses_emit': 4 * (2 + 3 * 4 + 1)}          # (four waves to a block)
    for name in KERNELS:
        assert isa_table[name]['lds'] == lds.get(name, 0), (name, isa_table[name])
