"""Compile-time properties of the DAQ digitiser's kernel (no GPU needed), from tools/isa_report.sh's table as
tests/test_isa_budget.py reads it: the kernel of kernels_daq_digitize.h is in the library, keeps nothing in scratch and fits the
8 waves per SIMD that blocks of 256 (its __launch_bounds__) can run at; it holds in LDS the tap table of 1024 words and nothing
else (the pulses go round a wave through v_readlane, the sums stay in registers)."""
import pytest

from test_isa_budget import isa_table          # noqa: F401  (the module-scoped fixture: one run of the report for this file)

KERNELS = ('k_daq_digitize',)


@pytest.mark.timeout(1000)
def test_the_digitiser_runs_at_full_occupancy_without_scratch(isa_table):
    for name in KERNELS:
        assert name in isa_table, name
        k = isa_table[name]
        assert k['scratch'] == 0 and k['waves'] == 8 and k['vgpr'] <= 64, (name, k)


def test_the_digitiser_keeps_the_tap_table_in_lds_and_nothing_else(isa_table):
    for name in KERNELS:
        assert isa_table[name]['lds'] == 4 * 1024, (name, isa_table[name])
