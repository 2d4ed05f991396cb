"""Compile-time properties of the dark-noise kernels (no GPU needed), from tools/isa_report.sh's table as tests/test_isa_budget.py
reads it: both kernels of kernels_daq_noise.h are in the library, keep nothing in scratch (the Philox block of a word's stream is
picked by selects, never indexed: it stays in registers through the loop over the candidates) and fit the 8 waves per SIMD that
blocks of 256 (their __launch_bounds__) can run at; LDS holds the block's counters only: a count per wave, and in the emit a count
per (wave, run of 256 words) and the block's place behind the cursor."""
import pytest

from test_isa_budget import isa_table          # noqa: F401  (the module-scoped fixture: one run of the report for this file)

KERNELS = ('k_daq_noise_count', 'k_daq_noise_emit')


@pytest.mark.timeout(1000)
def test_the_noise_kernels_run_at_full_occupancy_without_scratch(isa_table):
    for name in KERNELS:
        assert name in isa_table, name
        k = isa_table[name]
        assert k['scratch'] == 0 and k['waves'] == 8, (name, k)


def test_lds_is_the_counters_of_the_block(isa_table):
    lds = {'k_daq_noise_count': 4 * 4, 'k_daq_noise_emit': 4 * 4 + 4 * 4 * 8 + 4}
    for name in KERNELS:
        assert isa_table[name]['lds'] == lds[name], (name, isa_table[name])
