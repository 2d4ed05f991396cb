"""Compile-time properties of the particle stepper's kernels (no GPU needed), from tools/isa_report.sh's table as
tests/test_isa_budget.py reads it: the six kernels of kernels_particles.h are in the library, keep nothing in scratch or LDS, and
have the register counts and occupancies DESIGN 3.8 states.  Only the iteration itself (k_particles_advance: the state, two
points, the Philox block and the table's row pointers live at once) is below the 8 waves per SIMD that blocks of 256 can run at."""
import pytest

from test_isa_budget import isa_table          # noqa: F401  (the module-scoped fixture: one run of the report for this file)

# name -> (VGPRs, waves per SIMD), DESIGN 3.8 "Kernel resources"
KERNELS = {
    'k_particles_rays': (13, 8),
    'k_particles_medium': (25, 8),
    'k_particles_advance': (70, 7),
    'k_particles_counts': (8, 8),
    'k_particles_gather_points': (27, 8),
    'k_particles_gather_segments': (29, 8),
}


@pytest.mark.timeout(1000)
def test_the_stepper_keeps_nothing_in_scratch_or_lds(isa_table):
    for name in KERNELS:
        assert name in isa_table, name
        k = isa_table[name]
        assert k['scratch'] == 0 and k['lds'] == 0, (name, k)


def test_registers_and_occupancy_are_as_documented(isa_table):
    for name, (vgpr, waves) in KERNELS.items():
        k = isa_table[name]
        assert (k['vgpr'], k['waves']) == (vgpr, waves), (name, k)
