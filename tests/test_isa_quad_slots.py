"""The issue slots of k_raycast_quad's loop bodies as compiled (no GPU needed: hipcc cross-compiles gfx950), held against the
listing committed with the change that removed some: profiles/r22/isa_quad_after.txt, written by tools/quad_isa_phases.py.
The ray cast's time is VALU issue, so a copy, an old-value initialisation or an unfolded DPP move
that comes back costs time without failing any other test.  Instructions are counted by class only; two of a class may
come and go with the compiler."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT

MARGIN = 2
TOOL = os.path.join(ROOT, 'tools', 'quad_isa_phases.py')
LISTING = os.path.join(ROOT, 'profiles', 'r22', 'isa_quad_after.txt')


@pytest.fixture(scope='module')
def counts():
    if not os.path.exists('/opt/rocm/bin/hipcc'):
        pytest.skip('hipcc not available')
    out = subprocess.run([sys.executable, TOOL, '--counts'], check=True, capture_output=True, text=True, timeout=900).stdout
    return json.loads(out)


@pytest.fixture(scope='module')
def recorded():
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    try:
        import quad_isa_phases
    finally:
        sys.path.pop(0)
    return quad_isa_phases.parse_header(open(LISTING).read())


@pytest.mark.timeout(1000)
@pytest.mark.parametrize('phase', ['node_visit', 'round'])
def test_the_loop_bodies_are_no_longer_than_recorded(counts, recorded, phase):
    now, then = counts[phase], recorded[phase]
    print(phase, 'now', now, 'recorded', then)
    for what in ('total', 'valu', 'v_mov', 's_nop', 'wait_states', 'lds'):
        assert now[what] <= then[what] + MARGIN, (phase, what, now, then)


@pytest.mark.timeout(1000)
def test_the_quad_reductions_are_dpp_operations_on_the_value(counts, recorded):
    """Six reductions of two steps each (the decision word, the nearest child's key and its node; the nearest hit, its rank
    and its triangle): twelve DPP instructions, none of them a v_mov_b32_dpp -- a step the combiner did not fold into its
    consumer (its old-value initialisation would show as a plain v_mov, held above)."""
    for phase in ('node_visit', 'round'):
        assert recorded[phase]['dpp'] == 6 and recorded[phase]['dpp_mov'] == 0
        assert counts[phase]['dpp'] == 6 and counts[phase]['dpp_mov'] == 0, (phase, counts[phase])
