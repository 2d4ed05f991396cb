"""The HIP engine against the reference's OWN physics sources, bit for bit, with the CPU oracle not in the chain.

The comparand is oracle/_ref/libchroma_ref_physics_contract.so alone: chroma/cuda/propagate.cu and photon.h compiled for the host
(oracle/ref_physics_driver.cc) with their transcendental calls mapped onto include/chroma_math.h, driven by the reference's own
host loop.  Nothing here reads the reference tree.  tests/test_ref_physics_host.py holds the oracle to the same library on the CPU;
this file closes the triangle on the GPU: 8000 photons (below 8192: the one-launch tail from step 0) and 20000 (one step per
launch first), plain and weighted, through GPUPhotons.propagate and through the fused propagate_hits, on demo.tiny(), the stress
cube and one random-optics cube.  All nine photon fields and the draw counters, bit for bit (two NaNs count as equal); the flat
hits of the fused call are the ones derived from the reference's end state.
"""
import functools
import os

import numpy as np
import pytest

from chroma_amd import event
from conftest import ROOT, bomb
from test_ref_physics_host import assert_same, world
from test_gpu_hits import fetch
from test_gpu_hits_oracle import Expected, derive_hits, assert_hits, channel_arrays

REF_LIB = os.path.join(ROOT, 'oracle', '_ref', 'libchroma_ref_physics_contract.so')
pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not os.path.exists(REF_LIB), reason='oracle/_ref holds no physics library (needs the reference tree at build time)')]

SEED = 13
MAX_STEPS = 100


@pytest.fixture(scope='module')
def gpu():
    from chroma_amd import gpu as g
    ctx = g.create_cuda_context(0)
    yield g
    ctx.pop()


@functools.lru_cache(maxsize=None)
def reference(geometry_name, n, use_weights):
    """The reference's end state, computed once per input and shared by the two engine paths."""
    import oracle
    geometry, packed = world(geometry_name)
    ph = bomb(n, 19, wavelength=300.0, wavelength_hi=700.0)
    end, counters, stats = oracle.ref_propagate(packed, ph, seed=SEED, max_steps=MAX_STEPS, use_weights=use_weights, variant='contract')
    return ph, Expected(end, counters, stats['launches'], *derive_hits(geometry, end, counters))


@pytest.fixture(scope='module')
def detector(gpu):
    """GPUDetector by geometry name, made once each; released before the context goes."""
    made = {}

    def get(geometry_name):
        if geometry_name not in made:
            made[geometry_name] = gpu.GPUDetector(world(geometry_name)[0])
        return made[geometry_name]
    yield get
    made.clear()


@pytest.mark.parametrize('use_weights', [False, True], ids=['plain', 'weights'])
@pytest.mark.parametrize('n', [8000, 20000])
@pytest.mark.parametrize('geometry_name', ['tiny', 'stress', 'optics101'])
def test_propagate_is_the_reference(gpu, detector, geometry_name, n, use_weights):
    ph, want = reference(geometry_name, n, use_weights)
    gg = detector(geometry_name)
    gp = gpu.GPUPhotons(ph)
    stats = {}
    gp.propagate(gg, gpu.get_rng_states(64 * 1024, seed=SEED), max_steps=MAX_STEPS, use_weights=use_weights, stats=stats)
    what = '%s, %d photons, weights %s' % (geometry_name, n, use_weights)
    assert_same(gp.get(), want.end, gp.rng_counters.get(), want.counters, what)
    assert stats['launches'] == want.launches, '%s: %d launches, the reference %d' % (what, stats['launches'], want.launches)
    assert want.launches == 1 if (n < 8192 or use_weights) else want.launches > 1
    assert int(np.bitwise_or.reduce(want.end.flags)) & 0x1FE and want.counters.max() > 0


@pytest.mark.parametrize('use_weights', [False, True], ids=['plain', 'weights'])
@pytest.mark.parametrize('n', [8000, 20000])
@pytest.mark.parametrize('geometry_name', ['tiny', 'stress', 'optics101'])
def test_propagate_hits_is_the_reference(gpu, detector, geometry_name, n, use_weights):
    from chroma_amd import _lib
    ph, want = reference(geometry_name, n, use_weights)
    gg = detector(geometry_name)
    gp = gpu.GPUPhotons(ph)
    counts, earliest = channel_arrays(gpu, gg)
    stats = {}
    found = gp.propagate_hits(gg, _lib.Rng(SEED, 0), max_steps=MAX_STEPS, use_weights=use_weights, channel_arrays=(counts, earliest),
                              stats=stats, device=True)
    what = '%s, %d photons, weights %s, fused' % (geometry_name, n, use_weights)
    assert_same(gp.get(), want.end, gp.rng_counters.get(), want.counters, what)
    assert stats['launches'] == want.launches, '%s: %d launches, the reference %d' % (what, stats['launches'], want.launches)
    assert want.nhits > 20 and stats['nhits'] == want.nhits, '%s: nhits %d, derived from the reference %d' % (what, stats['nhits'], want.nhits)
    assert_hits(*fetch(*found), want, what)
    assert np.array_equal(counts.get(), want.counts) and np.array_equal(earliest.get(), want.earliest), what
    assert (want.hits.flags & event.SURFACE_DETECT).all()
