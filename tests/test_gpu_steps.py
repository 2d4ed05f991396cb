"""Photons from charged-particle steps on the device (chroma_steps_count / chroma_steps_generate) against the host twin,
bit for bit in all ten arrays and in the offsets, at the shapes where counting, scan and search can go wrong; then through
propagate_hits and Simulation.simulate."""
import ctypes

import numpy as np
import pytest

from chroma_amd import _lib, event
from chroma_amd.generator import steps as host
from chroma_amd.geometry import Material, standard_wavelengths

pytestmark = pytest.mark.gpu

SEED = 0x0123456789ABCDEF
WL = standard_wavelengths.astype(np.float64)
FIELDS = ('pos', 'dir', 'pol', 'wavelengths', 't', 'flags', 'last_hit_triangles', 'weights', 'evidx')


@pytest.fixture(scope='module')
def gpu():
    from chroma_amd import gpu as g
    ctx = g.create_cuda_context(0)
    yield g
    ctx.pop()


def medium(light_yield=100.0):
    """Water-like index falling with wavelength, a scintillation spectrum around 430 nm, a two-exponential waveform."""
    m = Material('medium')
    m.set('refractive_index', 1.36 - (WL - 200.0) * 5e-5)
    m.set('absorption_length', 1e6)
    m.set('scattering_length', 1e6)
    m.set('scintillation_spectrum', np.where(np.abs(WL - 430) < 50, 1.0 + np.cos((WL - 430) * np.pi / 50), 0.0))
    m.scintillation_light_yield = light_yield
    t = np.arange(0, 1000, 0.05)
    m.scintillation_waveform = np.column_stack([t, 0.7 * np.exp(-t / 3.0) / 3.0 + 0.3 * np.exp(-t / 12.0) / 12.0])
    return m


@pytest.fixture(scope='module')
def source():
    return host.LightSource(medium(), WL)


def line(n, a, b, t=(0.0, 1.0), beta=0.95, z=1.0, qedep=0.0, evidx=0):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    x = a + (b - a) * np.linspace(0, 1, n + 1)[:, None]
    tt = np.linspace(t[0], t[1], n + 1)
    return host.Segments(x[:-1], x[1:], tt[:-1], tt[1:], beta, z, qedep, evidx)


def stepped_vertex(pdgcode, n, start, direction, ke0, t0=0.0, dedx=0.2, step=5.0):
    direction = np.asarray(direction, dtype=float)
    x = np.asarray(start, dtype=float) + np.linspace(0, step * n, n + 1)[:, None] * direction
    dep = np.concatenate(([0.0], np.full(n, dedx * step)))
    st = event.Steps(x[:, 0], x[:, 1], x[:, 2], t0 + np.arange(n + 1) * step / 299.79, *(np.tile(direction, (n + 1, 1)).T),
                     ke0 - dedx * step * np.arange(n + 1), dep, 0.8 * dep)
    return event.Vertex('particle', start, direction, ke0, t0=t0, steps=st, pdgcode=pdgcode)


def assert_device_equals_host(gpu, segments, source, seed=SEED):
    got, offsets = gpu.steps.generate_photons(segments, source, seed, return_offsets=True)
    want_offsets, total = host.count_photons(segments, source, seed)
    assert np.array_equal(offsets, want_offsets)
    want = host.generate_photons(segments, source, seed)
    assert len(got) == total == len(want)
    have = got.get()
    for name in FIELDS:
        assert np.array_equal(getattr(have, name).view(np.uint32), getattr(want, name).view(np.uint32)), name
    assert not got.rng_counters.get().any()
    return want, want_offsets


def assert_same_hits(a, b):
    """Two sets of flat hits hold the same photons bit for bit.  The order of the hits of one (event, channel) is unspecified
    (the compaction goes through an atomic), so both sets are put in one order first: by every word of the photon."""
    assert len(a) == len(b)

    def ordered(p):
        words = np.column_stack([getattr(p, name).view(np.uint32).reshape(len(p), -1) for name in FIELDS + ('channel',)])
        return words[np.lexsort(words.T[::-1])]
    assert np.array_equal(ordered(a), ordered(b))


def test_no_segments_and_a_segment_without_photons(gpu, source):
    want, offsets = assert_device_equals_host(gpu, host.Segments.join([]), source)
    assert len(want) == 0 and np.array_equal(offsets, [0])
    want, offsets = assert_device_equals_host(gpu, line(1, (0, 0, 0), (0, 0, 0), qedep=0.0), source)
    assert len(want) == 0 and np.array_equal(offsets, [0, 0, 0])


def test_one_segment_across_a_block_and_65536(gpu, source):
    want, offsets = assert_device_equals_host(gpu, line(1, (0, 0, 0), (3, 4, 12), z=0.0, qedep=700.0), source)
    assert 68000 < len(want) < 72000 and (want.flags == event.SCINTILLATION).all()


def test_long_runs_of_empty_segments(gpu, source):
    rng = np.random.default_rng(3)
    n = 3000
    seg = line(n, (-500, 0, 0), (500, 30, -40), z=0.0, qedep=np.where(rng.uniform(size=n) < 0.8, 0.0, rng.uniform(0, 0.03, n)))
    want, offsets = assert_device_equals_host(gpu, seg, source)
    counts = np.diff(offsets.astype(np.int64))
    empty = np.flatnonzero(counts[1::2] == 0)
    assert 200 < len(want) < 2000 and np.diff(empty).tolist().count(1) > 1500 and counts.max() <= 12
    # Cherenkov light with means of 0 to 3 on the same track: both kinds of run interleave
    seg = line(n, (-0.5, 0, 0), (25, 1.5, -2), z=np.where(rng.uniform(size=n) < 0.5, 0.0, 1.0), qedep=rng.uniform(0, 0.03, n))
    want, offsets = assert_device_equals_host(gpu, seg, source)
    assert {event.CHERENKOV, event.SCINTILLATION} == set(np.unique(want.flags))


def test_two_vertices_and_both_count_branches(gpu, source):
    vertices = [stepped_vertex(13, 40, (0, 0, 0), (0, 0.6, 0.8), 300.0), stepped_vertex(-11, 25, (50, 0, -20), (1, 0, 0), 30.0, t0=3.0)]
    seg = host.segments_from_vertices(vertices, evidx=[3, 9], segment_base=123456789012)
    assert len(seg) == 65
    want, offsets = assert_device_equals_host(gpu, seg, source)
    first_of_second = offsets[2 * 40]
    assert (want.evidx[:first_of_second] == 3).all() and (want.evidx[first_of_second:] == 9).all() and 0 < first_of_second < len(want)
    # no segment spans the joint: every photon lies within 5 mm of its own vertex's line
    assert np.abs(want.pos[:first_of_second, 0]).max() < 1e-3 and np.abs(want.pos[first_of_second:, 1]).max() < 1e-3
    # means either side of 16: 0.15 and 0.17 of deposit at 100 photons a unit, Cherenkov means of ~15 and ~17 from the lengths
    mean_per_mm = source.expected_photons(line(1, (0, 0, 0), (1, 0, 0)))
    parts = [line(200, (0, 0, 0), (200 * m / mean_per_mm, 0, 0), qedep=q) for m, q in ((15.0, 0.15), (17.0, 0.17))]
    want, offsets = assert_device_equals_host(gpu, host.Segments.join(parts), source)
    counts = np.diff(offsets.astype(np.int64))
    assert 14 < counts[:400].mean() < 16 and 16 < counts[400:].mean() < 18


def test_capacity_one_short_is_an_error_and_nothing_is_written(gpu, source):
    ctx = gpu.get_context()
    seg = line(30, (0, 0, 0), (30, 0, 0), qedep=0.2)
    want = host.generate_photons(seg, source, SEED)
    n, guard = len(want), 64
    device = {name: gpu.to_gpu(getattr(seg, name).reshape(-1), ctx) for name in ('a', 'b', 't_a', 't_b', 'beta', 'z', 'qedep', 'evidx')}
    s = seg.struct({name: a.ptr for name, a in device.items()})
    d_offsets = gpu.empty(2 * len(seg) + 1, np.uint32, ctx)
    total = ctypes.c_uint64()
    _lib.check(ctx._lib.chroma_steps_count(ctx.handle, ctypes.byref(source.struct), ctypes.byref(s), SEED, d_offsets.ptr, ctypes.byref(total)))
    assert total.value == n > 256
    arrays, dev = _lib.PhotonArrays(), {}
    for name, width in (('pos', 3), ('dir', 3), ('pol', 3), ('wavelengths', 1), ('t', 1), ('flags', 1), ('last_hit_triangles', 1),
                        ('weights', 1), ('evidx', 1), ('rng_counters', 1)):
        dev[name] = gpu.GPUArray((n + guard) * width, np.uint32, ctx).fill(0xDEADBEEF)
        setattr(arrays, name, dev[name].ptr)
    rc = ctx._lib.chroma_steps_generate(ctx.handle, ctypes.byref(source.struct), ctypes.byref(s), SEED, d_offsets.ptr, ctypes.byref(arrays), n - 1)
    assert rc == -1 and b'room for' in ctx._lib.chroma_last_error()
    ctx.synchronize()
    assert all((a.get() == 0xDEADBEEF).all() for a in dev.values())
    _lib.check(ctx._lib.chroma_steps_generate(ctx.handle, ctypes.byref(source.struct), ctypes.byref(s), SEED, d_offsets.ptr, ctypes.byref(arrays), n))
    ctx.synchronize()
    for name, a in dev.items():
        got = a.get()
        width = len(got) // (n + guard)
        assert (got[n * width:] == 0xDEADBEEF).all(), name                      # the guard words behind the photons
        if name != 'rng_counters':
            assert np.array_equal(got[:n * width], getattr(want, name).view(np.uint32).reshape(-1)), name


def test_generated_photons_propagate_like_the_host_twins(gpu, tiny_geometry, source):
    """generate_photons + propagate_hits on the device against the host twin's photons uploaded and propagated by the same
    call: the same hits bit for bit, each with the bit of the process that made it."""
    detector = gpu.GPUDetector(tiny_geometry)
    vertices = [stepped_vertex(13, 60, (-150, 20, 0), (1, 0, 0), 400.0), stepped_vertex(11, 20, (0, 0, 300), (0, 0.6, -0.8), 25.0, t0=1.0)]
    seg = host.segments_from_vertices(vertices, evidx=[0, 1])
    hits = []
    for photons in (gpu.steps.generate_photons(seg, source, SEED), gpu.GPUPhotons(host.generate_photons(seg, source, SEED))):
        hits.append(photons.propagate_hits(detector, _lib.Rng(99, 0), max_steps=100, sort=True))
    a, b = hits
    assert len(a) > 100
    assert_same_hits(a, b)
    made_by = a.flags & (event.CHERENKOV | event.SCINTILLATION)
    assert set(np.unique(made_by)) == {event.CHERENKOV, event.SCINTILLATION} and (a.flags & event.SURFACE_DETECT).all()


def stepped_events():
    return [event.Event(vertices=[stepped_vertex(13, 30, (0, -100, 0), (0, 1, 0), 300.0)]),
            event.Event(vertices=[stepped_vertex(11, 10, (40, 0, 0), (0, 0, 1), 20.0), stepped_vertex(-11, 12, (40, 0, 0), (0, 0, -1), 20.0, t0=0.5)]),
            event.Event(vertices=[stepped_vertex(2212, 8, (0, 0, -50), (0.6, 0.8, 0), 900.0, dedx=0.5)])]


def test_simulation_takes_events_with_steps(gpu, tiny_geometry):
    """Three events with stepped vertices through Simulation.simulate against the same events given photons_beg by the host
    generator (same seed, the segments numbered on through the events)."""
    from chroma_amd.sim import Simulation
    light = medium(light_yield=200.0)
    sim = Simulation(tiny_geometry, seed=41, light_medium=light)
    got = list(sim.simulate(stepped_events(), keep_photons_beg=True, max_steps=100))
    src = host.LightSource(light)
    with_photons, base = [], 0
    for ev in stepped_events():
        seg = host.segments_from_vertices(ev.vertices, segment_base=base)
        base += len(seg)
        with_photons.append(event.Event(vertices=ev.vertices, photons_beg=host.generate_photons(seg, src, 41)))
    want = list(Simulation(tiny_geometry, seed=41).simulate(with_photons, keep_photons_beg=True, max_steps=100))
    assert len(got) == len(want) == 3
    for g, w in zip(got, want):
        assert g.id == w.id and g.nphotons == w.nphotons == len(g.photons_beg) > 500
        for name in FIELDS:
            assert np.array_equal(getattr(g.photons_beg, name).view(np.uint32), getattr(w.photons_beg, name).view(np.uint32)), name
        assert len(g.flat_hits) > 20
        assert_same_hits(g.flat_hits, w.flat_hits)
        assert sorted(g.hits) == sorted(w.hits)
    # photons_beg is fetched only when asked for, and the detector's own material is the default medium (water: Cherenkov light)
    plain = list(Simulation(tiny_geometry, seed=41).simulate(stepped_events()[:1], max_steps=100))
    assert plain[0].photons_beg is None and plain[0].nphotons > 500 and (plain[0].flat_hits.flags & event.CHERENKOV).all()


def test_events_with_photons_and_the_refusals_are_as_before(gpu, tiny_geometry, oracle_mod):
    from chroma_amd.sim import Simulation
    bomb = oracle_mod.generate_bomb(20000, seed=4)
    as_photons = list(Simulation(tiny_geometry, seed=5).simulate(bomb, max_steps=100))[0]
    as_event = list(Simulation(tiny_geometry, seed=5).simulate([event.Event(photons_beg=bomb)], max_steps=100))[0]
    assert len(as_event.flat_hits) > 0 and as_event.nphotons == 20000
    assert_same_hits(as_event.flat_hits, as_photons.flat_hits)
    # ... and they are the hits of the propagate call itself
    direct = gpu.GPUPhotons(bomb).propagate_hits(gpu.GPUDetector(tiny_geometry), gpu.get_rng_states(1, seed=5), max_steps=100, sort=True)
    assert_same_hits(as_event.flat_hits, direct)
    sim = Simulation(tiny_geometry, seed=5)
    bare = event.Vertex('mu-', (0, 0, 0), (0, 0, 1), 100.0, pdgcode=13)
    with pytest.raises(NotImplementedError, match='events without photons'):
        list(sim.simulate([event.Event(vertices=[bare])]))
    with pytest.raises(NotImplementedError, match='Vertex input'):
        list(sim.simulate([bare]))
