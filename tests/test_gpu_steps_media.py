"""Photons from charged-particle steps with a medium per segment on the device (chroma_steps_count_media /
chroma_steps_generate_media) against the host twin, bit for bit in all ten arrays and in the offsets; then with the media
located in the geometry on the device, and through Simulation(light_medium='located')."""
import ctypes

import numpy as np
import pytest

from chroma_amd import _lib, event
from chroma_amd.generator import steps as host

from test_steps_media_host import SEED, WL, material, mixed_medium, mixed_segments, three_media, assert_same_photons
from test_gpu_locate import INNER, OUTER, nested_boxes

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def gpu():
    from chroma_amd import gpu as g
    ctx = g.create_cuda_context(0)
    yield g
    ctx.pop()


@pytest.fixture(scope='module')
def media():
    return three_media()


def assert_device_equals_host(gpu, segments, media, medium, **kwargs):
    got, offsets = gpu.steps.generate_photons(segments, media, SEED, medium=medium, return_offsets=True, **kwargs)
    want_offsets, total = host.count_photons(segments, media, SEED, medium=medium)
    assert np.array_equal(offsets, want_offsets)
    want = host.generate_photons(segments, media, SEED, medium=medium)
    assert len(got) == total == len(want)
    assert_same_photons(got.get(), want)
    assert not got.rng_counters.get().any()
    return want, want_offsets


@pytest.mark.parametrize('n', (0, 1, 255, 256, 257, 1025))
def test_device_equals_host_twin(gpu, media, n):
    seg, medium = mixed_segments(n, seed=n + 1), mixed_medium(n, seed=n + 2)
    if n == 1:
        medium[:] = 1                # one segment, more than three blocks of photons
        seg = host.Segments(seg.a, seg.b, seg.t_a, seg.t_b, seg.beta, seg.z, 9.0, seg.evidx, seg.segment_base)
    want, offsets = assert_device_equals_host(gpu, seg, media, medium)
    if n:
        assert len(want) >= 3 * 256
    if n >= 255:
        assert set(np.unique(medium)) == {-1, 0, 1, 2, 3} and {event.CHERENKOV, event.SCINTILLATION} == set(np.unique(want.flags))
        # at least a quarter of the blocks of 256 photons straddle segments of different media
        owner = np.repeat(medium, np.diff(offsets[::2].astype(np.int64)))
        assert sum(len(set(owner[k:k + 256].tolist())) > 1 for k in range(0, len(owner), 256)) > len(owner) // 1024


def test_no_medium_anywhere_writes_nothing(gpu, media):
    ctx = gpu.get_context()
    seg = mixed_segments(257)
    for row in (-1, 3):
        want, offsets = assert_device_equals_host(gpu, seg, media, np.full(257, row, np.int32))
        assert len(want) == 0 and not offsets.any()
    # ... not one word of arrays with room for photons
    device = {name: gpu.to_gpu(getattr(seg, name).reshape(-1), ctx) for name in ('a', 'b', 't_a', 't_b', 'beta', 'z', 'qedep', 'evidx')}
    s = seg.struct({name: a.ptr for name, a in device.items()})
    d_medium = gpu.to_gpu(np.full(257, -1, np.int32), ctx)
    d_offsets = gpu.empty(2 * 257 + 1, np.uint32, ctx)
    total = ctypes.c_uint64(5)
    table = gpu.steps.device_media(media, ctx)
    assert gpu.steps.device_media(media, ctx) is table           # one handle per context
    _lib.check(ctx._lib.chroma_steps_count_media(ctx.handle, table.handle, ctypes.byref(s), d_medium.ptr, SEED, d_offsets.ptr, ctypes.byref(total)), ctx._lib)
    assert total.value == 0
    arrays, dev = _lib.PhotonArrays(), {}
    for name, width in (('pos', 3), ('dir', 3), ('pol', 3), ('wavelengths', 1), ('t', 1), ('flags', 1), ('last_hit_triangles', 1),
                        ('weights', 1), ('evidx', 1), ('rng_counters', 1)):
        dev[name] = gpu.GPUArray(64 * width, np.uint32, ctx).fill(0xDEADBEEF)
        setattr(arrays, name, dev[name].ptr)
    _lib.check(ctx._lib.chroma_steps_generate_media(ctx.handle, table.handle, ctypes.byref(s), d_medium.ptr, SEED, d_offsets.ptr, ctypes.byref(arrays), 64), ctx._lib)
    ctx.synchronize()
    assert all((a.get() == 0xDEADBEEF).all() for a in dev.values())
    # no medium array is refused
    assert ctx._lib.chroma_steps_count_media(ctx.handle, table.handle, ctypes.byref(s), None, SEED, d_offsets.ptr, ctypes.byref(total)) == -1
    assert b'medium' in ctx._lib.chroma_last_error()


# ---- media located in the geometry ------------------------------------------------------------------------------------
START, STEP, NSEG = -130.0, 5.0, 48


def track_x():
    """A straight track along x at y = 3, z = -7: 48 steps of 5 mm from outside the outer box, through A, B, A and out again,
    with step points on the four faces it crosses"""
    x = START + STEP * np.arange(NSEG + 1)
    assert all(face in x for face in (-OUTER / 2, -INNER / 2, INNER / 2, OUTER / 2)) and x[0] < -OUTER / 2 and x[-1] > OUTER / 2
    return x


def muon_track():
    """... as segments of a muon-like particle that leaves 2 MeV per step"""
    x = track_x()
    p = np.column_stack([x, np.full(NSEG + 1, 3.0), np.full(NSEG + 1, -7.0)])
    t = (x - START) / 299.79
    return host.Segments(p[:-1], p[1:], t[:-1], t[1:], 0.999, -1.0, 2.0, 0)


def stepped_event():
    """... and as the steps of a 4 GeV muon"""
    x = track_x()
    n = NSEG + 1
    dep = np.concatenate(([0.0], np.full(NSEG, 2.0)))
    st = event.Steps(x, np.full(n, 3.0), np.full(n, -7.0), (x - START) / 299.79, np.ones(n), np.zeros(n), np.zeros(n),
                     4000.0 - 2.0 * np.arange(n), dep, dep)
    return event.Event(vertices=[event.Vertex('mu-', (START, 3.0, -7.0), (1, 0, 0), 4000.0, steps=st, pdgcode=13)])


def analytic_rows(segments, rows, outside):
    a, b, c = rows
    mid = 0.5 * (segments.a[:, 0].astype(np.float64) + segments.b[:, 0])
    return np.where(np.abs(mid) < INNER / 2, b, np.where(np.abs(mid) < OUTER / 2, a, outside)).astype(np.int32)


def box_materials():
    """A and C give Cherenkov light only (C none at these speeds), B -- the inner box -- scintillates"""
    return material('A', 1.49), material('B', 1.52, 150.0), material('C', 1.0003)


def test_media_located_on_the_device(gpu):
    geometry, materials = nested_boxes(box_materials())
    rows = [geometry.unique_materials.index(m) for m in materials]
    gg = gpu.GPUGeometry(geometry)
    media = host.LightMedia.from_geometry(geometry, wavelengths=WL)
    seg = muon_track()
    got, offsets, located = gpu.steps.generate_photons(seg, media, SEED, gpu_geometry=gg, return_offsets=True, return_medium=True)
    located = located.get()
    # (the probe ray of a midpoint outside the outer box, along z beside the box, meets nothing: `outside`, -1)
    want_rows = analytic_rows(seg, rows, -1)
    assert (want_rows == rows[0]).sum() == 24 and (want_rows == rows[1]).sum() == 16 and (want_rows == -1).sum() == 8
    assert np.array_equal(located, want_rows)
    assert np.array_equal(located, gpu.steps.locate_materials(gpu.steps.segment_midpoints(seg), gg).get())
    want = host.generate_photons(seg, media, SEED, medium=want_rows)
    assert np.array_equal(offsets, host.count_photons(seg, media, SEED, medium=want_rows)[0])
    have = got.get()
    assert_same_photons(have, want)
    # only B scintillates: every scintillation photon starts in the inner box, and the track emits such light there
    scint = (have.flags & event.SCINTILLATION) != 0
    assert scint.sum() > 1000 and (np.abs(have.pos[scint]).max(axis=1) <= INNER / 2).all()
    cher = (have.flags & event.CHERENKOV) != 0
    assert cher.sum() > 1000 and (np.abs(have.pos[cher, 0]) > INNER / 2).any() and (np.abs(have.pos[:, 0]) <= OUTER / 2).all()
    # a medium array of the caller's goes the same way, from the host or from the device
    assert_device_equals_host(gpu, seg, media, want_rows)
    again = gpu.steps.generate_photons(seg, media, SEED, medium=gpu.to_gpu(located, gg.ctx))
    assert_same_photons(again.get(), want)
    with pytest.raises(ValueError, match='medium='):
        gpu.steps.generate_photons(seg, media, SEED)


def test_simulation_locates_the_media(gpu):
    """One stepped event through Simulation(light_medium='located') on the nested boxes as a detector (the inner box its one
    channel, every photon that reaches it detected): the photons are the host generator's for the analytic rows -- a segment
    outside every solid is in the detector_material, C -- and the hits those of the same photons given as photons_beg."""
    from chroma_amd.geometry import Surface
    from chroma_amd.sim import Simulation
    from test_gpu_steps import assert_same_hits
    pmt = Surface('pmt')
    pmt.set('detect', 1.0)
    geometry, materials = nested_boxes(box_materials(), inner_surface=pmt)
    rows = [geometry.unique_materials.index(m) for m in materials]
    sim = Simulation(geometry, seed=43, light_medium='located')
    ev = list(sim.simulate([stepped_event()], keep_photons_beg=True, max_steps=20))[0]
    media = sim.light_source
    assert isinstance(media, host.LightMedia) and [s.material for s in media.sources] == list(geometry.unique_materials)
    seg = host.segments_from_vertices(stepped_event().vertices)
    want_rows = analytic_rows(seg, rows, rows[2])
    want = host.generate_photons(seg, media, 43, medium=want_rows)
    assert ev.nphotons == len(want) == len(ev.photons_beg) > 2000
    assert_same_photons(ev.photons_beg, want)
    given = list(Simulation(geometry, seed=43).simulate([event.Event(photons_beg=want)], max_steps=20))[0]
    assert len(ev.flat_hits) > 1000
    assert_same_hits(ev.flat_hits, given.flat_hits)
    # the batches are cut by an upper bound of what the located media emit
    assert media.expected_at_most(seg) >= media.expected_photons(seg, want_rows) > 0.8 * len(want)
    # the next call numbers its segments on
    ev2 = list(sim.simulate([stepped_event()], keep_photons_beg=True, max_steps=20))[0]
    seg2 = host.segments_from_vertices(stepped_event().vertices, segment_base=len(seg))
    assert_same_photons(ev2.photons_beg, host.generate_photons(seg2, media, 43, medium=want_rows))
