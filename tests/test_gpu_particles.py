"""The charged-particle stepper on the device against its host twin, bit for bit: one iteration on synthetic casts, the loop in
one medium, the loop in the nested boxes against a loop written here over chroma_intersect_mesh and the host iteration, the
flat points and segments, and Simulation(stepper='csda') against the manual chain of calls."""
import ctypes

import numpy as np
import pytest

from chroma_amd import _lib, event
from chroma_amd.demo.optics import water
from chroma_amd.generator import particles as P

from test_gpu_locate import INNER, OUTER, nested_boxes, plain

pytestmark = pytest.mark.gpu

f32 = np.float32
SEED = 77
ALIVE, STOPPED, LEFT, TRUNCATED, UNTRACKED, NAN_ABORT = (P.STATUS[k] for k in ('ALIVE', 'STOPPED', 'LEFT', 'TRUNCATED', 'UNTRACKED', 'NAN_ABORT'))
KINDS = [('mu-', 100.0), ('e-', 10.0), ('p', 50.0), ('alpha', 20.0), ('mu+', 30.0), ('e+', 3.0), ('pi+', 60.0), ('K-', 80.0)]
STATE_FIELDS = [name for name, _ in P.ParticleState.FIELDS]
POINT_NAMES = [name for name, _, _ in P.POINT_FIELDS]


@pytest.fixture(scope='module')
def gpu():
    from chroma_amd import gpu as g
    ctx = g.create_cuda_context(0)
    yield g
    ctx.pop()


def vertex(name, ke, direction=(0, 0, 1), pos=(0, 0, 0), t0=0.0):
    return event.Vertex(name, pos, direction, ke, t0=t0, pdgcode=P.PDG_CODES.get(name))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def assert_same_tracks(got, want):
    assert np.array_equal(got.offsets, want.offsets) and np.array_equal(got.status, want.status)
    for name in POINT_NAMES:
        assert same_bits(getattr(got, name), getattr(want, name)), name


# ---- one iteration -----------------------------------------------------------------------------------------------------
def mixed_particles(n):
    """n particles at the origin along z, the kinds in turn; among them an unknown species, one at rest and one at a NaN"""
    vertices = [vertex(*KINDS[i % len(KINDS)]) for i in range(n)]
    for i in range(n):
        if i % 11 == 5:
            vertices[i] = vertex('gamma', 1.0)
        if i % 11 == 7:
            vertices[i] = vertex('mu-', 0.0)
        if i % 23 == 9:
            vertices[i] = vertex('p', 20.0, pos=(0, np.nan, 0))
    return vertices


def synthetic_casts(n, stepper, seed):
    """distance, triangle, medium per particle with every edge among them: a boundary at 0, at the physics step exactly and an
    ulp beyond it, no triangle ahead in water (row 0) and in vacuum (row 1), a free flight through vacuum to a triangle, rows
    outside the table, a loss that ends just above and just below the cut (the cut is the fourth particle's energy left)"""
    rng = np.random.default_rng(seed)
    probe = P.ParticleState(mixed_particles(n))
    matrix, struct = P.point_arrays(n * (stepper.max_steps + 1))
    P.advance(probe, stepper, SEED, struct, medium=np.zeros(n, np.int32))          # no triangle ahead, in water: the physics steps
    s_phys = matrix['pos'][n:2 * n, 2].copy() if n else np.zeros(0, f32)
    distance = rng.uniform(0.0, 8.0, n).astype(f32)
    triangle = rng.integers(0, 12, n).astype(np.int32)
    medium = np.zeros(n, np.int32)
    for i in range(n):
        case = i % 13
        if case == 0:
            distance[i] = 0.0
        elif case == 1:
            distance[i] = s_phys[i]
        elif case == 2:
            distance[i] = np.nextafter(s_phys[i], f32(np.inf))
        elif case == 3:
            distance[i], triangle[i] = np.inf, -1
        elif case == 4:
            distance[i], triangle[i], medium[i] = np.inf, -1, 1
        elif case == 5:
            medium[i] = 1
        elif case == 6:
            medium[i] = -1
        elif case == 7:
            medium[i] = 2
        elif case == 8:
            triangle[i] = -1          # a distance without a triangle
    return distance, triangle, medium


@pytest.fixture(scope='module')
def two_media():
    from chroma_amd.geometry import Material
    return P.StoppingMedia([water, Material('vacuum')], birks={'water': 0.1})


@pytest.mark.parametrize('n', (0, 1, 255, 256, 257, 1025))
def test_advance_equals_host_twin(gpu, two_media, n):
    ctx = gpu.get_context()
    # the cut: what the fourth kind (an alpha of 20 MeV) has left after its first free step, so that its loss ends ON the cut
    # for the free particles, above it for the ones stopped short by a boundary and below it ... for no one: see the second cut
    probe = P.ParticleState([vertex('alpha', 20.0)])
    matrix, struct = P.point_arrays(3)
    P.advance(probe, P.Stepper(two_media, max_steps=2, ke_cut=0.05, scatter=False, outside=0), SEED, struct)
    for ke_cut in (float(matrix['ke'][1]), float(np.nextafter(matrix['ke'][1], f32(100)))):
        stepper = P.Stepper(two_media, max_steps=2, max_step=5.0, max_loss=0.05, ke_cut=ke_cut, scatter=True, outside=0)
        rows = n * 3
        want = P.ParticleState(mixed_particles(n), evidx=np.arange(n), particle_base=1000)
        want_matrix, want_struct = P.point_arrays(rows, fill=-7)
        have = gpu.particles.DeviceParticles(P.ParticleState(mixed_particles(n), evidx=np.arange(n), particle_base=1000), ctx)
        dev_matrix = {name: gpu.to_gpu(want_matrix[name].reshape(-1) if rows else np.zeros(1, dtype), ctx) for name, dtype, _ in P.POINT_FIELDS}
        dev_struct = P.point_struct({name: a.ptr for name, a in dev_matrix.items()})
        table = gpu.particles.device_stopping_media(two_media, ctx)
        assert gpu.particles.device_stopping_media(two_media, ctx) is table          # one handle per (media, context)
        options = stepper.options()
        for iteration in range(3):          # the third finds nobody alive: max_steps is 2
            distance, triangle, medium = synthetic_casts(n, stepper, seed=iteration)
            P.advance(want, stepper, SEED, want_struct, distance, triangle, medium)
            d = [gpu.to_gpu(x if n else np.zeros(1, x.dtype), ctx) for x in (distance, triangle, medium)]
            _lib.check(ctx._lib.chroma_particles_advance(ctx.handle, table.handle, ctypes.byref(have.struct), ctypes.byref(options), SEED,
                                                         d[0].ptr, d[1].ptr, d[2].ptr, ctypes.byref(dev_struct)), ctx._lib)
            if iteration == 0 and n >= 255:          # the free alpha: its first loss ends on the cut and it lives, or below it
                assert want.status[3] == (STOPPED if ke_cut > matrix['ke'][1] else ALIVE)
            got = have.fetch()
            for name in STATE_FIELDS:
                assert same_bits(getattr(got, name), getattr(want, name)), (name, iteration)
            for name, _, width in P.POINT_FIELDS:
                assert same_bits(dev_matrix[name].get()[:rows * width], want_matrix[name].reshape(-1)), (name, iteration)
        if n >= 255:
            assert {LEFT, TRUNCATED, UNTRACKED, NAN_ABORT} <= set(np.unique(want.status)) and ALIVE not in want.status
            assert want.rng_counter.max() == 8 and (want.last_hit >= 0).any()


# ---- the loop ----------------------------------------------------------------------------------------------------------
def kinds(n, **kwargs):
    rng = np.random.default_rng(n)
    directions = rng.normal(size=(n, 3))
    return [vertex(*KINDS[i % len(KINDS)], direction=directions[i], pos=(i % 7, 0, 0), t0=float(i % 3), **kwargs) for i in range(n)]


@pytest.mark.parametrize('n', (1, 257))
def test_track_without_geometry_equals_host_loop(gpu, two_media, n):
    stepper = P.Stepper(two_media, max_steps=300, max_step=5.0)
    vertices = kinds(n)
    stepped, want = P.track(vertices, stepper, SEED, particle_base=5, medium=0)
    got_stepped, got = gpu.particles.track(vertices, stepper, SEED, particle_base=5, medium=0)
    assert_same_tracks(got, want)
    assert (want.status == STOPPED).all() and len(want.t) > 100 * n
    assert same_bits(got_stepped[-1].steps.ke, stepped[-1].steps.ke)
    truncated = P.Stepper(two_media, max_steps=7, max_step=5.0)
    assert_same_tracks(gpu.particles.track(vertices, truncated, SEED, medium=0)[1], P.track(vertices, truncated, SEED, medium=0)[1])


def stopping_materials():
    """A, B, C of the nested boxes as stopping media: water, an oil and a light foam (so that a track that leaves the boxes
    ends within a metre)"""
    a, b, c = plain('A', 1.5), plain('B', 1.4), plain('C', 1.0)
    a.density, a.composition = 1.0, {'H': 0.1119, 'O': 0.8881}
    b.density, b.composition = 0.86, {'H': 0.14, 'C': 0.86}
    c.density, c.composition = 0.3, {'N': 0.76, 'O': 0.24}
    return a, b, c


class Boxes(object):
    def __init__(self, gpu):
        self.geometry, self.materials = nested_boxes(stopping_materials())
        self.rows = [self.geometry.unique_materials.index(m) for m in self.materials]          # of A, B, C
        self.gg = gpu.GPUGeometry(self.geometry)
        self.media = P.StoppingMedia.from_geometry(self.geometry)
        from chroma_amd.gpu.geometry import pack_geometry
        self.codes = np.array(pack_geometry(self.geometry).arrays['material_codes'], dtype=np.uint32)


@pytest.fixture(scope='module')
def boxes(gpu):
    return Boxes(gpu)


def reference_loop(gpu, boxes, vertices, stepper, particle_base=0):
    """The loop of chroma_particles_track written out: the device's chroma_intersect_mesh for the live particles with their
    last_hit, the float32 side rule of test_gpu_locate.expected_materials on each particle's own direction, and the host
    iteration.  Returns a Tracks."""
    ctx = boxes.gg.ctx
    state = P.ParticleState(vertices, particle_base=particle_base)
    n = state.n
    matrix, struct = P.point_arrays(n * (stepper.max_steps + 1))
    mesh = boxes.geometry.mesh
    vtx = mesh.vertices.astype(f32)
    for _ in range(stepper.max_steps + 1):
        live = np.flatnonzero(state.status == ALIVE)
        if not len(live):
            break
        distance, triangle, medium = np.full(n, np.inf, f32), np.full(n, -1, np.int32), np.full(n, stepper.outside, np.int32)
        d_dist, d_tri = gpu.to_gpu(np.full(len(live), np.inf, f32), ctx), gpu.empty(len(live), np.int32, ctx)
        d_pos, d_dir, d_last = (gpu.to_gpu(np.ascontiguousarray(x[live]).reshape(-1), ctx) for x in (state.pos, state.dir, state.last_hit))
        _lib.check(ctx._lib.chroma_intersect_mesh(ctx.handle, boxes.gg.handle, len(live), d_pos.ptr, d_dir.ptr, d_last.ptr, d_dist.ptr, d_tri.ptr),
                   ctx._lib)
        tri, dist = d_tri.get(), d_dist.get()
        hit = tri >= 0
        d = state.dir[live]
        d = d / np.sqrt((d * d).sum(axis=1, dtype=f32), dtype=f32)[:, None]
        v = vtx[mesh.triangles[np.where(hit, tri, 0)]]
        normal = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 1]).astype(f32)
        normal = normal / np.sqrt((normal * normal).sum(axis=1, dtype=f32), dtype=f32)[:, None]
        cos = (normal * -d).sum(axis=1, dtype=f32)
        code = boxes.codes[np.where(hit, tri, 0)]
        material = np.where(cos > 0, (code >> 16) & 0xFF, (code >> 24) & 0xFF).astype(np.int32)
        distance[live], triangle[live] = dist, tri
        medium[live] = np.where(hit, material, stepper.outside)
        P.advance(state, stepper, SEED, struct, distance, triangle, medium)
    assert (state.status != ALIVE).all()
    flat, flat_struct = P.point_arrays(int(state.nsteps.sum()) + n)
    offsets = np.zeros(n + 1, np.uint32)
    particles = state.struct()
    _lib.check(_lib.load().chroma_particles_points_host(ctypes.byref(particles), stepper.max_steps, ctypes.byref(struct), ctypes.byref(flat_struct),
                                                        _lib.ptr(offsets), len(flat['t'])))
    return P.Tracks(flat, offsets, state)


def test_axis_run_crosses_the_boxes_face_by_face(gpu, boxes):
    A, B, C = boxes.rows
    stepper = P.Stepper(boxes.media, max_steps=400, max_step=10.0, scatter=False, outside=C)
    inside = [vertex('mu-', 100.0, direction=(0.31, -0.52, 0.79), pos=(1, 2, 3)), vertex('mu-', 100.0, direction=(0, 0, 1), pos=(1, 2, 3))]
    _, got = gpu.particles.track(inside, stepper, SEED, gpu_geometry=boxes.gg)
    assert_same_tracks(got, reference_loop(gpu, boxes, inside, stepper))
    lo, hi = int(got.offsets[1]), int(got.offsets[2])
    z, medium = got.pos[lo:hi, 2], got.medium[lo + 1:hi]
    assert (got.pos[lo:hi, :2] == (1, 2)).all() and got.status[1] == STOPPED
    changes = np.flatnonzero(np.diff(medium)) + 1
    assert medium[np.concatenate([[0], changes])].tolist() == [B, A, C]
    # one point on each box face to the float, and the medium changes there
    assert (z == f32(INNER / 2)).sum() == 1 and (z == f32(OUTER / 2)).sum() == 1
    assert z[changes].tolist() == [INNER / 2, OUTER / 2]
    assert medium[-1] == C and z[-1] > OUTER / 2


@pytest.mark.parametrize('n', (1, 257))
def test_track_in_the_boxes_equals_the_written_out_loop(gpu, boxes, n):
    A, B, C = boxes.rows
    rng = np.random.default_rng(n)
    vertices = [vertex('mu-', 100.0, direction=(0.31, -0.52, 0.79), pos=(1, 2, 3))]
    if n > 1:
        vertices += [vertex('mu-', 60.0, direction=(0, 0, -1), pos=(0, 0, 300)), vertex('mu-', 60.0, direction=(0, 0, 1), pos=(0, 0, 300)),
                     vertex('gamma', 1.0), vertex('p', 200.0, direction=(1, 0.2, 0.1), pos=(-150, 0, 0))]
        while len(vertices) < n:
            i = len(vertices)
            vertices.append(vertex(*KINDS[i % 4], direction=rng.normal(size=3), pos=rng.uniform(-120, 120, 3)))
    for outside in ((C, -1) if n > 1 else (C,)):
        stepper = P.Stepper(boxes.media, max_steps=300, max_step=10.0, scatter=True, outside=outside)
        _, got = gpu.particles.track(vertices, stepper, SEED, gpu_geometry=boxes.gg, particle_base=3)
        assert_same_tracks(got, reference_loop(gpu, boxes, vertices, stepper, particle_base=3))
        if n > 1:
            counts = np.diff(got.offsets.astype(np.int64))
            # aimed at the boxes from outside: through C into A; aimed away: LEFT with its vertex alone, or stopped in C
            first = got.medium[got.offsets[1] + 1:got.offsets[2]]
            assert first[0] == C and A in first
            if outside < 0:
                assert got.status[2] == LEFT and counts[2] == 1
            else:
                assert got.status[2] == STOPPED and (got.medium[got.offsets[2] + 1:got.offsets[3]] == C).all()
            assert got.status[3] == UNTRACKED and counts[3] == 1
            assert {A, B, C} <= set(np.unique(got.medium)) and (got.status[4:] != ALIVE).all()


# ---- points and segments -----------------------------------------------------------------------------------------------
def test_points_and_segments_equal_host_twins_and_refuse_short_room(gpu, boxes):
    ctx = boxes.gg.ctx
    A, B, C = boxes.rows
    stepper = P.Stepper(P.StoppingMedia.from_geometry(boxes.geometry, birks={'A': 0.1}), max_steps=300, max_step=10.0, outside=C)
    vertices = kinds(40) + [vertex('gamma', 1.0)]
    evidx = np.arange(41) // 3
    made, _, tracks = gpu.particles.track_segments(vertices, stepper, SEED, gpu_geometry=boxes.gg, evidx=evidx, segment_base=9, return_tracks=True)
    want, want_medium = tracks.segments(segment_base=9)
    got, got_medium = made.get()
    assert len(got) == len(want) == len(tracks.t) - 41 > 1000 and got.segment_base == 9
    for name in ('a', 'b', 't_a', 't_b', 'beta', 'z', 'qedep', 'evidx'):
        assert same_bits(getattr(got, name), getattr(want, name)), name
    assert np.array_equal(got_medium, want_medium) and (got.qedep < tracks.edep[tracks.medium >= 0]).any()
    # ... and those of the host twin from the same points as a matrix
    state = P.ParticleState(vertices, evidx=evidx)
    state.nsteps = (np.diff(tracks.offsets.astype(np.int64)) - 1).astype(np.uint32)
    matrix, struct = P.point_arrays(41 * 301)
    for i in range(41):
        lo, hi = int(tracks.offsets[i]), int(tracks.offsets[i + 1])
        for name in POINT_NAMES:
            matrix[name][np.arange(hi - lo) * 41 + i] = getattr(tracks, name)[lo:hi]
    twin = {name: np.zeros((len(want), 3) if name in 'ab' else len(want), np.uint32 if name == 'evidx' else f32) for name in ('a', 'b', 't_a', 't_b', 'beta', 'z', 'qedep', 'evidx')}
    twin_medium = np.zeros(len(want), np.int32)
    seg = _lib.StepSegments()
    for name, a in twin.items():
        setattr(seg, name, _lib.ptr(a))
    particles = state.struct()
    _lib.check(_lib.load().chroma_particles_segments_host(ctypes.byref(particles), 300, ctypes.byref(struct), ctypes.byref(seg), _lib.ptr(twin_medium), len(want)))
    for name, a in twin.items():
        assert same_bits(a, getattr(want, name)), name
    assert np.array_equal(twin_medium, want_medium)
    flat, flat_struct = P.point_arrays(len(tracks.t))
    offsets = np.zeros(42, np.uint32)
    _lib.check(_lib.load().chroma_particles_points_host(ctypes.byref(particles), 300, ctypes.byref(struct), ctypes.byref(flat_struct), _lib.ptr(offsets), len(tracks.t)))
    assert np.array_equal(offsets, tracks.offsets) and all(same_bits(flat[name], getattr(tracks, name)) for name in POINT_NAMES)
    assert _lib.load().chroma_particles_points_host(ctypes.byref(particles), 300, ctypes.byref(struct), ctypes.byref(flat_struct), _lib.ptr(offsets), len(tracks.t) - 1) == -1

    # one point, one segment too few: refused, and not a word of the canary-filled arrays is written
    run = gpu.particles._run(vertices, stepper, SEED, boxes.gg, ctx, 0, evidx, None)          # (kept: its particle arrays are read)
    assert run[2] == len(tracks.t)
    total, nseg = len(tracks.t), len(want)
    canary = {name: gpu.GPUArray(total * width, np.uint32, ctx).fill(0xDEADBEEF) for name, _, width in P.POINT_FIELDS}
    points = P.point_struct({name: a.ptr for name, a in canary.items()})
    d_offsets = gpu.GPUArray(42, np.uint32, ctx).fill(0xDEADBEEF)
    assert ctx._lib.chroma_particles_points(ctx.handle, ctypes.byref(points), d_offsets.ptr, total - 1) == -1
    assert b'room for' in ctx._lib.chroma_last_error()
    seg_canary = {name: gpu.GPUArray(nseg * (3 if name in 'ab' else 1), np.uint32, ctx).fill(0xDEADBEEF) for name in twin}
    d_medium = gpu.GPUArray(nseg, np.uint32, ctx).fill(0xDEADBEEF)
    seg = _lib.StepSegments()
    for name, a in seg_canary.items():
        setattr(seg, name, a.ptr)
    assert ctx._lib.chroma_particles_segments(ctx.handle, ctypes.byref(seg), d_medium.ptr, nseg - 1) == -1
    for a in list(canary.values()) + list(seg_canary.values()) + [d_offsets, d_medium]:
        assert (a.get() == 0xDEADBEEF).all()
    # with room: the same points again
    _lib.check(ctx._lib.chroma_particles_points(ctx.handle, ctypes.byref(points), d_offsets.ptr, total), ctx._lib)
    assert np.array_equal(d_offsets.get(), tracks.offsets) and same_bits(canary['ke'].get().view(f32), tracks.ke)

    # no particles: nothing happens
    _, empty = gpu.particles.track([], stepper, SEED, gpu_geometry=boxes.gg)
    assert len(empty) == 0 and len(empty.t) == 0 and empty.offsets.tolist() == [0]
    none = gpu.particles.track_segments([], stepper, SEED, gpu_geometry=boxes.gg)
    assert len(none) == 0


# ---- Simulation --------------------------------------------------------------------------------------------------------
def test_simulation_tracks_vertices_through_the_detector(gpu):
    from chroma_amd.geometry import Surface
    from chroma_amd.sim import Simulation
    from test_gpu_steps import assert_same_hits
    pmt = Surface('pmt')
    pmt.set('detect', 1.0)
    geometry, materials = nested_boxes(stopping_materials(), inner_surface=pmt)
    C = geometry.unique_materials.index(materials[2])
    muon = lambda: event.Vertex('mu-', (-90, 5, 3), (1, 0.1, 0.05), 100.0, pdgcode=13)
    sim = Simulation(geometry, seed=43, stepper='csda', particle_tracking=True)
    ev = list(sim.simulate([muon()], max_steps=20, keep_photons_beg=True))[0]
    assert ev.nphotons == len(ev.photons_beg) > 1000 and (ev.photons_beg.flags == event.CHERENKOV).all()
    assert len(ev.flat_hits) > 100
    # the manual chain on the simulation's own context: tracked, cut into segments, lit and propagated on the device
    stepper = sim.stepper
    assert isinstance(stepper, P.Stepper) and [m for m in stepper.media.materials] == list(geometry.unique_materials)
    import copy
    manual = copy.copy(stepper)
    manual.outside = C          # (the detector_material: where a particle with no triangle ahead is)
    light = gpu.steps.LightMedia.from_geometry(geometry)
    segments = gpu.particles.track_segments([muon()], manual, 43, gpu_geometry=sim.gpu_geometry)
    photons = gpu.steps.generate_photons(segments, light, 43, ctx=sim.context, medium=segments.medium[:len(segments)])
    assert len(photons) == ev.nphotons
    hits = photons.propagate_hits(sim.gpu_geometry, gpu.get_rng_states(1, seed=43), max_steps=20, sort=True)
    assert_same_hits(ev.flat_hits, hits)
    # particle_tracking: the vertex carries the steps that were made
    stepped, tracks = gpu.particles.track([muon()], manual, 43, gpu_geometry=sim.gpu_geometry)
    got = ev.vertices[0].steps
    assert got is not None and all(same_bits(getattr(got, name), getattr(stepped[0].steps, name)) for name in ('x', 'y', 'z', 't', 'dx', 'dy', 'dz', 'ke', 'edep', 'qedep'))
    assert tracks.status[0] == STOPPED and len(got.x) > 30
    # an Event without photons or steps, and a list of vertices: accepted; the next call numbers particles and segments on
    more = list(sim.simulate([event.Event(vertices=[muon()]), event.Event(vertices=[muon(), muon()])], max_steps=20))
    assert [len(e.vertices) for e in more] == [1, 2] and all(len(e.flat_hits) > 100 for e in more) and more[1].nphotons > 1.5 * more[0].nphotons
    assert list(sim.simulate(muon(), max_steps=20))[0].nphotons > 1000
    # without a stepper nothing changes: both refusals
    plain_sim = Simulation(geometry, seed=43)
    with pytest.raises(NotImplementedError, match='events without photons'):
        list(plain_sim.simulate([event.Event(vertices=[muon()])]))
    with pytest.raises(NotImplementedError, match='Vertex input'):
        list(plain_sim.simulate([muon()]))
