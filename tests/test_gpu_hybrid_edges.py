"""The hybrid render's kernels (k_hybrid_lookup, k_hybrid_reduce, k_hybrid_image, k_hybrid_pixels; chroma/cuda/hybrid_render.cu)
at their sizes, key runs and edges: launches through the C entry points (chroma_hybrid_lookup / _image / _pixels) on arrays this
file owns, every sample bit for bit against the oracle restatements of tests/test_gpu_hybrid_render.py, every table, image and
pixel against the NumPy restatements of chroma_amd.gpu.render.  Those restatements are the project's own reading of
hybrid_render.cu: tests/test_ref_hybrid_host.py holds them to the reference's file itself (compiled for the host into oracle/_ref),
on the scenes, bundles and launches defined here, and tests/test_gpu_ref_hybrid.py the kernels, with this file's call helpers.

Every array a call may write is GUARD rows longer than the call is told and holds a sentinel where the call has no business:
behind the array, in the sample rows of threads past the last triangle, everywhere when the call returns early or refuses.
Tables and images are added to, so their live rows start from values that show an addition (a sentinel of -6e18 would swallow
one); rows no sample reaches must keep their bits, -0.0 included.

The scenes are chosen for the run structure they give k_hybrid_reduce (one key more than eight blocks long; both sides of one
triangle as neighbouring keys; the records of key 0 between those of key_none when the triangle count is a power of two).  The
test without a `gpu` mark asserts from the oracle alone that they still do."""
import numpy as np
import pytest

from conftest import ROOT             # noqa: F401  (puts the repository on sys.path)
from chroma_amd.event import NAN_ABORT, NO_HIT, REFLECT_DIFFUSE, REFLECT_SPECULAR
from chroma_amd.gpu.render import hybrid_accumulate, hybrid_image_update, hybrid_pixels
from test_gpu_hybrid_render import _bits, _draws, _normals, _scene, _step_to_diffuse, _vertices, oracle_image, oracle_lookup  # noqa: F401

gpu_test = pytest.mark.gpu

f32 = np.float32
SENTINEL = 0xDEADBEEF           # as a float32 -6.26e18: no cos_theta, no table entry, no image value
GUARD = 64                      # rows behind every array (one block of the two sample kernels)
SIZES = (1, 63, 64, 65, 127, 128, 129, 257)
STRESS_SIZES = (1, 17, 33, 47)   # grey_stress has 48 triangles: the sizes that leave room for each arm of the cap
PIXEL_SIZES = (1, 63, 64, 65, 255, 256, 257)
SEED = 7
WAVELENGTH = 545.0
XYZ = (0.3, 1.0, 0.7)           # every channel lit, no power of two: cos_theta * xyz and xyz * lookup / n round
BIG_ID = 5000000000             # a stream id base past 2^32
INSIDE = (0.3, -0.5, 0.8)       # the ray of the image arrays' guard rows: from the origin it meets a wall of every room here


# ---- scenes (built once per module): name -> (geometry, packed, source) -----------------------------------------------
_memo = {}


def _once(fn):
    def get(*args):
        key = (fn.__name__,) + args
        if key not in _memo:
            _memo[key] = fn(*args)
        return _memo[key]
    get.__name__ = fn.__name__
    return get


def _clear():
    from chroma_amd.geometry import Material
    clear = Material('clear')                                     # as in test_lambertian_room
    clear.set('refractive_index', 1.0)
    clear.set('absorption_length', 1e30)
    clear.set('scattering_length', 1e30)
    return clear


def _sheet(centre, u, v, nu, nv):
    """A flat sheet of nu x nv cells (two triangles each) spanned by the edge vectors u and v around `centre`; the normal of
    every triangle is along u x v."""
    from chroma_amd.geometry import Mesh
    centre, u, v = [np.asarray(x, float) for x in (centre, u, v)]
    i, j = np.meshgrid(np.arange(nu + 1), np.arange(nv + 1), indexing='ij')
    vertices = centre + (i.reshape(-1, 1) / nu - 0.5) * u + (j.reshape(-1, 1) / nv - 0.5) * v
    at = lambda a, b: a * (nv + 1) + b                            # noqa: E731
    tris = []
    for a in range(nu):
        for b in range(nv):
            tris += [(at(a, b), at(a + 1, b), at(a + 1, b + 1)), (at(a, b), at(a + 1, b + 1), at(a, b + 1))]
    return Mesh(vertices, np.array(tris, np.int32))


def _flat(solids, material):
    from chroma_amd.geometry import Geometry
    from chroma_amd.gpu.geometry import pack_geometry
    from chroma_amd.loader import create_geometry_from_obj
    g = Geometry(material)
    for solid, displacement in solids:
        g.add_solid(solid, displacement=displacement)
    g = create_geometry_from_obj(g)
    return g, pack_geometry(g)


def _room_solid(clear):
    from chroma_amd import make
    from chroma_amd.demo.optics import lambertian_surface
    from chroma_amd.geometry import Solid, vacuum
    return Solid(make.box(1000.0, 1000.0, 1000.0), clear, vacuum, surface=lambertian_surface)


@_once
def room():
    """The Lambertian room of test_lambertian_room: 16 triangles, so key_none = 32 needs a bit no key of a triangle has."""
    clear = _clear()
    return _flat([(_room_solid(clear), None)], clear) + ((37.0, -210.0, 55.0),)


@_once
def room_sphere():
    """The room and an index-matched sphere without a surface in it (4432 triangles): the photons aimed at the sphere cross
    it undeflected and land on one wall triangle, one key more than eight blocks of k_hybrid_reduce long."""
    from chroma_amd import make
    from chroma_amd.geometry import Solid
    clear = _clear()
    return _flat([(_room_solid(clear), None), (Solid(make.sphere(20.0, 48), clear, clear), (300.0, 100.0, 400.0))], clear) \
        + ((37.0, -210.0, 55.0),)


SHEET_CENTRE = np.array([100.0, 0.0, 0.0])
MIRROR_CENTRE = np.array([150.0, 300.0, 0.0])


@_once
def room_sheet_mirror():
    """The room, a free-standing Lambertian sheet in the plane x = 100 (triangles 16 and 17, normal +x) and a free-standing
    mirror of 16 x 16 x 2 triangles whose normal bisects the directions to the source (the origin) and to the sheet's centre
    (530 triangles): the sheet is lit from the source on one side and by way of the mirror on the other."""
    from chroma_amd.demo.optics import lambertian_surface, shiny_surface
    from chroma_amd.geometry import Solid
    clear = _clear()
    unit = lambda a: a / np.linalg.norm(a)                        # noqa: E731
    normal = unit(unit(-MIRROR_CENTRE) + unit(SHEET_CENTRE - MIRROR_CENTRE))
    along = np.array([0.0, 0.0, 1.0])
    sheet = Solid(_sheet(SHEET_CENTRE, (0.0, 100.0, 0.0), (0.0, 0.0, 100.0), 1, 1), clear, clear, surface=lambertian_surface)
    mirror = Solid(_sheet(MIRROR_CENTRE, 100.0 * along, 100.0 * np.cross(normal, along), 16, 16), clear, clear, surface=shiny_surface)
    return _flat([(_room_solid(clear), None), (sheet, None), (mirror, None)], clear) + ((0.0, 0.0, 0.0),)


@_once
def sheet_mirror32():
    """No room: a Lambertian sheet (triangles 0 and 1, normal +x, half as high as the mirror's beam is) behind the source and
    a mirror of 5 x 3 x 2 triangles in front of it, 32 triangles.  The mirror's photons come back past the source onto the
    sheet against its normal (keys 0 and 2) or past it out of the world (key_none = 64): the records of key 0 lie between
    those of key_none in sample order, and only bit 6 tells them apart."""
    from chroma_amd.demo.optics import lambertian_surface, shiny_surface
    from chroma_amd.geometry import Solid
    clear = _clear()
    sheet = Solid(_sheet((-100.0, 0.0, 100.0), (0.0, 800.0, 0.0), (0.0, 0.0, 200.0), 1, 1), clear, clear, surface=lambertian_surface)
    mirror = Solid(_sheet((200.0, 0.0, 0.0), (0.0, 0.0, 120.0), (0.0, 120.0, 0.0), 5, 3), clear, clear, surface=shiny_surface)
    return _flat([(sheet, None), (mirror, None)], clear) + ((0.0, 0.0, 0.0),)


@_once
def grey_stress():
    """The scintillator stress cube (thin film, WLS, dichroic, detecting faces) in grey walls, from the existing file."""
    from chroma_amd.gpu.geometry import pack_geometry
    g = _scene('grey_stress')
    return g, pack_geometry(g), (37.0, -410.0, 55.0)


SCENES = {f.__name__: f for f in (room, room_sphere, room_sheet_mirror, sheet_mirror32, grey_stress)}
OUTSIDE_SOURCE = (37.0, -2100.0, 55.0)          # outside the room: the far walls are hidden behind the near one


def _ntri(scene):
    return len(SCENES[scene]()[0].mesh.triangles)


def _start_counters(n):
    """Draw counters a call continues from: different per thread, none zero."""
    return ((np.arange(n, dtype=np.uint64) * 7 + 3) % 1000 + 1).astype(np.uint32)


def _start_table(rows, salt):
    """Table or image rows an addition shows on: a third 0.0, a third -0.0, a third values in [0.5, 1.5)."""
    rng = np.random.default_rng(1000 + salt)
    t = (rng.random((rows, 3)) + 0.5).astype(f32)
    kind = rng.integers(0, 3, (rows, 3))
    t[kind == 0] = f32(0.0)
    t[kind == 1] = f32(-0.0)
    return t


# ---- the oracle's side, every launch restated once ---------------------------------------------------------------------
class Want(object):
    """The samples of one lookup launch (n live threads from triangle `offset`) by oracle_lookup."""

    def __init__(self, res, n, offset):
        self.tri, self.side, self.hist, self.cos, self.ctr, self.mine = res
        self.n, self.offset = n, offset

    def keys(self, ntri):
        return np.where(self.tri >= 0, 2 * self.tri.astype(np.int64) + self.side, 2 * ntri)

    def runs(self, ntri):
        """{key: run length} of the real keys, and the stably sorted keys."""
        k = np.sort(self.keys(ntri), kind='stable')
        keys, counts = np.unique(k[k < 2 * ntri], return_counts=True)
        return dict(zip(keys.tolist(), counts.tolist())), k

    def add_to(self, l1, l2, xyz=XYZ):
        contrib = (self.cos[:, None] * np.asarray(xyz, f32)[None, :]).astype(f32)
        return hybrid_accumulate(l1.copy(), l2.copy(), self.tri, self.side, contrib)


def want_lookup(oracle_mod, scene, n, offset, counters, max_steps=10, source=None, id_base=0, variant='contract'):
    counters = np.asarray(counters, np.uint32)[:n]
    key = ('lookup', scene, n, offset, counters.tobytes(), max_steps, source, id_base, variant)
    if key not in _memo:
        g, packed, src = SCENES[scene]()
        assert 0 <= offset and offset + n <= len(g.mesh.triangles)
        _memo[key] = Want(oracle_lookup(oracle_mod, packed, g, SEED, id_base, counters, n, offset, src if source is None else source,
                                        WAVELENGTH, max_steps, variant=variant), n, offset)
    return _memo[key]


def want_image(oracle_mod, scene, origins, directions, counters, max_steps=10, id_base=0, variant='contract'):
    n = len(origins)
    counters = np.asarray(counters, np.uint32)[:n]
    key = ('image', scene, np.asarray(origins, f32).tobytes(), np.asarray(directions, f32).tobytes(), counters.tobytes(), max_steps, id_base,
           variant)
    if key not in _memo:
        g, packed, _ = SCENES[scene]()
        _memo[key] = oracle_image(oracle_mod, packed, g, SEED, id_base, counters, origins, directions, WAVELENGTH, max_steps, variant=variant)
    return _memo[key]


def want_tables(oracle_mod, scene):
    """The tables one full launch from zero counters fills, starting from zero."""
    nt = _ntri(scene)
    w = want_lookup(oracle_mod, scene, nt, 0, np.zeros(nt, np.uint32))
    return w.add_to(np.zeros((nt, 3), f32), np.zeros((nt, 3), f32))


# ---- ray bundles of the image tests, all in room_sheet_mirror -----------------------------------------------------------
OUTSIDE_CAMERA = (0.0, -2000.0, 0.0)
CAMERAS = np.array([[0.0, 0.0, 0.0], [220.0, 40.0, -30.0]], f32)         # in front of the sheet (x < 100) and behind it


def _unit(rng, n):
    d = rng.normal(size=(n, 3))
    return (d / np.linalg.norm(d, axis=1)[:, None]).astype(f32)


@_once
def camera_bundle(n):
    """n rays from the two cameras in turn; half of them aimed at the Lambertian sheet (one camera sees its lookup1 side,
    the other its lookup2 side), the others anywhere (the walls, a few by way of the mirror); every eighth ray starts
    outside the room and points away from it, the only kind that does not diffuse in a closed Lambertian room."""
    rng = np.random.default_rng(300 + n)
    o = CAMERAS[np.arange(n) % 2]
    d = _unit(rng, n)
    aimed = np.arange(n) % 4 < 2
    target = np.column_stack([np.full(n, 100.0), rng.uniform(-45.0, 45.0, n), rng.uniform(-45.0, 45.0, n)]) - o
    d[aimed] = (target / np.linalg.norm(target, axis=1)[:, None]).astype(f32)[aimed]
    lost = np.arange(n) % 8 == 7
    o[lost] = OUTSIDE_CAMERA
    d[lost, 1] = -np.abs(d[lost, 1]) - f32(0.1)
    return np.ascontiguousarray(o, f32), np.ascontiguousarray(d, f32)


@_once
def outside_bundle():
    """129 rays from outside the room pointing away from it."""
    d = _unit(np.random.default_rng(41), 129)
    d[:, 1] = -np.abs(d[:, 1]) - f32(0.1)
    return np.tile(f32(OUTSIDE_CAMERA), (129, 1)), d


ZERO_RAY, NAN_RAY = 5, 37                        # both in the first wave of the bundle below


@_once
def broken_bundle():
    """camera_bundle(65) with one zero and one NaN direction."""
    o, d = camera_bundle(65)
    d = d.copy()
    d[ZERO_RAY] = 0.0
    d[NAN_RAY, 1] = np.nan
    return o, d


@_once
def scaled_bundle():
    """camera_bundle(129) with every second direction a quarter as long and every third a thousand times as long."""
    o, d = camera_bundle(129)
    scale = np.ones(129, f32)
    scale[1::2] = f32(0.25)
    scale[::3] = f32(1e3)
    return o, (d * scale[:, None]).astype(f32), scale


# ---- the test that needs no GPU: the scenes reach what they are meant to reach -------------------------------------------
def test_the_scenes_reach_their_runs_sides_and_misses(oracle_mod):
    """Exact conditions on the oracle's samples, so that a scene that drifts from its purpose fails here and a green GPU run
    is not read as coverage.  (It prints the figures; profiles/r20/INDEX.md has them as they were when this was written.)"""
    # room_sphere, the full launch: one key of at least two full blocks and a boundary, the room's own keys on both sides of it
    nt = _ntri('room_sphere')
    assert nt == 4432 and _ntri('room') == 16 and _ntri('room_sheet_mirror') == 530 and _ntri('sheet_mirror32') == 32
    w = want_lookup(oracle_mod, 'room_sphere', nt, 0, np.zeros(nt, np.uint32))
    runs, skeys = w.runs(nt)
    long_key = max(runs, key=runs.get)
    print('room_sphere: %d samples reach their triangle, %d diffuse, longest run %d on key %d, %d keys' % (
        w.mine.sum(), (w.tri >= 0).sum(), runs[long_key], long_key, len(runs)))
    assert runs[long_key] >= 513, runs
    assert min(runs) < long_key < max(runs), 'the long run has no neighbours'
    assert skeys[0] < 2 * nt, 'the first sorted record starts no run'
    assert (skeys == 2 * nt).any()
    # the second launch onto the same tables is another launch, not the first again
    w2 = want_lookup(oracle_mod, 'room_sphere', nt, 0, w.ctr)
    assert w2.runs(nt)[0].get(long_key, 0) >= 513 and not np.array_equal(_bits(w2.cos), _bits(w.cos))
    # ... over the sphere's triangles only: the long run starts at record 0 of the sort
    ws = want_lookup(oracle_mod, 'room_sphere', nt - 16, 16, np.zeros(nt - 16, np.uint32))
    runs_s, skeys_s = ws.runs(nt)
    print('room_sphere from triangle 16: runs %s' % runs_s)
    assert skeys_s[0] == min(runs_s) and runs_s[int(skeys_s[0])] >= 513
    # a serial sum of such a run in the opposite order gives other bits (what pins the order of the sum)
    sel = np.flatnonzero(w.keys(nt) == long_key)
    fwd, back = f32(0), f32(0)
    for c in w.cos[sel]:
        fwd = f32(fwd + c)
    for c in w.cos[sel][::-1]:
        back = f32(back + c)
    assert fwd.tobytes() != back.tobytes()

    # the room: every sample diffuses on its own triangle, so the last sorted record ends a run; from outside most are key_none
    w = want_lookup(oracle_mod, 'room', 16, 0, np.zeros(16, np.uint32))
    assert w.mine.all() and np.array_equal(w.tri, np.arange(16)) and (w.side == 1).all()
    w = want_lookup(oracle_mod, 'room', 16, 0, np.zeros(16, np.uint32), source=OUTSIDE_SOURCE)
    print('room from outside: triangles %s' % w.tri.tolist())
    assert 0 < (w.tri >= 0).sum() < 16 and (w.side[w.tri >= 0] == 0).all()

    # room_sheet_mirror: both sides of one triangle as neighbouring keys, both tables change, runs of hundreds on the walls
    nt = _ntri('room_sheet_mirror')
    w = want_lookup(oracle_mod, 'room_sheet_mirror', nt, 0, np.zeros(nt, np.uint32))
    runs, _ = w.runs(nt)
    print('room_sheet_mirror: %d reach their triangle, runs %s' % (w.mine.sum(), runs))
    both = [k // 2 for k in runs if k % 2 == 0 and k + 1 in runs]
    assert both and all(t in (16, 17) for t in both), runs
    assert any(min(runs[2 * t], runs[2 * t + 1]) >= 1 and max(runs[2 * t], runs[2 * t + 1]) >= 3 for t in both)
    l1, l2 = want_tables(oracle_mod, 'room_sheet_mirror')
    assert l1.any() and l2.any() and l1[both[0]].any() and l2[both[0]].any()
    assert sorted(runs.values())[-2] >= 100
    # at max_steps 1 a sample that reached its triangle (a mirror's) did not diffuse; at 0 none does
    w1 = want_lookup(oracle_mod, 'room_sheet_mirror', nt, 0, np.zeros(nt, np.uint32), max_steps=1)
    stuck = w1.mine & (w1.tri < 0)
    assert stuck.sum() >= 100 and (w1.hist[stuck] == REFLECT_SPECULAR).all()
    assert (w1.tri >= 0).any() and (w1.tri[w1.tri >= 0] == np.flatnonzero(w1.tri >= 0)).all()
    w0 = want_lookup(oracle_mod, 'room_sheet_mirror', nt, 0, np.zeros(nt, np.uint32), max_steps=0)
    assert w0.mine.any() and (w0.tri == -1).all() and (w0.hist == 0).all()

    # sheet_mirror32: records of key 0 with records of key_none between them in sample order
    w = want_lookup(oracle_mod, 'sheet_mirror32', 32, 0, np.zeros(32, np.uint32))
    keys = w.keys(32)
    print('sheet_mirror32: keys %s' % keys.tolist())
    zero = np.flatnonzero(keys == 0)
    assert len(zero) >= 3 and (keys[zero[0]:zero[-1]] == 64).any(), keys
    assert (keys == 2).sum() >= 3

    # grey_stress (48 triangles, the walls last): histories of more than one step, diffusions away from the sample's own triangle
    nt = _ntri('grey_stress')
    assert nt == 48
    for n in STRESS_SIZES:
        for offset in (0, nt - n):
            w = want_lookup(oracle_mod, 'grey_stress', n, offset, _start_counters(n + 45), id_base=BIG_ID)
            far = (w.tri >= 0) & (w.tri != np.arange(offset, offset + n))
            print('grey_stress, %d from %d: %d reach their triangle, %d diffuse, %d of them elsewhere; histories %s' % (
                n, offset, w.mine.sum(), (w.tri >= 0).sum(), far.sum(), sorted(set(w.hist.tolist()))))
    assert w.mine.sum() >= 10 and far.any() and len(set(w.hist.tolist())) >= 4               # (47 from triangle 1)
    w1 = want_lookup(oracle_mod, 'grey_stress', nt, 0, _start_counters(nt + 7), max_steps=1)
    assert (w1.mine & (w1.tri < 0)).any() and (w1.tri >= 0).any()

    # the image bundles: the sheet seen from both sides where both tables hold light; the outside bundle meets nothing
    l1, l2 = want_tables(oracle_mod, 'room_sheet_mirror')
    for n in SIZES:
        o, d = camera_bundle(n)
        tri, side, hist, _ = want_image(oracle_mod, 'room_sheet_mirror', o, d, _start_counters(n))
        lit1 = (tri >= 0) & (side == 1) & l1[np.maximum(tri, 0)].any(axis=1)
        lit2 = (tri >= 0) & (side == 0) & l2[np.maximum(tri, 0)].any(axis=1)
        print('camera bundle %d: %d diffuse, %d read light in lookup1, %d in lookup2' % (n, (tri >= 0).sum(), lit1.sum(), lit2.sum()))
        assert lit1.any()
        assert n < 63 or (lit2.sum() >= 5 and lit1.sum() >= 5 and (tri < 0).any())
    o, d = outside_bundle()
    _, first, _ = oracle_mod.distance_to_mesh(SCENES['room_sheet_mirror']()[1], o, (d / np.linalg.norm(d, axis=1)[:, None]).astype(f32))
    assert (first == -1).all()
    o, d = broken_bundle()
    tri, side, hist, ctr = want_image(oracle_mod, 'room_sheet_mirror', o, d, _start_counters(65))
    assert (hist[[ZERO_RAY, NAN_RAY]] == (NO_HIT | NAN_ABORT)).all() and (tri[[ZERO_RAY, NAN_RAY]] == -1).all()
    good = np.delete(np.arange(65), [ZERO_RAY, NAN_RAY])
    tri_g = want_image(oracle_mod, 'room_sheet_mirror', *camera_bundle(65), _start_counters(65))
    assert all(np.array_equal(a[good], b[good]) for a, b in zip((tri, side, hist, ctr), tri_g))


GRAZING_RAY = np.array([1055638222, 1058485921, 1059692941], np.uint32).view(f32)


def test_the_lookup_restatement_casts_the_direction_as_given(oracle_mod):
    """Sample 1003 of room_sphere's second full launch grazes the sphere (cos_theta 1.1e-4).  update_xyz_lookup normalises its
    direction once and hands it to intersect_mesh (hybrid_render.cu:84-87): triangle 1003, the sample's own.  distance_to_mesh
    divides by the norm once more (mesh.h:124-151), which moves this direction by an ulp and the ray onto triangle 3162, so
    oracle_lookup must not go through it; the first device run of this file found the restatement doing so."""
    g, packed, source = room_sphere()
    o, d = np.asarray([source], f32), GRAZING_RAY.reshape(1, 3)
    again = (d / np.sqrt((d * d).sum(axis=1, dtype=f32))[:, None]).astype(f32)
    assert not np.array_equal(_bits(again), _bits(d))
    assert oracle_mod.distance_to_mesh(packed, o, d, normalize=False)[1][0] == 1003
    assert oracle_mod.distance_to_mesh(packed, o, d)[1][0] == 3162
    nt = len(g.mesh.triangles)
    first = want_lookup(oracle_mod, 'room_sphere', nt, 0, np.zeros(nt, np.uint32))
    second = want_lookup(oracle_mod, 'room_sphere', nt, 0, first.ctr)
    assert second.mine[1003] and second.tri[1003] == 1 and _bits(second.cos)[1003] == 0x38e66000


def test_the_reference_loop_and_the_stepped_propagate_agree_but_for_a_grazing_ray(oracle_mod, monkeypatch):
    """oracle.to_diffuse (the loop of hybrid_render.cu:20-58, what the restatements use) against the route the restatements
    took before, oracle.propagate one step at a time (_step_to_diffuse): two walks through the oracle's step functions that
    give the same samples, multi-step histories included.  The one exception is sample 1003 above: propagate divides the
    direction by its norm at every step (propagate.cu:248), to_diffuse and the kernel never do, and the grazing ray draws a
    different number of times (found by the first device run of the draw counters)."""
    import test_gpu_hybrid_render as restated

    def stepped(scene, n, offset, counters, **kw):
        g, packed, source = SCENES[scene]()
        normals = _normals(g)
        monkeypatch.setattr(restated, '_to_diffuse', lambda om, pk, photons, active, seed, id_base, ctr, max_steps:
                            _step_to_diffuse(om, pk, normals, photons, active, seed, id_base, ctr, max_steps))
        try:
            return oracle_lookup(oracle_mod, packed, g, SEED, kw.get('id_base', 0), counters, n, offset, source, WAVELENGTH, 10)
        finally:
            monkeypatch.undo()

    def differing(w, res):
        return np.flatnonzero((w.tri != res[0]) | (w.side != res[1]) | (w.hist != res[2]) | (_bits(w.cos) != _bits(res[3])) | (w.ctr != res[4]))
    for scene, id_base in (('room_sheet_mirror', 0), ('sheet_mirror32', 0), ('grey_stress', BIG_ID)):
        nt = _ntri(scene)
        counters = _start_counters(nt)
        w = want_lookup(oracle_mod, scene, nt, 0, counters, id_base=id_base)
        assert len(differing(w, stepped(scene, nt, 0, counters, id_base=id_base))) == 0, scene
        assert scene != 'grey_stress' or len(set(w.hist.tolist())) >= 4
    nt = _ntri('room_sphere')
    first = want_lookup(oracle_mod, 'room_sphere', nt, 0, np.zeros(nt, np.uint32))
    assert len(differing(first, stepped('room_sphere', nt, 0, np.zeros(nt, np.uint32)))) == 0
    second = want_lookup(oracle_mod, 'room_sphere', nt, 0, first.ctr)
    apart = differing(second, stepped('room_sphere', nt, 0, first.ctr))
    print('room_sphere, second launch: the two routes differ for samples %s, cos_theta %s' % (apart.tolist(), second.cos[apart].tolist()))
    assert 1003 in apart and len(apart) <= 3                  # (890 when this was written: the same sample, one draw more)


def test_oracle_image_normalises_as_the_kernel_does(oracle_mod):
    """update_xyz_image divides every direction by its f32 norm (hybrid_render.cu:149) and so does oracle_image: a bundle
    scaled by powers of two gives the samples of the unscaled one bit for bit (the norm scales exactly)."""
    o, d = camera_bundle(129)
    c0 = _start_counters(129)
    base = want_image(oracle_mod, 'room_sheet_mirror', o, d, c0)
    for factor in (0.25, 4096.0):
        scaled = want_image(oracle_mod, 'room_sheet_mirror', o, (d * f32(factor)).astype(f32), c0)
        assert all(np.array_equal(a, b) for a, b in zip(base, scaled)), factor


# ---- the device side ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def ctx():
    from chroma_amd import gpu as g
    c = g.create_cuda_context(0)
    yield c
    c.pop()


@pytest.fixture(scope='module')
def device_scenes(ctx):
    """name -> (geometry, packed, source, GPUGeometry), uploaded on first use."""
    from chroma_amd import gpu
    made = {}

    def get(name):
        if name not in made:
            g, packed, source = SCENES[name]()
            made[name] = (g, packed, source, gpu.GPUGeometry(g, packed=packed))
        return made[name]
    yield get
    made.clear()


def _f3(v):
    import ctypes
    return (ctypes.c_float * 3)(*[float(x) for x in v])


def _sentinels(rows, width=1):
    return np.full(rows * width, SENTINEL, np.uint32)


class Arrays(object):
    """Named device arrays with their host images before and after a call."""

    def __init__(self, ctx):
        self.ctx, self.dev, self.before = ctx, {}, {}

    def put(self, name, host):
        from chroma_amd.gpu.tools import GPUArray
        host = np.ascontiguousarray(host).reshape(-1)
        self.dev[name] = GPUArray(host.size, np.uint32, self.ctx).set(host.view(np.uint32))
        self.before[name] = host.view(np.uint32).copy()

    def ptr(self, name, give=True):
        return self.dev[name].ptr if give else None

    def run(self, fn, *args):
        """The call; a refusal carries these arrays (`arrays` of the ChromaError), so that a test can look at them."""
        from chroma_amd import _lib
        try:
            _lib.check(fn(self.ctx.handle, *args))
        except _lib.ChromaError as e:
            e.arrays = self
            raise
        return self

    def after(self):
        self.ctx.synchronize()
        return {name: a.get() for name, a in self.dev.items()}

    def assert_untouched(self, what, names=None):
        after = self.after()
        for name in (names or self.before):
            assert np.array_equal(after[name], self.before[name]), '%s: %s was written' % (what, name)


def _guarded(live):
    """`live` (uint32 view of the rows the call is told of) followed by GUARD rows of sentinels of the same width."""
    live = np.ascontiguousarray(live)
    width = 1 if live.ndim == 1 else live.shape[1]
    return np.concatenate([live.view(np.uint32).reshape(-1), _sentinels(GUARD, width)])


LOOKUP_SAMPLES = ('triangle', 'side', 'history', 'cos')
IMAGE_SAMPLES = ('triangle', 'side', 'history')


def call_lookup(ctx, gg, ntri, nthreads, total, offset, source, counters, tables, max_steps=10, xyz=XYZ, id_base=0,
                give=(True, True, True, True), nlookup=None):
    """One chroma_hybrid_lookup.  `counters`: the start values of the `ncounters` counters the call is told of; `tables`: the
    [ntri][3] start values of lookup1 and lookup2.  Sample arrays of max(nthreads, 0) rows, all sentinel; GUARD rows of
    sentinels behind every array.  Returns the Arrays (raises ChromaError when the call refuses)."""
    from chroma_amd import _lib
    a = Arrays(ctx)
    a.put('counters', _guarded(np.asarray(counters, np.uint32)))
    for name in LOOKUP_SAMPLES:
        a.put(name, _sentinels(max(nthreads, 0) + GUARD))
    a.put('lookup1', _guarded(np.asarray(tables[0], f32).reshape(ntri, 3)))
    a.put('lookup2', _guarded(np.asarray(tables[1], f32).reshape(ntri, 3)))
    return a.run(
        ctx._lib.chroma_hybrid_lookup, gg.gpudata, int(nthreads), int(total), int(offset), _f3(source), _lib.Rng(SEED, id_base), a.ptr('counters'),
        len(counters), float(WAVELENGTH), _f3(xyz), a.ptr('lookup1'), a.ptr('lookup2'), ntri if nlookup is None else nlookup,
        int(max_steps), *[a.ptr(name, g) for name, g in zip(LOOKUP_SAMPLES, give)])


def check_lookup(a, want, ntri, what, xyz=XYZ):
    """Everything one lookup launch must have done to its arrays, and nothing else.  Returns the tables after it."""
    after, before, n = a.after(), a.before, want.n
    for name, w in (('triangle', want.tri.view(np.uint32)), ('side', want.side), ('history', want.hist), ('cos', _bits(want.cos))):
        bad = np.flatnonzero(after[name][:n] != w)
        assert len(bad) == 0, '%s: %s differs from the oracle for %d of %d samples, first %d: %08x, oracle %08x' % (
            what, name, len(bad), n, bad[0], after[name][bad[0]], w[bad[0]])
        assert (after[name][n:] == SENTINEL).all(), '%s: %s was written past the last live thread' % (what, name)
    assert np.array_equal(after['counters'][:n], want.ctr), '%s: draw counters' % what
    assert np.array_equal(after['counters'][n:], before['counters'][n:]), '%s: a thread without a triangle drew, or a guard counter was written' % what
    l1, l2 = [before[k][:3 * ntri].view(f32).reshape(ntri, 3) for k in ('lookup1', 'lookup2')]
    w1, w2 = want.add_to(l1, l2, xyz)
    for name, w, start, s in (('lookup1', w1, l1, 1), ('lookup2', w2, l2, 0)):
        got = after[name][:3 * ntri].reshape(ntri, 3)
        bad = np.flatnonzero((got != _bits(w)).any(axis=1))
        assert len(bad) == 0, '%s: %s differs from hybrid_accumulate in %d rows, first triangle %d: %s, wanted %s' % (
            what, name, len(bad), bad[0], got[bad[0]].view(f32), w[bad[0]])
        idle = np.ones(ntri, bool)
        idle[want.tri[(want.tri >= 0) & (want.side == s)]] = False
        assert np.array_equal(got[idle], _bits(start)[idle]), '%s: a row of %s no sample diffused on was written' % (what, name)
        assert (after[name][3 * ntri:] == SENTINEL).all(), '%s: guard rows of %s were written' % (what, name)
    return w1, w2


def call_image(ctx, gg, ntri, origins, directions, counters, tables, image, nlookup_calls, max_steps=10, xyz=XYZ, id_base=0,
               give=(True, True, True), nthreads=None):
    """One chroma_hybrid_image over the n rays given.  `image`: the [nimage][3] start values (nimage >= n).  The ray arrays
    hold a ray that meets the scene in their GUARD rows; everything else as call_lookup."""
    from chroma_amd import _lib
    n = len(origins)
    a = Arrays(ctx)
    a.put('origins', np.concatenate([np.asarray(origins, f32), np.zeros((GUARD, 3), f32)]))
    a.put('directions', np.concatenate([np.asarray(directions, f32), np.tile(f32(INSIDE), (GUARD, 1))]))
    a.put('counters', _guarded(np.asarray(counters, np.uint32)))
    for name in IMAGE_SAMPLES:
        a.put(name, _sentinels(n + GUARD))
    a.put('lookup1', _guarded(np.asarray(tables[0], f32).reshape(ntri, 3)))
    a.put('lookup2', _guarded(np.asarray(tables[1], f32).reshape(ntri, 3)))
    image = np.asarray(image, f32).reshape(-1, 3)
    a.put('image', _guarded(image))
    return a.run(
        ctx._lib.chroma_hybrid_image, gg.gpudata, n if nthreads is None else int(nthreads), _lib.Rng(SEED, id_base), a.ptr('counters'), len(counters),
        a.ptr('origins'), a.ptr('directions'), float(WAVELENGTH), _f3(xyz), a.ptr('lookup1'), a.ptr('lookup2'), ntri, a.ptr('image'),
        len(image), int(nlookup_calls), int(max_steps), *[a.ptr(name, g) for name, g in zip(IMAGE_SAMPLES, give)])


def check_image(a, want, n, nlookup_calls, what, xyz=XYZ):
    """Everything one image launch must have done, and nothing else.  Returns (image rows told of, counters told of) after it."""
    after, before = a.after(), a.before
    tri, side, hist, ctr = want
    for name, w in (('triangle', tri.view(np.uint32)), ('side', side), ('history', hist)):
        bad = np.flatnonzero(after[name][:n] != w)
        assert len(bad) == 0, '%s: %s differs from the oracle for %d of %d rays, first %d: %08x, oracle %08x' % (
            what, name, len(bad), n, bad[0], after[name][bad[0]], w[bad[0]])
        assert (after[name][n:] == SENTINEL).all(), '%s: guard rows of %s were written' % (what, name)
    assert np.array_equal(after['counters'][:n], ctr), '%s: draw counters' % what
    for name in ('origins', 'directions', 'lookup1', 'lookup2'):
        assert np.array_equal(after[name], before[name]), '%s: %s was written' % (what, name)
    assert np.array_equal(after['counters'][n:], before['counters'][n:]), '%s: counters past the last ray were written' % what
    ntri = (len(before['lookup1']) - 3 * GUARD) // 3
    l1, l2 = [before[k][:3 * ntri].view(f32).reshape(ntri, 3) for k in ('lookup1', 'lookup2')]
    rows = len(before['image']) // 3
    start = before['image'].view(f32).reshape(rows, 3)
    w = start.copy()
    w[:n] = hybrid_image_update(start[:n].copy(), tri, side, l1, l2, xyz, nlookup_calls)
    got = after['image'].reshape(rows, 3)
    bad = np.flatnonzero((got != _bits(w)).any(axis=1))
    assert len(bad) == 0, '%s: image differs from hybrid_image_update in %d rows, first %d: %s, wanted %s' % (
        what, len(bad), bad[0], got[bad[0]].view(f32), w[bad[0]])
    assert np.array_equal(got[:n][tri < 0], _bits(start)[:n][tri < 0]) and np.array_equal(got[n:], _bits(start)[n:]), \
        '%s: the image row of a ray that did not diffuse, or a guard row, was written' % what
    return got[:rows - GUARD].view(f32).copy(), after['counters'][:len(after['counters']) - GUARD].copy()


def call_pixels(ctx, n, image, nimages):
    """One chroma_hybrid_pixels over n pixels of `image` ([rows][3], rows >= n), the pixel array all sentinel."""
    a = Arrays(ctx)
    image = np.asarray(image, f32).reshape(-1, 3)
    a.put('image', image)
    a.put('pixels', _sentinels(len(image)))
    return a.run(ctx._lib.chroma_hybrid_pixels, int(n), a.ptr('image'), a.ptr('pixels'), int(nimages))


# ---- 1. lookup launch sizes, on each arm of the cap ---------------------------------------------------------------------
SIZE_CASES = [(scene, n) for scene in ('room_sphere', 'room_sheet_mirror') for n in SIZES] + [('grey_stress', n) for n in STRESS_SIZES]
ID_BASES = {'room_sphere': 0, 'room_sheet_mirror': 129, 'grey_stress': BIG_ID}


def _size_launch(scene, n, arm):
    """(nthreads, total_threads, offset, ncounters) that leave n live threads, capped by `arm` of
    min(offset + nthreads, total_threads, ntriangles)."""
    nt = _ntri(scene)
    if arm == 'nthreads':
        return n, nt, 0, n
    if arm == 'total':
        return n + 40, n, 0, n + 45
    return n + 40, nt + 100, nt - n, n + 40                     # 'ntriangles': a chunk that runs past the last triangle


@gpu_test
@pytest.mark.parametrize('arm', ['nthreads', 'total', 'ntriangles'])
@pytest.mark.parametrize('scene,n', SIZE_CASES)
def test_lookup_sizes_on_each_arm_of_the_cap(scene, n, arm, ctx, device_scenes, oracle_mod):
    g, packed, source, gg = device_scenes(scene)
    nt = len(g.mesh.triangles)
    nthreads, total, offset, ncounters = _size_launch(scene, n, arm)
    counters = _start_counters(ncounters)
    tables = (_start_table(nt, 1), _start_table(nt, 2))
    want = want_lookup(oracle_mod, scene, n, offset, counters, id_base=ID_BASES[scene])
    a = call_lookup(ctx, gg, nt, nthreads, total, offset, source, counters, tables, id_base=ID_BASES[scene])
    check_lookup(a, want, nt, '%s, %d live threads by %s' % (scene, n, arm))


@gpu_test
@pytest.mark.parametrize('scene', ['room', 'room_sphere'])
def test_lookup_with_no_live_thread_touches_nothing(scene, ctx, device_scenes):
    g, packed, source, gg = device_scenes(scene)
    nt = len(g.mesh.triangles)
    tables = (_start_table(nt, 3), _start_table(nt, 4))
    for nthreads, total, offset in ((65, 40, 40), (65, 40, 41), (65, nt, nt), (65, nt + 500, nt), (65, nt + 500, nt + 129),
                                    (0, nt, 0), (0, nt, 5), (65, 0, 0)):
        a = call_lookup(ctx, gg, nt, nthreads, total, offset, source, _start_counters(70), tables)
        a.assert_untouched('%s: nthreads %d, total_threads %d, offset %d' % (scene, nthreads, total, offset))


# ---- 2. the runs of k_hybrid_reduce --------------------------------------------------------------------------------------
@gpu_test
def test_reduce_a_run_of_eight_blocks_twice_onto_the_same_tables(ctx, device_scenes, oracle_mod):
    """room_sphere's full launch from zero tables, then once more from where it left counters and tables: more than two
    thousand samples on one key, summed in sample order and added once, the second time onto what the first left."""
    g, packed, source, gg = device_scenes('room_sphere')
    nt = len(g.mesh.triangles)
    counters, tables = np.zeros(nt, np.uint32), (np.zeros((nt, 3), f32), np.zeros((nt, 3), f32))
    for k in range(2):
        want = want_lookup(oracle_mod, 'room_sphere', nt, 0, counters)
        a = call_lookup(ctx, gg, nt, nt, nt, 0, source, counters, tables)
        tables = check_lookup(a, want, nt, 'room_sphere, full launch %d' % k)
        counters = want.ctr
    assert max(np.abs(tables[0]).max(), np.abs(tables[1]).max()) > 513 * 0.3 * 0.5 * 0.1         # light of many samples in one entry


@gpu_test
def test_reduce_a_long_run_that_starts_at_record_zero(ctx, device_scenes, oracle_mod):
    g, packed, source, gg = device_scenes('room_sphere')
    nt = len(g.mesh.triangles)
    counters, tables = np.zeros(nt - 16, np.uint32), (_start_table(nt, 5), _start_table(nt, 6))
    want = want_lookup(oracle_mod, 'room_sphere', nt - 16, 16, counters)
    check_lookup(call_lookup(ctx, gg, nt, nt - 16, nt, 16, source, counters, tables), want, nt, 'room_sphere from triangle 16')


@gpu_test
@pytest.mark.parametrize('scene,source', [('room_sheet_mirror', None), ('sheet_mirror32', None), ('room', None), ('room', OUTSIDE_SOURCE)])
def test_reduce_neighbouring_keys_key_zero_and_the_last_record(scene, source, ctx, device_scenes, oracle_mod):
    """Full launches of the small scenes, onto zero tables and onto lit ones: both sides of one triangle as keys 2t and 2t + 1
    (room_sheet_mirror); a power-of-two triangle count, where key_none is the only key with the top bit, with the records of
    key 0 between key_none's (sheet_mirror32) or a few one-record keys among them (the room from outside); no key_none at all,
    so the last record ends a run (the room from inside)."""
    g, packed, src, gg = device_scenes(scene)
    nt = len(g.mesh.triangles)
    counters = np.zeros(nt, np.uint32)
    want = want_lookup(oracle_mod, scene, nt, 0, counters, source=source)
    for what, tables in (('zero', (np.zeros((nt, 3), f32), np.zeros((nt, 3), f32))), ('lit', (_start_table(nt, 7), _start_table(nt, 8)))):
        a = call_lookup(ctx, gg, nt, nt, nt, 0, src if source is None else source, counters, tables)
        check_lookup(a, want, nt, '%s, full launch onto %s tables' % (scene, what))


# ---- 3. max_steps 0 and 1 ------------------------------------------------------------------------------------------------
@gpu_test
@pytest.mark.parametrize('max_steps', [0, 1])
@pytest.mark.parametrize('scene', ['room', 'room_sheet_mirror', 'grey_stress'])
def test_lookup_and_image_at_max_steps_0_and_1(scene, max_steps, ctx, device_scenes, oracle_mod):
    """At 0 the step loop does not run: no history, no triangle, tables and image untouched (every key is key_none), the
    counters advanced by the draws made before the loop (2 for the point on the triangle, 2 more for the polarisation of a
    sample that reached it).  At 1 a sample diffuses on the triangle it was aimed at or not at all."""
    g, packed, source, gg = device_scenes(scene)
    nt = len(g.mesh.triangles)
    n, offset = nt, 0
    counters = _start_counters(n + 7)
    tables = (_start_table(nt, 9), _start_table(nt, 10))
    want = want_lookup(oracle_mod, scene, n, offset, counters, max_steps=max_steps)
    a = call_lookup(ctx, gg, nt, n, nt, offset, source, counters, tables, max_steps=max_steps)
    check_lookup(a, want, nt, '%s at max_steps %d' % (scene, max_steps))
    after = a.after()
    tri = after['triangle'][:n].view(np.int32)
    if max_steps == 0:
        assert (tri == -1).all() and (after['history'][:n] == 0).all() and (after['side'][:n] == 0).all()
        assert np.array_equal(after['counters'][:n], counters[:n] + np.where(want.mine, 4, 2).astype(np.uint32))
        a.assert_untouched('%s at max_steps 0' % scene, ('lookup1', 'lookup2'))
    else:
        assert (tri[tri >= 0] == offset + np.flatnonzero(tri >= 0)).all()
        assert (after['history'][:n][tri >= 0] == REFLECT_DIFFUSE).all()
    if scene == 'room_sheet_mirror':
        o, d = camera_bundle(129)
        c0 = _start_counters(129)
        wi = want_image(oracle_mod, scene, o, d, c0, max_steps=max_steps)
        ai = call_image(ctx, gg, nt, o, d, c0, want_tables(oracle_mod, scene), _start_table(129, 11), 3, max_steps=max_steps)
        check_image(ai, wi, 129, 3, 'image at max_steps %d' % max_steps)
        if max_steps == 0:
            ai.assert_untouched('image at max_steps 0', ('image',))
            assert (ai.after()['history'][:129] == 0).all() and np.array_equal(ai.after()['counters'][:129], c0 + np.uint32(2))


# ---- 4. the image pass ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def mirror_tables(ctx, device_scenes, oracle_mod):
    """lookup1 and lookup2 of room_sheet_mirror as one full launch on the device fills them from zero."""
    g, packed, source, gg = device_scenes('room_sheet_mirror')
    nt = len(g.mesh.triangles)
    a = call_lookup(ctx, gg, nt, nt, nt, 0, source, np.zeros(nt, np.uint32), (np.zeros((nt, 3), f32), np.zeros((nt, 3), f32)))
    after = a.after()
    l1, l2 = [after[k][:3 * nt].view(f32).reshape(nt, 3).copy() for k in ('lookup1', 'lookup2')]
    w1, w2 = want_tables(oracle_mod, 'room_sheet_mirror')
    assert np.array_equal(_bits(l1), _bits(w1)) and np.array_equal(_bits(l2), _bits(w2)) and l1.any() and l2.any()
    return l1, l2


@gpu_test
@pytest.mark.parametrize('n', SIZES)
def test_image_sizes_two_passes_onto_a_lit_image(n, ctx, device_scenes, oracle_mod, mirror_tables):
    """Two passes in a row, the second continuing the first's counters and adding onto its image; the image starts non-zero
    and is told to be longer than the bundle for every second size."""
    g, packed, source, gg = device_scenes('room_sheet_mirror')
    nt = len(g.mesh.triangles)
    o, d = camera_bundle(n)
    nimage = n + (5 if SIZES.index(n) % 2 else 0)
    ncounters = n + (0 if SIZES.index(n) % 2 else 3)
    nlookup_calls = (1, 3, 7)[SIZES.index(n) % 3]
    counters, image = _start_counters(ncounters), _start_table(nimage, 12)
    for k in range(2):
        want = want_image(oracle_mod, 'room_sheet_mirror', o, d, counters)
        a = call_image(ctx, gg, nt, o, d, counters, mirror_tables, image, nlookup_calls)
        image2, counters = check_image(a, want, n, nlookup_calls, '%d rays, pass %d' % (n, k))
        assert n < 63 or not np.array_equal(_bits(image2), _bits(image))
        image = image2


@gpu_test
@pytest.mark.parametrize('nlookup_calls', [1, 3, 7])
def test_image_divides_by_the_lookup_calls(nlookup_calls, ctx, device_scenes, oracle_mod, mirror_tables):
    g, packed, source, gg = device_scenes('room_sheet_mirror')
    o, d = camera_bundle(257)
    c0 = _start_counters(257)
    want = want_image(oracle_mod, 'room_sheet_mirror', o, d, c0)
    a = call_image(ctx, gg, len(g.mesh.triangles), o, d, c0, mirror_tables, np.zeros((257, 3), f32), nlookup_calls)
    image, _ = check_image(a, want, 257, nlookup_calls, 'nlookup_calls %d' % nlookup_calls)
    assert image.any()


@gpu_test
def test_image_normalises_scaled_directions(ctx, device_scenes, oracle_mod, mirror_tables):
    g, packed, source, gg = device_scenes('room_sheet_mirror')
    o, d, scale = scaled_bundle()
    c0 = _start_counters(129)
    want = want_image(oracle_mod, 'room_sheet_mirror', o, d, c0)
    a = call_image(ctx, gg, len(g.mesh.triangles), o, d, c0, mirror_tables, _start_table(129, 13), 3)
    check_image(a, want, 129, 3, 'directions scaled by 0.25 and 1e3')
    # a quarter as long is exact in f32: those rays are the unscaled bundle's
    unscaled = want_image(oracle_mod, 'room_sheet_mirror', *camera_bundle(129), c0)
    quarter = scale == f32(0.25)
    assert np.array_equal(a.after()['triangle'][:129][quarter], unscaled[0].view(np.uint32)[quarter])


@gpu_test
def test_image_of_rays_that_leave_the_world(ctx, device_scenes, oracle_mod, mirror_tables):
    g, packed, source, gg = device_scenes('room_sheet_mirror')
    o, d = outside_bundle()
    c0 = _start_counters(129)
    want = want_image(oracle_mod, 'room_sheet_mirror', o, d, c0)
    a = call_image(ctx, gg, len(g.mesh.triangles), o, d, c0, mirror_tables, _start_table(129, 14), 1)
    check_image(a, want, 129, 1, 'outside bundle')
    after = a.after()
    assert (after['history'][:129] == NO_HIT).all() and (after['triangle'][:129].view(np.int32) == -1).all()
    assert np.array_equal(after['counters'][:129], c0 + np.uint32(2))           # the polarisation's two draws
    a.assert_untouched('outside bundle', ('image',))


@gpu_test
def test_image_with_a_zero_and_a_nan_direction(ctx, device_scenes, oracle_mod, mirror_tables):
    """The two rays end with NO_HIT | NAN_ABORT before their first step (to_diffuse, hybrid_render.cu:27-31); the rays of the
    same wave are those of the bundle without them."""
    g, packed, source, gg = device_scenes('room_sheet_mirror')
    o, d = broken_bundle()
    c0 = _start_counters(65)
    want = want_image(oracle_mod, 'room_sheet_mirror', o, d, c0)
    a = call_image(ctx, gg, len(g.mesh.triangles), o, d, c0, mirror_tables, _start_table(65, 15), 7)
    check_image(a, want, 65, 7, 'zero and NaN directions')
    after = a.after()
    broken = [ZERO_RAY, NAN_RAY]
    assert (after['history'][broken] == (NO_HIT | NAN_ABORT)).all() and (after['triangle'][broken].view(np.int32) == -1).all()
    assert np.array_equal(after['counters'][broken], c0[broken] + np.uint32(2))
    assert np.array_equal(after['image'].reshape(-1, 3)[broken], a.before['image'].reshape(-1, 3)[broken])
    good = np.delete(np.arange(65), broken)
    whole = want_image(oracle_mod, 'room_sheet_mirror', *camera_bundle(65), c0)
    for name, w in zip(IMAGE_SAMPLES, whole):
        assert np.array_equal(after[name][:65][good], w.view(np.uint32)[good]), name


# ---- 5. pixels, without a geometry ---------------------------------------------------------------------------------------
def _pixel_values():
    """The channel values k_hybrid_pixels branches on, and each times 3 and times 255 (so that it meets the same branches
    after the division by nimages)."""
    one = f32(1)
    v = [np.nan, np.inf, -np.inf, -0.0, -1e-45, 1e-45, 0.0, 1.0, np.nextafter(one, f32(0)), np.nextafter(one, f32(2)), 2.0, -1.0,
         3.0e38, -3.0e38, 0.5]
    for k in (1, 2, 3, 127, 128, 254, 255):
        for num in (k, k + 0.5):
            x = f32(num / 255.0)
            v += [np.nextafter(x, f32(-1)), x, np.nextafter(x, f32(2))]
    v = np.array(v, f32)
    with np.errstate(over='ignore'):
        return np.concatenate([v, v * f32(3), v * f32(255)]).astype(f32)


def _pixel_image(rows):
    v = _pixel_values()
    i = np.arange(rows)
    return np.stack([v[i % len(v)], v[(i + 5) % len(v)], v[(3 * i + 11) % len(v)]], axis=1).astype(f32)


def test_the_pixel_image_holds_every_branch():
    """The restatement on the values the device test uses, against plain Python arithmetic for the ones that need no rounding
    argument, and the coverage of the k / 255 boundaries counted."""
    v = _pixel_values()
    assert len(v) < 257                                           # every value is in the red channel of the largest image
    px = hybrid_pixels(np.stack([v, v, v], axis=1), 1)
    assert (px >> 24 == 0xFF).all()
    red = (px >> 16) & 0xFF
    for x, want in ((np.nan, 0), (np.inf, 255), (-np.inf, 0), (-0.0, 0), (-1e-45, 0), (0.0, 0), (1.0, 255), (2.0, 255), (-1.0, 0),
                    (0.5, 127), (np.nextafter(f32(1), f32(0)), 254), (3.0e38, 255)):
        sel = np.flatnonzero(_bits(v) == _bits(f32(x))) if not np.isnan(x) else np.flatnonzero(np.isnan(v))
        assert len(sel) and (red[sel] == want).all(), (x, red[sel])
    for nimages in (1, 3, 255):
        r = (hybrid_pixels(np.stack([v, v, v], axis=1), nimages) >> 16) & 0xFF
        assert len(np.unique(r)) >= 10                              # both sides of several k / 255 steps
        assert sorted(set(np.unique(r)) & {0, 1, 127, 128, 254, 255}) == [0, 1, 127, 128, 254, 255]


@gpu_test
@pytest.mark.parametrize('nimages', [1, 3, 255])
@pytest.mark.parametrize('n', PIXEL_SIZES)
def test_pixels_clamp_floor_and_pack(n, nimages, ctx):
    image = _pixel_image(n + GUARD)
    a = call_pixels(ctx, n, image, nimages)
    after = a.after()
    want = hybrid_pixels(image[:n], nimages)
    bad = np.flatnonzero(after['pixels'][:n] != want)
    assert len(bad) == 0, '%d of %d pixels differ, first %d: %08x, wanted %08x of %s' % (len(bad), n, bad[0], after['pixels'][bad[0]],
                                                                                       want[bad[0]], image[bad[0]])
    assert (after['pixels'][:n] >> 24 == 0xFF).all()
    assert (after['pixels'][n:] == SENTINEL).all(), 'guard pixels were written'
    a.assert_untouched('pixels', ('image',))


@gpu_test
def test_pixels_of_no_pixel_touch_nothing(ctx):
    call_pixels(ctx, 0, _pixel_image(65), 1).assert_untouched('no pixels')


# ---- 6. refusals not covered by test_bad_arguments_are_refused_before_any_launch ----------------------------------------
@gpu_test
def test_refusals_leave_every_array_untouched(ctx, device_scenes, oracle_mod):
    from chroma_amd import _lib
    g, packed, source, gg = device_scenes('room_sheet_mirror')
    nt = len(g.mesh.triangles)
    tables = (_start_table(nt, 16), _start_table(nt, 17))

    def refused(what, fn, *args, **kw):
        with pytest.raises(_lib.ChromaError) as info:
            fn(*args, **kw)
        info.value.arrays.assert_untouched(what)

    counters = _start_counters(129)
    for give in ((True, False, False, False), (False, True, True, True), (True, True, False, True), (True, False, True, True),
                 (False, False, False, True), (True, True, True, False), (False, False, True, False)):
        refused('lookup with sample outputs %s' % (give,), call_lookup, ctx, gg, nt, 129, nt, 0, source, counters, tables, give=give)
    for nthreads, total, offset in ((129, nt, -1), (129, -1, 0), (-1, nt, 0), (-129, nt, 0), (129, nt, -(2 ** 31))):
        refused('lookup with nthreads %d, total_threads %d, offset %d' % (nthreads, total, offset), call_lookup, ctx, gg, nt, nthreads, total,
                offset, source, counters, tables)
    o, d = camera_bundle(129)
    image = _start_table(129, 18)
    for give in ((True, False, False), (True, True, False), (False, True, True), (False, False, True)):
        refused('image with sample outputs %s' % (give,), call_image, ctx, gg, nt, o, d, counters, tables, image, 1, give=give)
    for nlookup_calls in (0, -1):
        refused('image with nlookup_calls %d' % nlookup_calls, call_image, ctx, gg, nt, o, d, counters, tables, image, nlookup_calls)
    refused('image with a negative ray count', call_image, ctx, gg, nt, o, d, counters, tables, image, 1, nthreads=-1)
    refused('pixels with a negative count', call_pixels, ctx, -1, _pixel_image(65), 1)
    # and the calls still work afterwards
    want = want_lookup(oracle_mod, 'room_sheet_mirror', 129, 0, counters)
    check_lookup(call_lookup(ctx, gg, nt, 129, nt, 0, source, counters, tables), want, nt, 'after the refusals')
