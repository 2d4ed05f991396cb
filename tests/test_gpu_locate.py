"""chroma_locate_materials: the material each point lies in, against the CPU oracle's ray cast followed by a NumPy float32
restatement of fill_state's choice of side, and its deciding triangle against chroma_intersect_mesh for the same rays."""
import ctypes

import numpy as np
import pytest

from chroma_amd import _lib
from chroma_amd.geometry import Geometry, Material, Solid

pytestmark = pytest.mark.gpu

f32 = np.float32
SIZES = (0, 1, 63, 64, 65, 257, 4099)
DIRECTIONS = {'default': None, 'generic': (0.31, -0.52, 0.79)}
OUTSIDE = -7
OUTER, INNER = 200.0, 80.0          # edges of the two nested boxes, mm


def plain(name, n):
    m = Material(name)
    m.set('refractive_index', n)
    m.set('absorption_length', 1e6)
    m.set('scattering_length', 1e6)
    return m


def nested_boxes(materials=None, inner_surface=None):
    """A box of B inside a box of A, the outer box's outer material C (also the material around everything); the rows of
    A, B, C in unique_materials are read off the geometry.  ``inner_surface``: a Detector whose one channel is the inner box."""
    from chroma_amd.detector import Detector
    from chroma_amd.loader import create_geometry_from_obj
    from chroma_amd.make import box
    a, b, c = materials or (plain('A', 1.5), plain('B', 1.4), plain('C', 1.0))
    g = Geometry(c) if inner_surface is None else Detector(c)
    g.add_solid(Solid(box(OUTER, OUTER, OUTER), a, c))
    inner = Solid(box(INNER, INNER, INNER), b, a, surface=inner_surface)
    if inner_surface is None:
        g.add_solid(inner)
    else:
        g.add_pmt(inner)
    return create_geometry_from_obj(g), (a, b, c)


def probe_points(edges, n=max(SIZES), seed=5):
    """The exact centre, the points 1e-3 mm either side of every face centre of the boxes with these edges, then uniform
    points in a cube 1.5 x the largest box: the first n of them."""
    special = [(0.0, 0.0, 0.0)]
    for edge in edges:
        for axis in range(3):
            for sign in (-1.0, 1.0):
                for off in (-1e-3, 1e-3):
                    p = [0.0, 0.0, 0.0]
                    p[axis] = sign * (edge / 2.0 + off)
                    special.append(tuple(p))
    rng = np.random.default_rng(seed)
    half = 0.75 * max(edges)
    pts = np.concatenate([np.array(special), rng.uniform(-half, half, (n - len(special), 3))])
    return np.ascontiguousarray(pts, dtype=np.float32)


def expected_materials(geometry, packed_codes, points, direction, tri):
    """fill_state's rule (photon.h:99-120) in float32 NumPy on the oracle's triangle: (material, |dot(normal, d)|)."""
    d = np.asarray((0.0, 0.0, 1.0) if direction is None else direction, dtype=f32)
    d = d / np.sqrt((d * d).sum(dtype=f32), dtype=f32)
    mesh = geometry.mesh
    hit = tri >= 0
    v = mesh.vertices.astype(f32)[mesh.triangles[np.where(hit, tri, 0)]]
    normal = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 1]).astype(f32)
    normal = normal / np.sqrt((normal * normal).sum(axis=1, dtype=f32), dtype=f32)[:, None]
    cos = (normal * -d).sum(axis=1, dtype=f32)
    code = packed_codes[np.where(hit, tri, 0)]
    material = np.where(cos > 0, (code >> 16) & 0xFF, (code >> 24) & 0xFF).astype(np.int32)
    return np.where(hit, material, OUTSIDE).astype(np.int32), np.where(hit, np.abs(cos), 1.0)


@pytest.fixture(scope='module')
def gpu():
    from chroma_amd import gpu as g
    ctx = g.create_cuda_context(0)
    yield g
    ctx.pop()


class Scene(object):
    def __init__(self, gpu, oracle_mod, geometry, edges):
        from chroma_amd.gpu.geometry import pack_geometry
        self.geometry = geometry
        packed = pack_geometry(geometry)
        codes = np.array(packed.arrays['material_codes'], dtype=np.uint32)
        self.points = probe_points(edges)
        self.want = {}
        for name, direction in DIRECTIONS.items():
            d = np.tile(np.asarray((0, 0, 1) if direction is None else direction, dtype=np.float32), (len(self.points), 1))
            _, tri, _ = oracle_mod.distance_to_mesh(packed, self.points, d)
            self.want[name] = (tri,) + expected_materials(geometry, codes, self.points, direction, tri)
        self.gg = gpu.GPUGeometry(geometry)


@pytest.fixture(scope='module')
def boxes(gpu, oracle_mod):
    geometry, materials = nested_boxes()
    scene = Scene(gpu, oracle_mod, geometry, (OUTER, INNER))
    scene.rows = [geometry.unique_materials.index(m) for m in materials]
    return scene


@pytest.fixture(scope='module')
def stress(gpu, oracle_mod):
    from conftest import make_stress_geometry
    return Scene(gpu, oracle_mod, make_stress_geometry(), (2000.0, 200.0))


def intersect_mesh(gpu, gg, points, direction):
    ctx, n = gg.ctx, len(points)
    d = np.tile(np.asarray((0, 0, 1) if direction is None else direction, dtype=np.float32), (n, 1))
    d_o, d_d = gpu.to_gpu(points.reshape(-1), ctx), gpu.to_gpu(d.reshape(-1), ctx)
    dist, tri = gpu.empty(n, np.float32, ctx), gpu.empty(n, np.int32, ctx).fill(-5)
    _lib.check(ctx._lib.chroma_intersect_mesh(ctx.handle, gg.handle, n, d_o.ptr, d_d.ptr, None, dist.ptr, tri.ptr), ctx._lib)
    return tri.get()


def check(gpu, scene, name, n):
    direction = DIRECTIONS[name]
    points = scene.points[:n]
    material, triangle = gpu.steps.locate_materials(points, scene.gg, direction=direction, outside=OUTSIDE, return_triangles=True)
    material, triangle = material.get(), triangle.get()
    assert len(material) == len(triangle) == n
    if n == 0:
        return
    # the deciding triangle is chroma_intersect_mesh's for the same rays: exactly, every ray
    assert np.array_equal(triangle, intersect_mesh(gpu, scene.gg, points, direction))
    tri, want, cos = (x[:n] for x in scene.want[name])
    # ... and the oracle's; the material follows from it wherever the ray does not graze its triangle
    assert np.array_equal(triangle, tri)
    grazing = cos < 1e-5
    assert grazing.sum() <= 0.005 * n, grazing.sum()
    assert np.array_equal(material[~grazing], want[~grazing])
    assert (material[tri < 0] == OUTSIDE).all()
    # without the triangles asked for, the same materials
    assert np.array_equal(gpu.steps.locate_materials(gpu.to_gpu(points.reshape(-1), scene.gg.ctx), scene.gg, direction=direction, outside=OUTSIDE).get(), material)
    return material


@pytest.mark.parametrize('n', SIZES)
@pytest.mark.parametrize('name', sorted(DIRECTIONS))
def test_nested_boxes(gpu, boxes, name, n):
    material = check(gpu, boxes, name, n)
    if n < 63:
        return
    a, b, c = boxes.rows
    p = boxes.points[:n].astype(np.float64)
    r = np.abs(p).max(axis=1)                  # Chebyshev distance from the centre: which box a point is in
    analytic = np.where(r < INNER / 2, b, np.where(r < OUTER / 2, a, c))
    inside = r < OUTER / 2
    assert np.array_equal(material[inside], analytic[inside])
    assert material[0] == b and {a, b, c, OUTSIDE} >= set(material.tolist()) and {a, b} <= set(material.tolist())
    # outside the outer box: C where the probe ray meets the box, `outside` where it meets nothing
    assert set(material[~inside].tolist()) <= {c, OUTSIDE} and (material[~inside] == OUTSIDE).any()
    # the 24 points 1e-3 mm either side of the face centres (in probe_points' order: inside, then outside the face)
    faces = material[1:25].reshape(2, 3, 2, 2)
    assert (faces[0, ..., 0] == a).all() and (faces[1, ..., 0] == b).all() and (faces[1, ..., 1] == a).all()


@pytest.mark.parametrize('n', SIZES)
@pytest.mark.parametrize('name', sorted(DIRECTIONS))
def test_stress_geometry(gpu, stress, name, n):
    material = check(gpu, stress, name, n)
    if n >= 257:
        assert OUTSIDE in material and len(set(material.tolist())) >= 3


def test_bad_arguments_are_refused(gpu, boxes):
    ctx, gg = boxes.gg.ctx, boxes.gg
    pts = gpu.to_gpu(boxes.points[:4].reshape(-1), ctx)
    out = gpu.empty(4, np.int32, ctx)
    lib = ctx._lib
    zero = (ctypes.c_float * 3)(0.0, 0.0, 0.0)
    assert lib.chroma_locate_materials(ctx.handle, gg.handle, 4, pts.ptr, zero, -1, out.ptr, None) == -1
    assert b'direction' in lib.chroma_last_error()
    assert lib.chroma_locate_materials(ctx.handle, gg.handle, -1, pts.ptr, None, -1, out.ptr, None) == -1
    assert b'negative' in lib.chroma_last_error()
    assert lib.chroma_locate_materials(ctx.handle, gg.handle, 4, None, None, -1, out.ptr, None) == -1
    assert lib.chroma_locate_materials(ctx.handle, gg.handle, 4, pts.ptr, None, -1, None, None) == -1
    assert lib.chroma_locate_materials(ctx.handle, gg.handle, 0, pts.ptr, None, -1, out.ptr, None) == 0
