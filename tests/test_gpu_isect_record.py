"""The 48-byte intersection records the fast walks' triangle test reads (GeoView::tri_isect, csrc/device_common.h), and
that test itself (intersect_triangle_edges, csrc/propagate_device.h).

  * Every record equals a NumPy float32 restatement: e1 = v1 - v0, e2 = v2 - v0, v0, and the rank of the 48-byte vertex
    record of the same index, in the layout {e1.x, e2.x, e1.y, e2.y} {e1.z, e2.z, v0.x, v0.y} {v0.z, rank, 0, 0}.
  * Through chroma_distance_to_mesh (both the default quad walk and the literal walk, whose triangle tests are now all
    in the edge form), every hit's distance equals, bit for bit, the vertex-form Moeller-Trumbore of intersect_triangle
    restated in NumPy float32 for that ray and triangle -- on random rays, on rays nearly parallel to the triangle they
    aim at, and on the 3.6e5 aimed rays of C3 -- and the literal walk equals the oracle (the vertex form in the
    reference's arithmetic) on every ray."""
import gc

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CHUNK = 1 << 23                 # records compared at a time (C3 holds ~170 M)
MT_NEG_EPS = np.uint32(0xB58637BD).view(np.float32)
MT_ONE_EPS = np.uint32(0x3F800008).view(np.float32)
MT_POS_EPS = np.uint32(0x358637BD).view(np.float32)
FLT_EPSILON = np.float32(np.finfo(np.float32).eps)


@pytest.fixture(scope='module')
def gpu():
    from chroma_amd import gpu as g
    ctx = g.create_cuda_context(0)
    yield g
    ctx.pop()


def _slice(gg, name, first, count, width, dtype):
    from chroma_amd.gpu.tools import GPUArray
    arr = gg._device_array(name, dtype)
    item = np.dtype(dtype).itemsize
    assert arr.size % width == 0
    return GPUArray.from_pointer(arr.ptr + first * width * item, count * width, dtype, gg, ctx=arr.ctx).get().reshape(count, width)


def check_isect_records(gg, packed):
    vertices = packed.arrays['vertices'].reshape(-1, 3)
    triangles = packed.arrays['triangles'].reshape(-1, 3)
    dev_to_tri = gg._device_array('dev_to_tri', np.uint32).get()
    nrecords = len(dev_to_tri)
    arr = gg._device_array('triangle_isect', np.float32)
    assert arr.size == 12 * nrecords and arr.ptr % 16 == 0
    for first in range(0, nrecords, CHUNK):
        n = min(CHUNK, nrecords - first)
        got = _slice(gg, 'triangle_isect', first, n, 12, np.float32).view(np.uint32)
        v = vertices[triangles[dev_to_tri[first:first + n]]]                   # [n][3 vertices][xyz], float32
        v0, e1, e2 = v[:, 0], v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]
        want = np.zeros((n, 12), np.float32)
        want[:, 0:6:2] = e1
        want[:, 1:6:2] = e2
        want[:, 6:9] = v0
        want = want.view(np.uint32)
        want[:, 9] = _slice(gg, 'triangle_records', first, n, 12, np.uint32)[:, 11]          # the rank
        assert np.array_equal(got, want), 'intersection records %d..%d' % (first, first + n)
        del got, v, v0, e1, e2, want


def _dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1],
                     a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                     a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)


def vertex_form(o, d, v0, v1, v2):
    """intersect_triangle (csrc/propagate_device.h) in float32: (hit, distance) per row."""
    with np.errstate(all='ignore'):
        edge1, edge2 = v1 - v0, v2 - v0
        h = _cross(d, edge2)
        a = _dot(edge1, h)
        f = np.float32(1.0) / a
        s = o - v0
        u = f * _dot(s, h)
        q = _cross(s, edge1)
        v = f * _dot(d, q)
        t = f * _dot(edge2, q)
        hit = ~((a > -FLT_EPSILON) & (a < FLT_EPSILON)) & ~((u < MT_NEG_EPS) | (u > MT_ONE_EPS)) & \
            ~((v < MT_NEG_EPS) | ((u + v) > MT_ONE_EPS)) & (t > MT_POS_EPS) & (t < np.float32(np.inf))
    return hit, t


def _normalised(d):
    """k_rays_from_arrays' direction / norm(direction), in float32."""
    d = d.astype(np.float32)
    n = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    return d / n[:, None]


def cast(gpu, gg, o, d, walk):
    from chroma_amd import _lib
    from chroma_amd.gpu.tools import to_gpu, GPUArray
    ctx = gpu.get_context()
    n = len(o)
    d_o, d_d = to_gpu(np.ascontiguousarray(o, np.float32).reshape(-1), ctx), to_gpu(np.ascontiguousarray(d, np.float32).reshape(-1), ctx)
    ctx.set_walk(walk)
    try:
        dist = GPUArray(n, np.float32, ctx).fill(np.float32(-1.0))
        tri = GPUArray(n, np.int32, ctx).fill(np.int32(-1))
        _lib.check(ctx._lib.chroma_distance_to_mesh(ctx.handle, gg.handle, n, d_o.ptr, d_d.ptr, dist.ptr, tri.ptr))
        return tri.get(), dist.get()
    finally:
        ctx.set_walk('quad')


def check_hits_are_the_vertex_form(gpu, gg, packed, o, d, oracle_mod=None, min_hits=0.0):
    vertices = packed.arrays['vertices'].reshape(-1, 3)
    triangles = packed.arrays['triangles'].reshape(-1, 3)
    o = np.ascontiguousarray(o, np.float32)
    dn = _normalised(d)
    results = {}
    for walk in ('quad', 'literal'):
        tri, dist = cast(gpu, gg, o, d, walk)
        hit = tri >= 0
        assert hit.mean() >= min_hits, (walk, hit.mean())
        v = vertices[triangles[tri[hit]]]
        ok, t = vertex_form(o[hit], dn[hit], v[:, 0], v[:, 1], v[:, 2])
        assert ok.all(), '%s walk: %d hits the vertex form misses' % (walk, np.count_nonzero(~ok))
        assert np.array_equal(t.view(np.uint32), dist[hit].view(np.uint32)), '%s walk: %d distances differ from the vertex form' % (
            walk, np.count_nonzero(t.view(np.uint32) != dist[hit].view(np.uint32)))
        results[walk] = (tri, dist)
    if oracle_mod is not None:
        wd, wt, _ = oracle_mod.distance_to_mesh(packed, o, d.astype(np.float32))
        ltri, ldist = results['literal']
        assert np.array_equal(ltri, wt), 'literal walk: %d rays differ from the oracle' % np.count_nonzero(ltri != wt)
        h = wt >= 0
        assert np.array_equal(ldist[h].view(np.uint32), wd[h].view(np.uint32))
    return results


def random_rays(rng, n, lo, hi):
    o = rng.uniform(lo, hi, (n, 3)).astype(np.float32)          # (inside the world box)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    return o, d


def grazing_rays(rng, packed, n):
    """Rays aimed at a point inside a triangle from far along its plane, tilted out of it by ~1e-4..1e-7 radians: a tiny
    `a`, a large 1/a."""
    vertices = packed.arrays['vertices'].reshape(-1, 3).astype(np.float64)
    triangles = packed.arrays['triangles'].reshape(-1, 3)
    pick = rng.integers(0, len(triangles), n)
    v = vertices[triangles[pick]]
    w = rng.dirichlet([1.0, 1.0, 1.0], n)
    target = (w[:, :, None] * v).sum(axis=1)
    e1, e2 = v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]
    nrm = np.cross(e1, e2)
    nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    along = e1 / np.linalg.norm(e1, axis=1)[:, None]
    tilt = 10.0 ** rng.uniform(-7, -4, n) * rng.choice([-1.0, 1.0], n)
    d = along + tilt[:, None] * nrm
    d /= np.linalg.norm(d, axis=1)[:, None]
    o = target - 50.0 * d
    return o.astype(np.float32), d.astype(np.float32)


def _demo(gpu, builder):
    from chroma_amd import demo
    from chroma_amd.loader import create_geometry_from_obj
    from chroma_amd.gpu.geometry import pack_geometry
    geometry = create_geometry_from_obj(getattr(demo, builder)())
    packed = pack_geometry(geometry)
    return geometry, packed, gpu.GPUDetector(geometry, packed=packed)


@pytest.mark.parametrize('builder', ['tiny', 'scintillator_stress'])
def test_isect_records_and_hits(gpu, oracle_mod, builder):
    geometry, packed, gg = _demo(gpu, builder)
    check_isect_records(gg, packed)
    rng = np.random.default_rng(11)
    lo = np.array([gg.world_origin[k] for k in ('x', 'y', 'z')], np.float64)
    o, d = random_rays(rng, 40000, lo, lo + 65535.0 * float(gg.world_scale))
    check_hits_are_the_vertex_form(gpu, gg, packed, o, d, oracle_mod, min_hits=0.05)
    o, d = grazing_rays(rng, packed, 40000)
    r = check_hits_are_the_vertex_form(gpu, gg, packed, o, d, oracle_mod)
    assert (r['literal'][0] >= 0).mean() > 0.1
    del gg, packed, geometry
    gc.collect()


@pytest.mark.timeout(3000)
def test_isect_records_and_aimed_rays_of_c3(gpu, oracle_mod):
    geometry, packed, gg = _demo(gpu, 'detector29k')
    check_isect_records(gg, packed)
    # tests/test_gpu_configs.py::test_c3_aimed_ray_sweep_the_deviation_class_is_a_checked_invariant's rays
    v, t = geometry.mesh.vertices.astype(np.float64), geometry.mesh.triangles
    rng = np.random.default_rng(3)
    for _ in range(2):
        rng.choice(len(t), size=60000, replace=False)
    pick = rng.choice(len(t), size=60000, replace=False)
    origin = np.array([0.0, 0.0, 1200.0])
    tri = v[t[pick]]
    targets = np.concatenate([tri.reshape(-1, 3), 0.5 * (tri[:, 0] + tri[:, 1]), 0.5 * (tri[:, 1] + tri[:, 2]), tri.mean(axis=1)])
    d = targets - origin
    d = d[np.linalg.norm(d, axis=1) > 1e-9]
    d /= np.linalg.norm(d, axis=1)[:, None]
    assert len(d) == 360000
    o32 = np.tile(origin.astype(np.float32), (len(d), 1))
    check_hits_are_the_vertex_form(gpu, gg, packed, o32, np.ascontiguousarray(d, dtype=np.float32), oracle_mod, min_hits=0.5)
    del gg, packed, geometry
    gc.collect()
