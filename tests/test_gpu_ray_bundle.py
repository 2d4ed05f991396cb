"""chroma_intersect_mesh / chroma_distance_to_mesh -- the ray-bundle cast -- against the CPU oracle at its sizes, its edge
rays and under every walk: the lane-per-ray k_distance_to_mesh (walks 'reference', 'exact', 'literal_lane') and the fast
path k_rays_from_arrays -> k_raycast_quad -> k_distance_finish -> k_distance_retry (every other walk).

Every expectation is oracle.distance_to_mesh's, compared bit for bit on every row.  One helper (`cast`) makes every call:
the outputs carry 64 guard elements past n, the distances start as a NaN that is not the default one and the triangles
as -2, so a kernel that writes past n, writes a distance on a miss, or leaves a triangle unwritten is seen.
"""
import re
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from conftest import make_stress_geometry
from test_gpu_parity import _aimed_photons, _host_walk, assert_bit_exact

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC0BEEF          # a quiet NaN with a payload: not what np.nan, 0.0f / 0.0f or a kernel's own NaN looks like
UNWRITTEN = -2                 # no triangle id and no HIT_* code the call may return
GUARD = 64
WALKS = ('reference', 'wide', 'coop', 'quad', 'pair', 'exact', 'literal_lane')
LANE_WALKS = ('reference', 'exact', 'literal_lane')          # (k_distance_to_mesh; plan.isect_quad false)
INT32_MAX, INT32_MIN = np.iinfo(np.int32).max, np.iinfo(np.int32).min


@pytest.fixture(scope='module')
def gpu():
    from chroma_amd import gpu as g
    ctx = g.create_cuda_context(0)
    yield g
    ctx.pop()


@pytest.fixture(scope='module')
def tiny_gg(gpu, tiny_geometry):
    return gpu.GPUDetector(tiny_geometry)


def oracle_cast(oracle_mod, packed, o, d, last=None):
    """(distance bits with SENTINEL on a miss, triangle) from oracle.distance_to_mesh, the rays dealt to a few threads."""
    o, d = np.ascontiguousarray(o, dtype=np.float32), np.ascontiguousarray(d, dtype=np.float32)
    n = len(o)
    if n == 0:
        return np.empty(0, np.uint32), np.empty(0, np.int32)
    cuts = np.linspace(0, n, min(8, 1 + n // 20000) + 1).astype(int)
    oracle_mod.distance_to_mesh(packed, o[:1], d[:1])                      # (binds the entry point before the threads use it)

    def part(k):
        a, b = cuts[k], cuts[k + 1]
        return oracle_mod.distance_to_mesh(packed, o[a:b], d[a:b], last_hits=None if last is None else last[a:b])[:2]
    with ThreadPoolExecutor(len(cuts) - 1) as pool:
        parts = list(pool.map(part, range(len(cuts) - 1)))
    wd = np.concatenate([p[0] for p in parts])
    wt = np.concatenate([p[1] for p in parts])
    return np.where(wt >= 0, wd.view(np.uint32), np.uint32(SENTINEL)), wt


class Rays(object):
    """A bundle on the device (uploaded once; a call may cast any prefix of it)."""

    def __init__(self, ctx, o, d, last=None):
        from chroma_amd.gpu.tools import to_gpu
        self.o, self.d = np.ascontiguousarray(o, dtype=np.float32), np.ascontiguousarray(d, dtype=np.float32)
        self.last = None if last is None else np.ascontiguousarray(last, dtype=np.int32)
        self.n = len(self.o)
        self.d_o, self.d_d = to_gpu(self.o.reshape(-1), ctx), to_gpu(self.d.reshape(-1), ctx)
        self.d_last = None if last is None else to_gpu(self.last, ctx)


def cast(ctx, gg, rays, n=None, walk='quad', use_last=True, triangles=True, counting=False):
    """One chroma_intersect_mesh call over the first n rays, under `walk`, on guarded and poisoned outputs; the context's
    walk and counting are put back whatever happens.  Returns (distance bits, triangles or None)."""
    from chroma_amd import _lib
    from chroma_amd.gpu.tools import GPUArray
    n = rays.n if n is None else n
    dist = GPUArray(n + GUARD, np.uint32, ctx).fill(np.uint32(SENTINEL))
    tri = GPUArray(n + GUARD, np.int32, ctx).fill(np.int32(UNWRITTEN))
    last = rays.d_last if use_last else None
    ctx.set_walk(walk)
    try:
        ctx.set_counting(counting)
        if counting:
            ctx.read_stats()                                   # (reading starts the counters again at zero)
        _lib.check(ctx._lib.chroma_intersect_mesh(ctx.handle, gg.handle, n, rays.d_o.ptr, rays.d_d.ptr,
                                                  None if last is None else last.ptr, dist.ptr, tri.ptr if triangles else None))
        if counting:
            stats = ctx.read_stats()
            assert stats['stack_overflows'] == 0, stats
    finally:
        ctx.set_walk('quad')
        ctx.set_counting(False)
    gd, gt = dist.get(), tri.get()
    assert (gd[n:] == SENTINEL).all(), '%s walk, %d rays: distances written past n' % (walk, n)
    assert (gt[n:] == UNWRITTEN).all(), '%s walk, %d rays: triangles written past n' % (walk, n)
    if not triangles:
        assert (gt == UNWRITTEN).all()
        return gd[:n], None
    return gd[:n], gt[:n]


def same(got, want, what):
    """Every row, bit for bit: `want` is (distance bits, triangles) of the oracle, `got` what cast() returned."""
    (gd, gt), (wd, wt) = got, want
    n = len(gd)
    bad = gd != wd[:n]
    assert not bad.any(), '%s: distance of %d of %d rays differs, first %d: %08x, oracle %08x' % (
        what, bad.sum(), n, np.flatnonzero(bad)[0], gd[bad][0], wd[:n][bad][0])
    if gt is not None:
        bad = gt != wt[:n]
        assert not bad.any(), '%s: triangle of %d of %d rays differs, first %d: %d, oracle %d' % (
            what, bad.sum(), n, np.flatnonzero(bad)[0], gt[bad][0], wt[:n][bad][0])


def every_form(ctx, gg, rays, n, walk, plain, excluded, what):
    """The call in all its forms over the first n rays: with and without the last-hit array, with d_triangle and with
    NULL, counting off and on.  `plain` / `excluded`: the oracle's rows without / with the last hits."""
    for use_last, want in ((False, plain), (True, excluded)):
        if want is None:
            continue
        for triangles in (True, False):
            for counting in (False, True):
                form = '%s, %s walk, %d rays%s%s%s' % (what, walk, n, ', last hits' if use_last else '',
                                                       '' if triangles else ', no triangle array', ', counting' if counting else '')
                same(cast(ctx, gg, rays, n, walk, use_last, triangles, counting), want, form)


def inside_rays(rng, n):
    """Random origins inside demo.tiny()'s sphere of PMTs, random directions."""
    return rng.uniform(-1500, 1500, (n, 3)).astype(np.float32), rng.normal(size=(n, 3)).astype(np.float32)


# ---- a. sizes x walks ---------------------------------------------------------------------------------------------
def bundle_sizes(ctx):
    """The 16-lane groups, the waves and the 256-thread blocks; then where a launch of k_raycast_quad fills its grid (R rays
    per wave, W waves: cast_waves) and where its waves begin to claim big chunks of B rays (ray_chunk: n > 4 B W), as the
    host resolves R, W and B for this device; and a size above W B, a grid of big chunks."""
    R, W, B = _host_walk('quad', int(re.search(r'(\d+) CUs\)', ctx.device_name()).group(1)))
    return [1, 15, 16, 17, 63, 64, 65, 255, 256, 257, R * W - 1, R * W, R * W + 1, R * W + R, 2 * R * W + 5, B * W + 77,
            4 * B * W, 4 * B * W + 1]


@pytest.fixture(scope='module')
def pool(gpu, oracle_mod, tiny_packed):
    """One pool of rays for every size (a bundle of n rays is its first n), on the device once, with the oracle's rows for
    it: plain, and with a last-hit array that holds the plain winner for every third ray, another triangle for the next
    and -1 for the rest."""
    ctx = gpu.get_context()
    nmax = max(bundle_sizes(ctx))
    rng = np.random.default_rng(2718)
    o, d = inside_rays(rng, nmax)
    plain = oracle_cast(oracle_mod, tiny_packed, o, d)
    k = np.arange(nmax) % 3
    last = np.where(k == 0, plain[1], np.where(k == 1, rng.integers(0, tiny_packed.desc.ntriangles, nmax), -1)).astype(np.int32)
    excluded = oracle_cast(oracle_mod, tiny_packed, o, d, last)
    return Rays(ctx, o, d, last), plain, excluded


def test_pool_is_not_vacuous(pool):
    """By the oracle alone: the pool's rays hit, and its last-hit array changes what they hit."""
    rays, plain, excluded = pool
    share = (plain[1] >= 0).mean()
    print('share of the pool\'s rays that hit: %.4f' % share)
    assert share >= 0.9
    assert (excluded[1][::3] != plain[1][::3])[plain[1][::3] >= 0].all()            # an excluded winner never wins
    assert (excluded[1][::3] >= 0).mean() > 0.05                                      # ... and some such rays go on to another triangle


@pytest.mark.parametrize('walk', WALKS)
def test_every_size_under_every_walk(gpu, tiny_gg, pool, walk):
    """Every size of bundle_sizes(), every form of the call, under every walk name the context accepts."""
    ctx = gpu.get_context()
    rays, plain, excluded = pool
    for n in bundle_sizes(ctx):
        every_form(ctx, tiny_gg, rays, n, walk, plain, excluded, 'tiny')


# ---- b. last-hit ids ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('walk', ('quad',) + LANE_WALKS)
def test_last_hit_ids_inside_and_outside_the_mesh(gpu, oracle_mod, tiny_gg, tiny_packed, walk):
    """Seven kinds of last-hit id dealt over the lanes (7 and 64 share no factor: every kind meets every lane of a wave
    within seven waves).  An id outside [0, ntriangles) excludes nothing under every walk (include/chroma_hip.h)."""
    ctx = gpu.get_context()
    ntri = int(tiny_packed.desc.ntriangles)
    n = 4 * 7 * 64 + 29
    rng = np.random.default_rng(31)
    o, d = inside_rays(rng, n)
    plain = oracle_cast(oracle_mod, tiny_packed, o, d)
    same(cast(ctx, tiny_gg, Rays(ctx, o, d), walk=walk, use_last=False), plain, 'no last hits, %s walk' % walk)
    kind = np.arange(n) % 7
    other = (np.maximum(plain[1], 0) + 1 + rng.integers(0, ntri - 1, n)) % ntri          # a valid id that is not the winner
    ids = np.select([kind == 0, kind == 1, kind == 2, kind == 3, kind == 4, kind == 5],
                    [plain[1], -1, other, ntri, INT32_MAX, -7], INT32_MIN).astype(np.int32)
    want = oracle_cast(oracle_mod, tiny_packed, o, d, ids)
    got = cast(ctx, tiny_gg, Rays(ctx, o, d, ids), walk=walk)
    same(got, want, 'mixed last hits, %s walk' % walk)
    # the exclusion matters: a ray whose winner is excluded goes on to another triangle, or to none
    had = (kind == 0) & (plain[1] >= 0)
    assert had.sum() > 200 and (got[1][had] != plain[1][had]).all() and (got[1][had] >= 0).sum() >= 10
    # ... and an id that names no triangle of the mesh changes nothing
    outside = (kind == 1) | (kind >= 3)
    assert np.array_equal(got[1][outside], plain[1][outside]) and np.array_equal(got[0][outside], plain[0][outside])
    assert (got[1][outside] >= 0).sum() > 1000


# ---- c. edge rays ---------------------------------------------------------------------------------------------------
def edge_kinds(geometry, packed):
    """name -> a function of a numpy generator giving one ray of the kind (origin, direction, last hit)."""
    v = geometry.mesh.vertices.astype(np.float32)
    t = geometry.mesh.triangles
    wo = np.array([packed.desc.world_origin[k] for k in range(3)], dtype=np.float32)
    ws = np.float32(packed.desc.world_scale)

    def inside(rng):
        return rng.uniform(-1200, 1200, 3).astype(np.float32)

    def anywhere(rng):
        return rng.normal(size=3).astype(np.float32)

    def unit(rng):
        u = rng.normal(size=3)
        return u / np.linalg.norm(u)

    def corner(rng, last):
        k = int(rng.integers(0, len(t)))
        return v[t[k, int(rng.integers(0, 3))]], anywhere(rng), k if last else -1

    def centroid(rng, last):
        k = int(rng.integers(0, len(t)))
        return (v[t[k]].astype(np.float64).mean(axis=0)).astype(np.float32), anywhere(rng), k if last else -1

    def box_plane(rng):
        o = inside(rng)
        axis = int(rng.integers(0, 3))
        o[axis] = wo[axis] + np.float32(np.round((o[axis] - wo[axis]) / ws)) * ws
        return o, anywhere(rng), -1

    def in_plane(rng):
        a, b, c = v[t[int(rng.integers(0, len(t)))]].astype(np.float64)
        along = (b - a) / np.linalg.norm(b - a)
        return ((a + b + c) / 3 - 50.0 * along).astype(np.float32), along.astype(np.float32), -1

    def far_back(rng):
        u = unit(rng)
        return (1e7 * u).astype(np.float32), (-u).astype(np.float32), -1

    kinds = {
        'zero direction': lambda rng: (inside(rng), np.zeros(3, np.float32), -1),
        'NaN direction': lambda rng: (inside(rng), np.array([np.nan, 0.6, 0.8], np.float32), -1),
        'NaN origin': lambda rng: (np.array([100.0, np.nan, -50.0], np.float32), anywhere(rng), -1),
        'infinite direction': lambda rng: (inside(rng), np.array([0.5, np.inf, 0.5], np.float32), -1),
        'component 1e-38': lambda rng: (inside(rng), np.array([1e-38, 1.0, 1e-38], np.float32), -1),
        'component 1e-20': lambda rng: (inside(rng), np.array([0.6, 1e-20, -0.8], np.float32), -1),
        'origin 1e30': lambda rng: (np.array([40.0, 1e30, 7.0], np.float32), anywhere(rng), -1),
        'origin 3e38': lambda rng: (np.full(3, 3e38, np.float32), anywhere(rng), -1),
        'origin 1e7, aimed back': far_back,
        'on a vertex': lambda rng: corner(rng, False),
        'on a vertex, last hit': lambda rng: corner(rng, True),
        'on a centroid': lambda rng: centroid(rng, False),
        'on a centroid, last hit': lambda rng: centroid(rng, True),
        'on a box plane': box_plane,
        'in a triangle\'s plane': in_plane,
    }
    for name, axis in (('+x', (1, 0, 0)), ('-x', (-1, 0, 0)), ('+y', (0, 1, 0)), ('-y', (0, -1, 0)), ('+z', (0, 0, 1)), ('-z', (0, 0, -1))):
        kinds['axis ' + name] = lambda rng, axis=axis: (inside(rng), np.array(axis, np.float32), -1)
    return kinds


# of these, the rays k_rays_from_arrays does not find "moderate" (a NaN, |1/d| >= 1e30 or |o/d| >= 1e30): the literal walk's
NOT_MODERATE = ('zero direction', 'NaN direction', 'NaN origin', 'infinite direction', 'component 1e-38', 'origin 1e30',
                'origin 3e38', 'axis +x', 'axis -x', 'axis +y', 'axis -y', 'axis +z', 'axis -z')

# how many of a kind's five rays in edge_bundle() hit, by the oracle (recorded from it; asserted below)
EDGE_HITS = {'zero direction': 0, 'NaN direction': 0, 'NaN origin': 0, 'infinite direction': 0, 'component 1e-38': 0,
             'component 1e-20': 5, 'origin 1e30': 0, 'origin 3e38': 0, 'origin 1e7, aimed back': 5, 'on a vertex': 3,
             'on a vertex, last hit': 5, 'on a centroid': 5, 'on a centroid, last hit': 5, 'on a box plane': 5,
             'in a triangle\'s plane': 5, 'axis +x': 5, 'axis -x': 5, 'axis +y': 5, 'axis -y': 5, 'axis +z': 5, 'axis -z': 5}


def moderate(o, d):
    """k_rays_from_arrays' test in float32."""
    o, d = o.astype(np.float32), d.astype(np.float32)
    with np.errstate(all='ignore'):
        norm = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        d = d / norm[:, None]
        noid, inv = (-o) / d, np.float32(1.0) / d
        return (np.abs(inv) < np.float32(1e30)).all(axis=1) & (np.abs(noid) < np.float32(1e30)).all(axis=1)


def edge_bundle(geometry, packed):
    """Ordinary rays with five of every kind among them.  Kind k has wave k of the bundle: its rays sit in the wave's first
    and last lane and on both sides of one of its 16-lane boundaries, and in lane 37, which is the last slot of the bundle
    of 64 k + 38 rays.  Returns (origins, directions, last hits, {kind: its slots})."""
    kinds = edge_kinds(geometry, packed)
    rng = np.random.default_rng(1618)
    n = 64 * len(kinds) + 1
    o, d = inside_rays(rng, n)
    last = np.full(n, -1, np.int32)
    where = {}
    for k, (name, make) in enumerate(kinds.items()):
        edge = 16 * (1 + k % 3)
        where[name] = [64 * k + lane for lane in (0, edge - 1, edge, 37, 63)]
        for slot in where[name]:
            o[slot], d[slot], last[slot] = make(rng)
    name = 'on a centroid'                                    # (the kind of the bundle's own last slot)
    o[n - 1], d[n - 1], last[n - 1] = kinds[name](rng)
    return o, d, last, where


def test_edge_rays(gpu, oracle_mod, tiny_geometry, tiny_gg, tiny_packed):
    """The rays of edge_kinds() among ordinary ones, each kind in the last slot of a bundle, a wave of nothing else, and a
    bundle that goes to the literal walk whole: the fast path and the lane kernel give the oracle's rows."""
    ctx = gpu.get_context()
    o, d, last, where = edge_bundle(tiny_geometry, tiny_packed)
    n = len(o)
    want = oracle_cast(oracle_mod, tiny_packed, o, d, last)
    hits = {name: int((want[1][slots] >= 0).sum()) for name, slots in where.items()}
    print('edge rays that hit, of five of a kind:', hits)
    assert hits == EDGE_HITS
    special = np.concatenate(list(where.values()))
    assert not moderate(o[np.concatenate([where[k] for k in NOT_MODERATE])], d[np.concatenate([where[k] for k in NOT_MODERATE])]).any()
    assert moderate(o[where['component 1e-20']], d[where['component 1e-20']]).all()
    rays = Rays(ctx, o, d, last)
    for walk in ('quad',) + LANE_WALKS:
        every_form(ctx, tiny_gg, rays, n, walk, None, want, 'edge rays')
        for k in range(len(where)):                          # each kind in the last slot of a bundle
            same(cast(ctx, tiny_gg, rays, 64 * k + 38, walk), want, 'edge rays, %s walk, %d rays' % (walk, 64 * k + 38))
    # a wave of such rays only; a bundle no ray of which is moderate (the retry list holds n)
    for what, pick, count in (('64 edge rays', special, 64), ('300 rays that are not moderate', np.concatenate([where[k] for k in NOT_MODERATE]), 300)):
        pick = np.resize(pick, count)
        if count == 300:
            assert not moderate(o[pick], d[pick]).any()
        for walk in ('quad',) + LANE_WALKS:
            every_form(ctx, tiny_gg, Rays(ctx, o[pick], d[pick], last[pick]), count, walk, None, (want[0][pick], want[1][pick]), what)


def test_a_bundle_in_which_every_ray_misses(gpu, oracle_mod, tiny_gg, tiny_packed):
    """257 rays from outside the detector pointing away: every distance keeps its sentinel, every triangle is -1."""
    ctx = gpu.get_context()
    rng = np.random.default_rng(57)
    u = rng.normal(size=(257, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    o, d = (4000.0 * u).astype(np.float32), u.astype(np.float32)
    want = oracle_cast(oracle_mod, tiny_packed, o, d)
    assert (want[1] == -1).all() and (want[0] == SENTINEL).all()
    rays = Rays(ctx, o, d, np.full(257, 5, np.int32))
    for walk in WALKS:
        every_form(ctx, tiny_gg, rays, 257, walk, want, want, 'rays that all miss')


# ---- d. ties at small sizes -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [257, 4097])
def test_ties_at_small_sizes(gpu, oracle_mod, tiny_geometry, tiny_gg, tiny_packed, n):
    """Rays through vertices, edge midpoints and centroids: several triangles at one distance, and the winners that
    k_distance_finish hands to k_distance_retry.  Plain, then with the first winner excluded."""
    ctx = gpu.get_context()
    ph = _aimed_photons(tiny_geometry, (0.0, 0.0, 0.0), n)
    pick = (np.arange(n) * (len(ph) // n))                    # (vertices, edge midpoints and centroids alike)
    o, d = ph.pos[pick].astype(np.float32), ph.dir[pick].astype(np.float32)
    plain = oracle_cast(oracle_mod, tiny_packed, o, d)
    excluded = oracle_cast(oracle_mod, tiny_packed, o, d, plain[1])
    tie = (plain[1] >= 0) & (excluded[1] >= 0) & (excluded[1] != plain[1]) & (excluded[0] == plain[0])
    print('%d of %d aimed rays find another triangle at the same distance bits' % (tie.sum(), n))
    assert tie.sum() >= n // 20
    rays = Rays(ctx, o, d, plain[1])
    for walk in ('quad', 'exact'):
        every_form(ctx, tiny_gg, rays, n, walk, plain, excluded, 'aimed rays')


# ---- e. other geometries -----------------------------------------------------------------------------------------------
def _few_triangles(ntri):
    from chroma_amd.geometry import Geometry, Solid, Mesh, vacuum
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [5, 5, 5], [6, 5, 5], [5, 6, 5]], dtype=np.float32)
    g = Geometry()
    g.add_solid(Solid(Mesh(v[:3 * ntri], np.arange(3 * ntri, dtype=np.int32).reshape(-1, 3)), vacuum, vacuum))
    return g


def _other_geometry(which):
    """(geometry, origins, directions) for 4097 rays."""
    from chroma_amd.loader import create_geometry_from_obj
    rng = np.random.default_rng(77)
    n = 4097
    if which in ('one triangle', 'two triangles'):
        geometry = create_geometry_from_obj(_few_triangles(1 if which == 'one triangle' else 2))
        tri = geometry.mesh.vertices[geometry.mesh.triangles[rng.integers(0, len(geometry.mesh.triangles), n)]].astype(np.float64)
        w = rng.dirichlet([1.0, 1.0, 1.0], n) * 1.6 - 0.2                       # points in and a little around the triangles
        o = rng.uniform(-3, 9, (n, 3))
        d = (w[:, :, None] * tri).sum(axis=1) - o
        return geometry, o.astype(np.float32), d.astype(np.float32)
    if which == 'stress':
        geometry = make_stress_geometry()
        return geometry, rng.uniform(-150, 150, (n, 3)).astype(np.float32), rng.normal(size=(n, 3)).astype(np.float32)
    from test_gpu_fuzz import _geometries
    geometry = create_geometry_from_obj(dict(_geometries())[which])
    o = rng.uniform(-400, 400, (n, 3)).astype(np.float32)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    d[:400] = np.round(d[:400])                                                  # exactly axis-parallel and diagonal rays
    d[np.abs(d).sum(axis=1) == 0] = [0, 0, 1]
    o[400:800] = np.round(o[400:800] / 250.0) * 250.0                            # origins ON the shared face planes
    return geometry, o, d


@pytest.mark.parametrize('which', ['one triangle', 'two triangles', 'stress', 'soup1', 'soup2', 'soup3', 'twins', 'nested'])
def test_other_geometries(gpu, oracle_mod, which):
    """Meshes of one and of two triangles, the stress cube, and the soups, twin spheres and nested boxes of
    tests/test_gpu_fuzz.py, plain and with every winner excluded.  (The default walk casts all of them with k_raycast_quad:
    none is too deep for its stack, so no case here reaches the lane kernel under the default walk.)"""
    from chroma_amd.gpu.geometry import pack_geometry
    ctx = gpu.get_context()
    geometry, o, d = _other_geometry(which)
    packed = pack_geometry(geometry)
    gg = gpu.GPUDetector(geometry) if hasattr(geometry, 'num_channels') else gpu.GPUGeometry(geometry)
    plain = oracle_cast(oracle_mod, packed, o, d)
    excluded = oracle_cast(oracle_mod, packed, o, d, plain[1])
    hit = plain[1] >= 0
    print('%s: %d of %d rays hit, %d of them again with the winner excluded' % (which, hit.sum(), len(o), (excluded[1][hit] >= 0).sum()))
    if which == 'one triangle':
        # (mesh.h:42-118 tests the CHILDREN of the root: a tree that is one leaf has none, and no ray hits its triangle)
        assert len(geometry.bvh.nodes) == 1 and not hit.any()
    else:
        assert hit[:257].sum() >= 90
    rays = Rays(ctx, o, d, plain[1])
    for n in (257, 4097):
        for walk in ('quad', 'reference'):
            every_form(ctx, gg, rays, n, walk, plain, excluded, which)


# ---- f. one context, many calls ---------------------------------------------------------------------------------------
def test_one_context_many_calls(gpu, oracle_mod, tiny_geometry, tiny_packed):
    """The cast shares the context's queues, ray records, hit entries, retry list and step block with propagate calls:
    on a context of its own, bundles of 64, 5000 and 64 rays (the queues grow for the second), then a propagate, a cast and
    the propagate's next steps, each against the oracle."""
    g = gpu
    module_ctx = g.get_context()
    ctx = g.create_cuda_context(0)
    try:
        gg = g.GPUDetector(tiny_geometry)
        rng = np.random.default_rng(99)
        o, d = inside_rays(rng, 5000)
        o[7], d[7] = 0.0, (0.0, 0.0, 1.0)                      # (one ray for k_distance_retry in every bundle)
        plain = oracle_cast(oracle_mod, tiny_packed, o, d)
        last = np.where(np.arange(5000) % 2 == 0, plain[1], -1).astype(np.int32)
        excluded = oracle_cast(oracle_mod, tiny_packed, o, d, last)
        rays = Rays(ctx, o, d, last)
        for n in (64, 5000, 64):
            same(cast(ctx, gg, rays, n), excluded, 'fresh context, %d rays' % n)
        ph = oracle_mod.generate_bomb(20000, seed=8)
        gp = g.GPUPhotons(ph)
        rng_states = g.get_rng_states(64, seed=33)
        gp.propagate(gg, rng_states, max_steps=2)
        want, counters, _ = oracle_mod.propagate(tiny_packed, ph, seed=33, max_steps=2, nthreads=8)
        same(cast(ctx, gg, rays, 5000, use_last=False), plain, 'after a propagate call')
        assert_bit_exact(gp.get(), want, 'propagate before the cast')
        gp.propagate(gg, rng_states, max_steps=3)
        want, counters, _ = oracle_mod.propagate(tiny_packed, want, seed=33, max_steps=3, nthreads=8, rng_counters=counters)
        assert_bit_exact(gp.get(), want, 'propagate after the cast')
        assert np.array_equal(gp.rng_counters.get(), counters)
        same(cast(ctx, gg, rays, 4097, walk='reference'), excluded, 'after the second propagate call')
    finally:
        ctx.pop()
        module_ctx.push()                                      # (the module's geometry and pool live on this one)


def test_empty_bundles_and_null_arrays(gpu, tiny_gg):
    """n == 0 and n < 0 are no work and no error; a null origin, direction or distance is refused before any launch."""
    from chroma_amd.gpu.tools import GPUArray
    ctx = gpu.get_context()
    lib = ctx._lib
    rays = Rays(ctx, *inside_rays(np.random.default_rng(3), 64), last=np.full(64, -1, np.int32))
    dist = GPUArray(64, np.uint32, ctx).fill(np.uint32(SENTINEL))
    tri = GPUArray(64, np.int32, ctx).fill(np.int32(UNWRITTEN))
    for n in (0, -1, INT32_MIN):
        assert lib.chroma_intersect_mesh(ctx.handle, tiny_gg.handle, n, rays.d_o.ptr, rays.d_d.ptr, rays.d_last.ptr, dist.ptr, tri.ptr) == 0
        assert lib.chroma_distance_to_mesh(ctx.handle, tiny_gg.handle, n, rays.d_o.ptr, rays.d_d.ptr, dist.ptr, tri.ptr) == 0
    for o, d, out in ((None, rays.d_d.ptr, dist.ptr), (rays.d_o.ptr, None, dist.ptr), (rays.d_o.ptr, rays.d_d.ptr, None)):
        assert lib.chroma_intersect_mesh(ctx.handle, tiny_gg.handle, 64, o, d, rays.d_last.ptr, out, tri.ptr) != 0
        assert b'bad argument' in lib.chroma_last_error()
        assert lib.chroma_distance_to_mesh(ctx.handle, tiny_gg.handle, 64, o, d, out, tri.ptr) != 0
    assert lib.chroma_intersect_mesh(None, tiny_gg.handle, 64, rays.d_o.ptr, rays.d_d.ptr, None, dist.ptr, tri.ptr) != 0
    assert lib.chroma_intersect_mesh(ctx.handle, None, 64, rays.d_o.ptr, rays.d_d.ptr, None, dist.ptr, tri.ptr) != 0
    ctx.synchronize()
    assert (dist.get() == SENTINEL).all() and (tri.get() == UNWRITTEN).all()


# ---- g. the Python shape ------------------------------------------------------------------------------------------------
def test_the_kernel_by_name(gpu, tiny_gg, pool):
    """mesh.h's distance_to_mesh looked up by name and called with the reference kernel's arguments: the rows of the same
    257 rays under the default walk."""
    from chroma_amd.gpu import get_cu_module, GPUFuncs
    from chroma_amd.gpu.tools import GPUArray
    ctx = gpu.get_context()
    rays, plain, _ = pool
    n = 257
    dist = GPUArray(n + GUARD, np.uint32, ctx).fill(np.uint32(SENTINEL))
    GPUFuncs(get_cu_module('mesh.h')).distance_to_mesh(np.int32(n), rays.d_o, rays.d_d, tiny_gg.gpudata, dist, block=(64, 1, 1), grid=(n // 64 + 1, 1))
    gd = dist.get()
    assert (gd[n:] == SENTINEL).all()
    same((gd[:n], None), plain, 'distance_to_mesh by name')
    same(cast(ctx, tiny_gg, rays, n, use_last=False, triangles=False), (gd[:n], None), 'the C call on the same rays')
