"""k_render and k_color_solids (chroma_render / chroma_color_solids; chroma/cuda/render.cu:37-181, sorting.h:64-98,
mesh.h:153-166) at their ties, edges and sizes: synthetic bundles through the C entry point, every ray's pixel, list length
and list entries bit for bit against oracle.render (and the oracle against the reference's own kernel compiled for gfx950
where oracle/_ref holds it).  Every call runs on arrays that are 64 rows longer than the bundle: pixels, distances and
colours are filled with a sentinel before the call, the guard rows hold real rays, and afterwards the guard rows of all four
arrays must be as they were; so must the list rows of every ray that met nothing.

A chain of calls is a continued render (keep_last_render): the device continues its own arrays (sentinels in the slots
beyond a list's length), the oracle its own (zeros there).

The test without a `gpu` mark measures from the oracle's output alone that the bundles reach what they are meant to reach
(ties, full lists, misses, colours whose order shows in the pixels)."""
import copy
import os

import numpy as np
import pytest

from conftest import ROOT             # noqa: F401  (puts the repository on sys.path)
from test_gpu_render import REF_LIB, _lists_equal, _ref_render

gpu_test = pytest.mark.gpu

SENTINEL = 0xDEADBEEF           # as a float32 -6.26e18: no distance, no colour component
GUARD = 64                      # rows behind every bundle (one block of k_render)
GUARD_LEN = 7                   # dxlen of the guard rows
BG = 0x7F102030
STACK_LDS = 24                  # chroma_internal.h: the entries of a render stack held in LDS
SIZES = (1, 63, 64, 65, 127, 128, 129, 257)
INSIDE = (0.3, -0.5, 0.8)       # the guard rows' ray: from the origin of every scene here it meets triangles


class Call(object):
    def __init__(self, o, d, alpha_depth, bg=0):
        self.o = np.ascontiguousarray(o, np.float32)
        self.d = np.ascontiguousarray(d, np.float32)
        assert self.o.shape == self.d.shape and self.o.shape[1] == 3
        self.alpha_depth, self.bg = alpha_depth, bg


def _unit(rng, n):
    d = rng.normal(size=(n, 3))
    return (d / np.linalg.norm(d, axis=1)[:, None]).astype(np.float32)


def _axes():
    return np.concatenate([np.eye(3), -np.eye(3)]).astype(np.float32)


# ---- geometries (built once per module) -------------------------------------------------------------------------------
_scenes = {}


def _memo(fn):
    def get():
        if fn.__name__ not in _scenes:
            _scenes[fn.__name__] = fn()
        return _scenes[fn.__name__]
    return get


CUBE_COLORS = (0x40E02010, 0xA010D030, 0x002040F0)      # the two coincident cubes (alpha bytes 0x40, 0xA0), the opaque inner one


def _build_cubes(colors):
    from chroma_amd import make
    from chroma_amd.geometry import Geometry, Solid, vacuum
    from chroma_amd.loader import create_geometry_from_obj
    from chroma_amd.gpu.geometry import pack_geometry
    g = Geometry(vacuum)
    for size, color in zip((100.0, 100.0, 50.0), colors):
        g.add_solid(Solid(make.cube(size), vacuum, vacuum, color=color))
    g = create_geometry_from_obj(g)
    return g, pack_geometry(g)


@_memo
def cubes():
    """Two coincident cubes of side 100 and an opaque one of side 50, all centred at the origin: 48 triangles."""
    return _build_cubes(CUBE_COLORS)


@_memo
def cubes_swapped():
    return _build_cubes((CUBE_COLORS[1], CUBE_COLORS[0], CUBE_COLORS[2]))


@_memo
def shells():
    """Three concentric spheres, one solid each, one distinct colour per triangle (alpha bytes 0x20 .. 0xDF)."""
    from chroma_amd import make
    from chroma_amd.geometry import Geometry, Solid, vacuum
    from chroma_amd.loader import create_geometry_from_obj
    from chroma_amd.gpu.geometry import pack_geometry
    g = Geometry(vacuum)
    for radius in (20.0, 40.0, 60.0):
        g.add_solid(Solid(make.sphere(radius, 16), vacuum, vacuum))
    g = create_geometry_from_obj(g)
    nt = len(g.mesh.triangles)
    rng = np.random.default_rng(21)
    rgb = rng.choice(1 << 24, nt, replace=False).astype(np.uint32)
    g.colors = (rng.integers(0x20, 0xE0, nt).astype(np.uint32) << np.uint32(24)) | rgb
    assert len(np.unique(g.colors)) == nt
    return g, pack_geometry(g)


def _recoloured(geometry, colors):
    from chroma_amd.gpu.geometry import pack_geometry
    g = copy.copy(geometry)
    g.colors = np.ascontiguousarray(colors, np.uint32)
    return g, pack_geometry(g)


@_memo
def lite():
    """demo.detector_lite(): the project's geometry whose reference walk can need more than STACK_LDS stack entries (51 by the
    backward sweep of tests/test_gpu_wide.py; demo.tiny() and the stress geometry stay below)."""
    from chroma_amd import demo
    from chroma_amd.loader import create_geometry_from_obj
    from chroma_amd.gpu.geometry import pack_geometry
    g = create_geometry_from_obj(demo.detector_lite())
    return g, pack_geometry(g)


# Rays whose render stack goes past STACK_LDS on detector_lite: DEEP_TARGET is the centre of the box of the last inner node on
# the deepest chain of the sweep, DEEP_ORIGIN the origin of the deepest of 6000 random rays aimed at it.  Most rays of the
# geometry stay below 20 entries; of rays from DEEP_ORIGIN into the 40 mm cube around DEEP_TARGET about one in five passes 24.
DEEP_ORIGIN = (-405.20966, -3652.9907, 1104.7382)
DEEP_TARGET = (1781.17, -1823.09, 1738.86)


def walk_depth(geometry, o, d):
    """The most entries the render's stack holds for one ray (render.cu:88-120: every inner child whose box the ray meets is
    pushed, the last one popped first), by a plain walk in float64."""
    nodes = np.ascontiguousarray(geometry.bvh.nodes).view(np.uint32).reshape(-1, 4)
    wo = np.asarray(geometry.bvh.world_coords.world_origin, np.float64)
    ws = float(geometry.bvh.world_coords.world_scale)
    o, inv = np.asarray(o, np.float64), 1.0 / np.asarray(d, np.float64)
    stack, deepest = [int(nodes[0, 3])], 1
    while stack:
        w = stack.pop()
        kids = nodes[(w & 0x0FFFFFFF):(w & 0x0FFFFFFF) + (w >> 28)]
        t0 = (wo + (kids[:, :3] & 0xFFFF) * ws - o) * inv
        t1 = (wo + (kids[:, :3] >> 16) * ws - o) * inv
        hit = np.maximum(np.minimum(t0, t1).max(axis=1), 0.0) <= np.maximum(t0, t1).min(axis=1)
        stack += [int(x) for x in kids[hit & (kids[:, 3] >> 28 != 0), 3]]
        deepest = max(deepest, len(stack))
    return deepest


# ---- bundles: name -> (scene, chain of calls), every one from a fixed seed --------------------------------------------
def _zeros(n):
    return np.zeros((n, 3), np.float32)


def _signed_zero_axes():
    """(+-1, +-0, +-0) and its rotations: the six axis directions with every sign of the two zeros (24 rays; the first
    six rows are the plain axes)."""
    rows = [a for a in _axes()]
    for axis in range(3):
        for s in (1.0, -1.0):
            for z1 in (0.0, -0.0):
                for z2 in (0.0, -0.0):
                    v = [z1, z2]
                    v.insert(axis, s)
                    if not (z1 == 0.0 and z2 == 0.0 and not np.signbit(z1) and not np.signbit(z2)):
                        rows.append(v)
    return np.array(rows, np.float32)


def _plane_directions(rng, n):
    """One component exactly 0 (+0.0 and -0.0 in turn), the other two random."""
    d = _unit(rng, n)
    k = rng.integers(0, 3, n)
    d[np.arange(n), k] = np.where(np.arange(n) % 2 == 0, np.float32(0.0), np.float32(-0.0))
    return d


def _shell_origins(rng, n):
    """Points between the inner cube (half side 25) and the coincident ones (half side 50)."""
    o = rng.uniform(-45.0, 45.0, size=(4 * n, 3))
    return o[np.abs(o).max(axis=1) > 30.0][:n].astype(np.float32)


def _bundles():
    if 'bundles' in _scenes:
        return _scenes['bundles']
    b = {}
    for n in SIZES:
        b['size-%d' % n] = ('tiny', [Call(_zeros(n), _unit(np.random.default_rng(100 + n), n), 3)])
    rng = np.random.default_rng(1)
    d = _unit(rng, 1000) * (10.0 ** rng.uniform(-2.0, 2.0, size=(1000, 1))).astype(np.float32)
    for a in (1, 2, 3, 10):
        b['alpha-%d' % a] = ('tiny', [Call(_zeros(1000), d, a, BG)])
    b['axes-origin'] = ('tiny', [Call(_zeros(24), _signed_zero_axes(), 10, BG)])
    rng = np.random.default_rng(2)
    o = rng.uniform(-1200.0, 1200.0, size=(300, 3)).astype(np.float32)
    d = _axes()[rng.integers(0, 6, 300)]
    d[1::2] = np.where(d[1::2] == 0, np.float32(-0.0), d[1::2])
    b['axes-inside'] = ('tiny', [Call(o, d, 10, BG)])
    b['planes'] = ('tiny', [Call(_zeros(500), _plane_directions(np.random.default_rng(3), 500), 10, BG)])
    # ties, on the coincident cubes
    d = _unit(np.random.default_rng(4), 1000)
    b['ties-4'] = ('cubes', [Call(_zeros(1000), d, 4, BG)])
    b['ties-2'] = ('cubes', [Call(_zeros(1000), d, 2, BG)])
    b['ties-axes'] = ('cubes', [Call(_zeros(24), _signed_zero_axes(), 4, BG)])
    v = np.asarray(cubes()[0].mesh.vertices, np.float32)
    b['ties-vertices'] = ('cubes', [Call(_zeros(len(v)), v, 6, BG)])
    # (from the centre the opaque inner cube hides what lies behind it in the PIXEL; between the cubes it does not)
    rng = np.random.default_rng(5)
    so, sd = _shell_origins(rng, 1000), _unit(rng, 1000)
    for a in (4, 2, 1):
        b['shell-%d' % a] = ('cubes', [Call(so, sd, a, BG)])
    # continued renders
    d = _unit(np.random.default_rng(6), 1000)
    moved = _zeros(1000) + np.float32(3.0)
    b['continue-4'] = ('cubes', [Call(_zeros(1000), d, 4), Call(moved, d, 4)])
    b['continue-1'] = ('cubes', [Call(_zeros(1000), d, 1, BG), Call(moved, d, 1, BG)])
    b['continue-shell'] = ('cubes', [Call(so, sd, 4, BG), Call(so + np.float32(2.0) * sd, sd, 4, BG)])
    # half of the rays outside the world box pointing away, then all from the centre, then the same half outside again (a ray
    # that holds a list and misses the root box composites the list it has)
    out_o, out_d = _zeros(1000), d.copy()
    out_o[::2] = np.float32(1000.0) * d[::2]
    b['continue-outside'] = ('cubes', [Call(out_o, out_d, 4, BG), Call(_zeros(1000), d, 4, BG), Call(out_o, out_d, 4, BG)])
    o = np.tile(np.float32([0.0, -6000.0, 0.0]), (200, 1))
    b['outside'] = ('tiny', [Call(o, _unit(np.random.default_rng(7), 200), 3, BG)])
    rng = np.random.default_rng(8)
    b['colours'] = ('shells', [Call(np.tile(np.float32([5.0, -3.0, 8.0]), (1000, 1)), _unit(rng, 1000), 3, BG)])
    rng = np.random.default_rng(10)
    o = np.tile(np.float32(DEEP_ORIGIN), (257, 1))
    b['deep-stack'] = ('lite', [Call(o, np.float32(DEEP_TARGET) + rng.uniform(-20.0, 20.0, size=(257, 3)).astype(np.float32) - o, 10, BG)])
    _scenes['bundles'] = b
    return b


BUNDLE_NAMES = (['size-%d' % n for n in SIZES] + ['alpha-%d' % a for a in (1, 2, 3, 10)] +
                ['axes-origin', 'axes-inside', 'planes', 'ties-4', 'ties-2', 'ties-axes', 'ties-vertices', 'shell-4', 'shell-2',
                 'shell-1', 'continue-4', 'continue-1', 'continue-shell', 'continue-outside', 'outside', 'colours', 'deep-stack'])


def _oracle_chain(oracle_mod, packed, calls):
    """[(pixels, state)] of a chain on the oracle, each call continuing the one before."""
    out, state = [], None
    for c in calls:
        pixels, state = oracle_mod.render(packed, c.o, c.d, alpha_depth=c.alpha_depth, bg_color=c.bg, state=state)
        out.append((pixels, state))
    return out


def _want(oracle_mod, name, tiny_packed):
    """The oracle's results of a bundle, computed once."""
    key = 'want-' + name
    if key not in _scenes:
        scene, calls = _bundles()[name]
        packed = tiny_packed if scene == 'tiny' else globals()[scene]()[1]
        _scenes[key] = _oracle_chain(oracle_mod, packed, calls)
    return _scenes[key]


def _ties(state):
    """Per ray: does its list hold two equal distances?"""
    dx, dxlen, _ = state
    k = np.arange(1, dx.shape[1])[None, :] < dxlen[:, None]
    return ((dx[:, 1:] == dx[:, :-1]) & k).any(axis=1)


# ---- the test that needs no GPU: the bundles reach what they are meant to reach ---------------------------------------
def measure(oracle_mod, tiny_packed):
    """name -> figure: what the oracle gives for the bundles (printed by the test below, kept in profiles/r14)."""
    def res(name, call=-1):
        return _want(oracle_mod, name, tiny_packed)[call]

    def full(name, call=-1):
        return res(name, call)[1][1] == _bundles()[name][1][call].alpha_depth
    m = {}
    for name in BUNDLE_NAMES:
        for k in range(len(_bundles()[name][1])):
            pix, st = res(name, k)
            key = name if len(_bundles()[name][1]) == 1 else '%s call %d' % (name, k)
            m[key] = dict(rays=len(pix), miss=int((st[1] == 0).sum()), ties=int(_ties(st).sum()), full=int(full(name, k).sum()),
                          longest=int(st[1].max()), background=int((pix == _bundles()[name][1][k].bg).sum()))
    pix, st = res('axes-origin')
    m['axes-origin']['ties in the six plain axes'] = int(_ties(st)[:6].sum())
    m['axes-origin']['finite'] = bool(np.isfinite(st[0][np.arange(10)[None, :] < st[1][:, None]]).all())
    # with the colours of the two coincident solids exchanged: rays whose kept entries change, rays whose pixel changes
    swapped = cubes_swapped()[1]
    for name in ('ties-4', 'ties-2', 'ties-axes', 'ties-vertices', 'shell-4', 'shell-2', 'shell-1'):
        pix, st = res(name)
        pix2, st2 = _oracle_chain(oracle_mod, swapped, _bundles()[name][1])[-1]
        assert np.array_equal(st[1], st2[1]) and np.array_equal(st[0], st2[0]), name
        k = np.arange(st[0].shape[1])[None, :] < st[1][:, None]
        m[name]['entries change on swap'] = int(((st[2] != st2[2]).any(axis=2) & k).any(axis=1).sum())
        m[name]['pixel changes on swap'] = int((pix != pix2).sum())
    m['colours']['distinct pixels'] = len(np.unique(res('colours')[0]))
    return m


def test_the_bundles_reach_ties_full_lists_misses_and_colours(oracle_mod, tiny_packed):
    """Inequalities with room under the figures measured when this was written (profiles/r14/INDEX.md), so that a changed
    seed or demo geometry cannot empty a case without this failing."""
    assert list(_bundles()) == BUNDLE_NAMES
    m = measure(oracle_mod, tiny_packed)
    for key, figures in m.items():
        print('%-24s %s' % (key, figures))
    # tiny, from its centre
    a = m['axes-origin']
    assert a['miss'] == 0 and a['finite'] and a['ties in the six plain axes'] >= 1 and a['ties'] >= 4 and a['full'] >= 4
    assert m['planes']['ties'] >= 3 and m['planes']['full'] >= 1 and m['planes']['miss'] < 400
    assert m['axes-inside']['miss'] < 30
    assert m['alpha-1']['full'] == 1000 and m['alpha-2']['full'] >= 20 and m['alpha-3']['full'] >= 10
    assert 3 <= m['alpha-10']['longest'] < 10 and m['alpha-10']['miss'] < 850
    for n in SIZES:
        assert m['size-%d' % n]['miss'] < n
    o = m['outside']
    assert o['miss'] >= 100 and o['rays'] - o['miss'] >= 3 and o['background'] == o['miss'] and (BG >> 24) != 0
    # the coincident cubes
    for name in ('ties-4', 'ties-axes', 'ties-vertices', 'shell-4'):
        assert m[name]['ties'] == m[name]['rays'], name
    assert m['ties-4']['longest'] == 3
    assert m['ties-2']['full'] == 1000 and m['ties-2']['ties'] == 0            # the tie sits ON the cut: one of the pair is dropped
    assert m['ties-axes']['full'] == 24 and m['ties-vertices']['full'] == m['ties-vertices']['rays']
    assert m['shell-2']['full'] == 1000 and m['shell-1']['full'] == 1000 and m['shell-2']['ties'] > 400
    assert m['continue-4 call 0']['full'] == 0 and m['continue-4 call 1']['full'] == 1000 and m['continue-4 call 1']['ties'] == 1000
    assert m['continue-1 call 0']['full'] == 1000 and m['continue-shell call 1']['full'] > 500
    first, second, third = [_want(oracle_mod, 'continue-outside', tiny_packed)[k] for k in range(3)]
    assert (first[1][1][::2] == 0).all() and (first[0][::2] == BG).all() and (first[1][1][1::2] == 3).all()
    assert (second[1][1][::2] == 3).all() and (second[1][1][1::2] == 4).all()
    assert np.array_equal(third[1][1], second[1][1]) and (third[0][::2] != BG).all()       # a held list shows though the ray misses the root
    # order matters.  From the centre the opaque inner cube is in front, so the exchange shows in the entries the lists keep
    # (every random ray; an axis or vertex ray can fill its list with inner triangles alone), not in the pixel; between the
    # cubes it shows in the pixel of most rays
    for name in ('ties-4', 'ties-2'):
        assert m[name]['entries change on swap'] == 1000 and m[name]['pixel changes on swap'] == 0
    assert m['ties-axes']['entries change on swap'] >= 6 and m['ties-vertices']['entries change on swap'] >= 6
    for name in ('shell-4', 'shell-2', 'shell-1'):
        assert m[name]['pixel changes on swap'] > 500, name
    # one colour per triangle: many pixel values
    assert m['colours']['distinct pixels'] > 500 and m['colours']['full'] > 900
    assert len(np.unique(shells()[0].solid_id)) == 3 and len(shells()[0].mesh.triangles) > 255 + 257


def test_the_deep_stack_rays_walk_past_the_lds_half():
    """The 257 rays on detector_lite are there to take the render's stack through its scratch half: of the first 64, at
    least 4 [9 when this was written] hold more than STACK_LDS entries at some point of the walk."""
    call = _bundles()['deep-stack'][1][0]
    depths = np.array([walk_depth(lite()[0], call.o[i], call.d[i]) for i in range(64)])
    print('deep-stack: stack entries of the first 64 rays: max %d, %d rays above %d' % (depths.max(), (depths > STACK_LDS).sum(), STACK_LDS))
    assert (depths > STACK_LDS).sum() >= 4 and depths.max() >= STACK_LDS + 3


# ---- the device side ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def ctx():
    from chroma_amd import gpu as g
    c = g.create_cuda_context(0)
    yield c
    c.pop()


@pytest.fixture(scope='module')
def device_scenes(ctx, tiny_geometry, tiny_packed):
    """name -> (geometry, packed, GPUGeometry), uploaded on first use."""
    from chroma_amd import gpu
    made = {}

    def get(name):
        if name not in made:
            g, packed = (tiny_geometry, tiny_packed) if name == 'tiny' else globals()[name]()
            made[name] = (g, packed, gpu.GPUGeometry(g, packed=packed))
        return made[name]
    yield get
    made.clear()


class DeviceRays(object):
    """The arrays of chroma_render for n rays and GUARD rows more: pixels, dx and
    colour all sentinel, dxlen 0 for the bundle and GUARD_LEN behind it, a ray that meets the scene in every guard row."""

    def __init__(self, ctx, n, alpha_depth):
        from chroma_amd.gpu.tools import GPUArray
        self.ctx, self.n, self.alpha_depth, rows = ctx, n, alpha_depth, n + GUARD
        self.pos = GPUArray(rows * 3, np.float32, ctx)
        self.dir = GPUArray(rows * 3, np.float32, ctx)
        self.pixels = GPUArray(rows, np.uint32, ctx).fill(SENTINEL)
        self.dx = GPUArray(rows * alpha_depth, np.uint32, ctx).fill(SENTINEL)
        self.color = GPUArray(rows * alpha_depth * 4, np.uint32, ctx).fill(SENTINEL)
        self.dxlen = GPUArray(rows, np.uint32, ctx).set(np.r_[np.zeros(n, np.uint32), np.full(GUARD, GUARD_LEN, np.uint32)])

    def host(self):
        rows, a = self.n + GUARD, self.alpha_depth
        return (self.pixels.get(), self.dx.get().reshape(rows, a), self.dxlen.get(), self.color.get().reshape(rows, a, 4))

    def render(self, gg, call, nthreads=None):
        """One chroma_render over the first n rows (pixels refilled with the sentinel first).  Returns the four arrays
        before and after, whole."""
        from chroma_amd import _lib
        n = self.n
        assert call.alpha_depth == self.alpha_depth and len(call.o) == n
        self.pos.set(np.concatenate([call.o, np.zeros((GUARD, 3), np.float32)]).reshape(-1))
        self.dir.set(np.concatenate([call.d, np.tile(np.float32(INSIDE), (GUARD, 1))]).reshape(-1))
        self.pixels.fill(SENTINEL)
        before = self.host()
        _lib.check(self.ctx._lib.chroma_render(self.ctx.handle, gg.gpudata, n if nthreads is None else nthreads, self.pos.ptr, self.dir.ptr,
                                               call.alpha_depth, self.pixels.ptr, self.dx.ptr, self.dxlen.ptr, self.color.ptr,
                                               call.bg & 0xFFFFFFFF))
        return before, self.host()


def _check_call(before, after, n, want, wstate, bg, what):
    """Everything one call must have done to the four arrays, and nothing else."""
    names = ('pixels', 'dx', 'dxlen', 'color')
    for name, b, a in zip(names, before, after):
        assert np.array_equal(a[n:], b[n:]), '%s: guard rows of %s were written' % (what, name)
    assert (after[0][n:] == SENTINEL).all() and (after[1][n:] == SENTINEL).all() and (after[3][n:] == SENTINEL).all()
    assert (after[2][n:] == GUARD_LEN).all()
    pixels, dx, dxlen, color = [a[:n] for a in after]
    bad = np.flatnonzero(pixels != want)
    assert len(bad) == 0, '%s: %d of %d pixels differ from the oracle, first ray %d: %08x, oracle %08x' % (
        what, len(bad), n, bad[0], pixels[bad[0]], want[bad[0]])
    _lists_equal((dx.view(np.float32), dxlen, color.view(np.float32)), wstate, what + ': engine vs oracle')
    miss = wstate[1] == 0
    assert (pixels[miss] == (bg & 0xFFFFFFFF)).all(), what + ': a ray that met nothing does not show the background'
    assert np.array_equal(dx[miss], before[1][:n][miss]) and np.array_equal(color[miss], before[3][:n][miss]), \
        what + ': the list rows of a ray that met nothing were written'


def _run_bundle(ctx, scene, calls, oracle_results, what):
    geometry, packed, gg = scene
    n = len(calls[0].o)
    rays = DeviceRays(ctx, n, calls[0].alpha_depth)
    have_ref = os.path.exists(REF_LIB)
    previous = None
    for k, (call, (want, wstate)) in enumerate(zip(calls, oracle_results)):
        before, after = rays.render(gg, call)
        _check_call(before, after, n, want, wstate, call.bg, '%s call %d' % (what, k))
        if have_ref:
            rpix, rstate = _ref_render(geometry, call.o, call.d, call.alpha_depth, call.bg, state=previous)
            assert np.array_equal(rpix, want), '%s call %d: oracle vs the compiled reference: %d pixels' % (what, k, (rpix != want).sum())
            _lists_equal(wstate, rstate, '%s call %d: oracle vs compiled reference' % (what, k))
        previous = wstate
    return rays


@gpu_test
@pytest.mark.parametrize('name', BUNDLE_NAMES)
def test_render_bundle_matches_the_oracle(name, ctx, device_scenes, oracle_mod, tiny_packed):
    scene, calls = _bundles()[name]
    _run_bundle(ctx, device_scenes(scene), calls, _want(oracle_mod, name, tiny_packed), name)


@gpu_test
def test_render_of_no_rays_touches_nothing(ctx, device_scenes):
    _, _, gg = device_scenes('tiny')
    rays = DeviceRays(ctx, 65, 3)
    call = Call(_zeros(65), _unit(np.random.default_rng(9), 65), 3, BG)
    for nthreads in (0, -1):
        before, after = rays.render(gg, call, nthreads=nthreads)
        for b, a in zip(before, after):
            assert np.array_equal(a, b)
        assert (after[0] == SENTINEL).all() and (after[1] == SENTINEL).all() and (after[3] == SENTINEL).all()
        assert (after[2][:65] == 0).all()


# ---- k_color_solids on its 256-thread block edges ------------------------------------------------------------------------
def _windows(ntriangles):
    out = []
    for first in (0, 1, 255):
        out += [(first, count) for count in (1, 255, 256, 257, ntriangles - first)]
    return out


@gpu_test
def test_color_solids_windows_and_the_render_after_one(ctx, device_scenes, oracle_mod):
    """chroma_color_solids over windows (first, count) around the kernel's block of 256, against NumPy, the whole colour array
    compared (so a triangle outside the window must keep its colour); a solid id at or beyond `nsolids` keeps its colour; the
    render reads the recoloured array by triangle id."""
    from chroma_amd import _lib
    from chroma_amd.gpu.tools import GPUArray
    geometry, packed, gg = device_scenes('shells')
    solid_id = np.asarray(geometry.solid_id)
    nt, nsolids = len(solid_id), 3
    before = np.asarray(geometry.colors, np.uint32)
    assert np.array_equal(gg.colors.get(), before)
    new = np.array([0x11AA0000, 0x8800BB00, 0xC00000CC], np.uint32)
    new_gpu = GPUArray(nsolids, np.uint32, ctx).set(new)

    def recolour(first, count, hit, ns):
        gg.colors.set(before)
        hit_gpu = GPUArray(nsolids, np.uint8, ctx).set(np.asarray(hit, np.uint8))
        _lib.check(ctx._lib.chroma_color_solids(ctx.handle, gg.handle, first, count, hit_gpu.ptr, new_gpu.ptr, ns))
        want = before.copy()
        sel = np.zeros(nt, bool)
        sel[first:first + count] = True
        sel &= (solid_id < ns) & np.asarray(hit, bool)[solid_id]
        want[sel] = new[solid_id[sel]]
        got = gg.colors.get()
        bad = np.flatnonzero(got != want)
        assert len(bad) == 0, 'window (%d, %d), hit %s, nsolids %d: %d colours differ, first triangle %d' % (first, count, hit, ns, len(bad), bad[0])
        return want
    for first, count in _windows(nt):
        want = recolour(first, count, (1, 0, 1), nsolids)
        changed = np.flatnonzero(want != before)
        assert len(changed) and changed.min() >= first and changed.max() < first + count
    recolour(0, 0, (1, 1, 1), nsolids)                                                  # no triangle: nothing
    # a solid id in the map at or beyond nsolids keeps its colour: the last sphere with arrays of two solids
    want = recolour(0, nt, (1, 1, 1), 2)
    assert np.array_equal(want[solid_id == 2], before[solid_id == 2]) and (want[solid_id < 2] != before[solid_id < 2]).all()
    gg.color_solids(np.array([True, True]), new[:2])                                  # the same through the method
    assert np.array_equal(gg.colors.get(), want)
    # the render after it reads colors[triangle id] of the recoloured array
    want = recolour(1, nt - 1, (0, 1, 1), nsolids)
    g2, packed2 = _recoloured(geometry, want)
    calls = _bundles()['colours'][1]
    results = _oracle_chain(oracle_mod, packed2, calls)
    assert (results[0][0] != _oracle_chain(oracle_mod, packed, calls)[0][0]).mean() > 0.5
    try:
        _run_bundle(ctx, (g2, packed2, gg), calls, results, 'colours after color_solids')
    finally:
        gg.colors.set(before)
